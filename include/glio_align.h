/* glio_align.h -- the frame the GNSS factors live in, estimated on the device: yaw_enu_local and anc_ecef of a glio_gnss_frame from a local trajectory and
 * the double-differenced pseudoranges along it.  The reference never estimates them: it reads them from the yaml and makes yaw_enu_local = 0 true by
 * starting the attitude from the data set's ground-truth heading (Estimator.cpp:1434-1448).  The result goes into glio_set_gnss /
 * glio_batch_set_small_factors unchanged.  Opt-in: no other entry point changes.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * MODEL.  For a frame (psi, a): R_el = ecef2rotation(a) Rz(psi); the receiver of a factor is at R_el (ratio P_i + (1 - ratio) P_j) + a; the rows, the 0.05
 * down-weighting against `threshold` BEFORE the whitening and the whitening by W are dd_psr_factor_20::Evaluate.  C(psi, a; threshold) = 1/2 sum r^2 over
 * all rows of all factors.  The positions P_k are constants (the caller's trajectory in the local frame); a factor's own `threshold` field is not read.
 *
 * STEP.  delta = (d_e, d_n, d_u, d_psi); a <- a + ecef2rotation(a) d_enu, psi <- psi + d_psi, and the rotation is recomputed at the new anchor after every
 * step.  The Jacobian LEAVES OUT the dependence of ecef2rotation(a) on a (relative size |P| / 6.4e6): the result is the FIXED POINT of this iteration,
 * not the exact minimiser of C.
 *
 * COARSE SEARCH.  n_hypotheses yaws psi_h = 2 pi h / H at the start anchor, every weight 1.  For each the 3 x 3 system in d_enu is solved and
 * c_h = 1/2 (r^T r - b^T (A^T A)^-1 b) is its reduced cost.  The lowest c_h wins, the LOWEST h on a tie; a hypothesis whose system has a pivot that is not
 * positive and finite is left out (its cost reads +INFINITY).  n_hypotheses = 0 skips the search and refines from the caller's yaw.
 *
 * REFINEMENT.  One round per threshold, in list order; each round is Gauss-Newton on the 4 x 4 system, unknowns ordered (d_e, d_n, d_u, d_psi), so the last
 * Cholesky pivot s is the yaw's Schur complement.  A round ends when |d_psi| <= yaw_tolerance and |d_enu| <= pos_tolerance, or after
 * max_iterations_per_round.  psi is wrapped to (-pi, pi] at the end.
 *
 * OBSERVABILITY.  s <= 1e-9 H_psipsi at any linearisation, a pivot that is not positive and finite, or no hypothesis left in: status UNOBSERVABLE and `out`
 * equals `start` bit for bit.  Otherwise yaw_sigma = 1 / sqrt(s) at the LAST linearisation (unit-variance rows).  max_yaw_sigma > 0 turns a delivered
 * result with a larger yaw_sigma into status WEAK.
 *
 * INFO.  round_cost / round_downweighted are those of the round's last linearisation (the point its last step left from).  covariance is the 4 x 4 inverse
 * of J^T J at the last linearisation of the solve, rows of unit variance, order (e, n, u, psi).
 *
 * BITS.  No atomic takes part in any sum; every partial sum has a fixed place and order that depend on the factors' row counts and H only.  The result is
 * bit-identical from run to run.
 *
 * ONE host wait per solve, at the end: the search, every round and the terminations are decided on the device; launches behind the deciding iteration
 * return at once.  REFUSALS are GLIO_E_ARG and leave `out`, the factors, the positions and the options as they were.  A glio_align owns one HIP stream
 * and is not thread-safe. */
#ifndef GLIO_ALIGN_H_
#define GLIO_ALIGN_H_
#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLIO_ALIGN_MAX_ROUNDS 8
#define GLIO_ALIGN_MAX_HYPOTHESES 4096
#define GLIO_ALIGN_MAX_ITERATIONS 64

enum { GLIO_ALIGN_OK = 0, GLIO_ALIGN_WEAK = 1, GLIO_ALIGN_UNOBSERVABLE = 2 };

typedef struct glio_align glio_align;

typedef struct glio_align_opts {
    int32_t n_hypotheses;              /* H, 0 .. GLIO_ALIGN_MAX_HYPOTHESES; default 72 */
    int32_t n_rounds;                  /* 1 .. GLIO_ALIGN_MAX_ROUNDS; default 4 */
    int32_t max_iterations_per_round;  /* 1 .. GLIO_ALIGN_MAX_ITERATIONS; default 10 */
    int32_t reserved_;
    double  thresholds[GLIO_ALIGN_MAX_ROUNDS];   /* default {1e9, 10, 8, 6}: the batch stage's schedule (Estimator.cpp:2764-2767) */
    double  yaw_tolerance;             /* rad; default 1e-8 */
    double  pos_tolerance;             /* m; default 1e-6 */
    double  max_yaw_sigma;             /* rad, 0 = none */
} glio_align_opts;

typedef struct glio_align_info {
    int32_t status;                    /* GLIO_ALIGN_* */
    int32_t winner;                    /* the winning hypothesis, -1 without a search */
    int32_t n_rows;
    int32_t n_rounds;                  /* rounds that ran */
    int32_t round_iterations[GLIO_ALIGN_MAX_ROUNDS];
    int32_t round_downweighted[GLIO_ALIGN_MAX_ROUNDS];
    double  coarse_cost;               /* c of the winner (0 without a search) */
    double  runner_up_cost;            /* the second lowest c (+INFINITY when no second hypothesis was left in, 0 without a search) */
    double  round_cost[GLIO_ALIGN_MAX_ROUNDS];
    double  yaw_sigma;                 /* 1 / sqrt(s); 0 when UNOBSERVABLE */
    double  yaw_schur;                 /* s at the last linearisation */
    double  h_yaw_yaw;                 /* H_psipsi at the last linearisation */
    double  covariance[16];            /* (J^T J)^-1, row major, order (e, n, u, psi); zeros when UNOBSERVABLE */
} glio_align_info;

void glio_align_opts_default(glio_align_opts* o);
/* sizeof() of glio_align_opts, glio_align_info; returns how many there are (2) */
int glio_align_struct_sizes(int32_t* out, int n);

/* GLIO_E_ARG: max_factors outside [1, 2^22], max_positions outside [1, 2^24], a bad device, a null pointer */
int glio_align_create(int device, int max_factors, int max_positions, glio_align** out);
void glio_align_destroy(glio_align* al);
/* GLIO_E_ARG (the options stay): n_hypotheses, n_rounds (more than 8 thresholds) or max_iterations_per_round out of range, a threshold that is not positive
 * (NaN included), a tolerance or max_yaw_sigma that is negative or not finite */
int glio_align_set_opts(glio_align* al, const glio_align_opts* opts);
/* slot_i / slot_j index the position table, as in glio_batch_set_small_factors.  The factors are copied to the device and unpacked there into row
 * records, one per double difference; a factor's rows stay in one workgroup.  GLIO_E_ARG (the previous factors stay): n_dd outside [1, max_factors], a
 * slot outside [0, max_positions), n_sat outside [2, GLIO_DD_MAX_SAT], a master outside [0, n_sat), a null pointer */
int glio_align_set_factors(glio_align* al, int n_dd, const glio_dd_psr* dd);
/* position k is base[k * stride_doubles .. + 2]: a [n][7] pose table is passed as it lies with stride 7.  GLIO_E_ARG (the previous table stays): n outside
 * [1, max_positions], stride_doubles < 3, a null pointer */
int glio_align_set_positions(glio_align* al, int n, const double* base, int stride_doubles);
/* the estimate, from `start` (any anchor within the drive's neighbourhood).  info may be null.  GLIO_E_ARG (`out` untouched): no factors, no positions, a
 * factor's slot outside the position table, a start that is not finite, a null pointer */
int glio_align_solve(glio_align* al, const glio_gnss_frame* start, glio_gnss_frame* out, glio_align_info* info);
/* C(frame; threshold) and the number of down-weighted rows: the reference's DD cost at a given frame.  n_downweighted may be null. */
int glio_align_cost(glio_align* al, const glio_gnss_frame* frame, double threshold, double* cost, int32_t* n_downweighted);
/* the reduced costs of the last solve's search into costs [capacity]; *n = how many there are, the H of that solve (costs may be null to ask for it).
 * GLIO_E_ARG for a capacity below it (nothing written), GLIO_E_STATE before a solve with n_hypotheses > 0 */
int glio_align_read_coarse(glio_align* al, double* costs, int capacity, int32_t* n);
/* device time of the last solve or cost call (HIP events), ms; GLIO_E_STATE before the first */
int glio_align_last_device_ms(glio_align* al, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_ALIGN_H_ */

/* glio_batch_cov.h -- the marginal covariance of every keyframe of the batch stage (Estimator::optimizeBatchWithLandMark, glio_batch_*), on the
 * device: the B x B diagonal blocks of H^-1 and the blocks (k, k + 1), by a selected inversion down the elimination tree of the block cyclic reduction
 * that the trust-region solve factors with.  The normal matrix never leaves the device.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * THE MATRIX.  H is exactly the matrix glio_batch_solve_tr2 linearises at (poses, speed_bias): plane constraints (or their moment records), delta_q,
 * relative-pose factors, DD pseudoranges at the threshold currently set and, when set, the ImuFactor chain.  Unscaled: no mu D^2, no lambda, no 1e-12
 * shift.  It is the H whose diagonal glio_batch_linearize_full returns.  Coordinates are those of oracle/orc_batch2.c:20: keyframe-major, per keyframe
 * [dt3 dtheta3 | dv3 dba3 dbg3] (B = 15 with the chain, 6 without).  theta is Ceres' left half-angle tangent exactly as glio_cov.h describes it, so
 * glio::pose3Covariance / sliding.pose3_covariance apply unchanged to the leading 6 x 6 of a block.
 *
 * ANCHOR.  Without GNSS factors H is singular (the gauge: 6 dimensions for the pose problem, position and yaw with the chain), so a covariance exists
 * only relative to something held fixed.  anchor_keyframe = a >= 0 holds the six POSE columns of keyframe a constant -- the covariance conditioned on
 * that pose; its speed / bias columns stay free.  Those six rows and columns are left out of the system (in the operator: identity block, zero
 * couplings, as a padding keyframe; no large diagonal) and are reported as exact zeros in diag[a], next[a - 1] and next[a].  -1: none.
 *
 * NOT POSITIVE DEFINITE.  The matrix is factored in fp64 after Jacobi scaling S H S, S = diag(1 / sqrt(H_kk)), with no regularisation.  A diagonal
 * entry outside the anchor that is not positive and finite, or a pivot that is not, gives GLIO_E_NUMERIC; bad_keyframe names the keyframe (the first
 * one of the super-block, for a pivot) met first in elimination order, and diag / next are untouched.  A gauge left free ends this way, not in numbers.
 * min_pivot / max_pivot are over the squared diagonal of the factor of the SCALED matrix (identity columns of the anchor and of padding included).
 *
 * REFUSALS.  GLIO_E_ARG: a null stage, poses or diag; an anchor outside [-1, K); speed_bias null with the chain set; a stage whose band the block
 * cyclic reduction does not cover.  GLIO_E_STATE: a sharded stage (world > 1).  A refusal touches no buffer another entry point reads.
 *
 * BITS.  Every sum is in a fixed order, no atomic takes part in a value.  Results are bit-identical from run to run; diag[k] is symmetric to the bit
 * (the lower triangle is computed and mirrored); next may be NULL without changing a bit of diag.
 *
 * NO SIDE EFFECT.  The call linearises as glio_batch_linearize_full does and factors in the solver's workspaces, which every solve fills anew: a
 * glio_batch_solve_tr2 / _solve_tr / _linearize_full after it returns the bits it returns without it, with or without valid moment records.  What
 * the inversion itself needs is allocated at the first call: a stage that never asks allocates nothing.  ONE host wait, at the end; the result
 * goes through pinned memory and is handed over only if no pivot failed.  Not thread-safe against other calls on the same stage. */
#ifndef GLIO_BATCH_COV_H_
#define GLIO_BATCH_COV_H_
#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct glio_batch_cov_info {
    int32_t n;            /* B K */
    int32_t B;            /* 15 with the IMU chain, 6 without */
    int32_t anchor;       /* as passed */
    int32_t bad_keyframe; /* -1, or the keyframe in whose super-block the first pivot was not positive and finite */
    int32_t levels;       /* elimination levels walked */
    int32_t pad_;
    double  min_pivot, max_pivot;
} glio_batch_cov_info;

/* sizeof() of glio_batch_cov_info; returns how many there are (1) */
int glio_batch_cov_struct_sizes(int32_t* out, int n);
/* diag [K][B][B]: block (k, k) of H^-1;  next [K-1][B][B] (may be NULL): block (k, k+1);  row major.  info may be NULL. */
int glio_batch_covariance(glio_batch* b, const double* poses /*[K][7]*/, const double* speed_bias /*[K][9] or NULL*/,
                          int anchor_keyframe /* -1: none */, double* diag, double* next, glio_batch_cov_info* info);
/* device time of the last call from the start of the linearisation to the result's copy (HIP events), ms; GLIO_E_STATE before the first */
int glio_batch_covariance_last_device_ms(glio_batch* b, float* ms);
/* the same by stage, for timing: linearise, factor, down-sweep (with the triangular solves and the pre-eliminated blocks), gather, copy */
int glio_batch_covariance_last_stage_ms(glio_batch* b, float* ms5);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_BATCH_COV_H_ */

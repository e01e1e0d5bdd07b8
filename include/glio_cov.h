/* glio_cov.h -- the marginal covariance of the window's estimate, on the device: selected rows and columns of H^-1 with H = J^T J the matrix
 * glio_linearize returns (after loss correction and local parameterisation, unscaled).  What ceres::Covariance gives a Ceres user on the same problem
 * and what the reference's loosely-coupled mode reads from isam->marginalCovariance (Estimator.cpp:1937-1938, :4579).
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * COORDINATES.  The columns are those of glio_linearize (oracle/orc_solver.c:160-190): slot s has its translation increment at 15 s .. 15 s + 2, the
 * three tangent coordinates of its quaternion at 15 s + 3 .. 15 s + 5, speed / accelerometer bias / gyroscope bias at 15 s + 6 .. 15 s + 14;
 * clock-drift epoch e is at 15 W + e.  The quaternion tangent is that of Ceres' QuaternionParameterization (orc_quat_plus): the increment d multiplies on
 * the LEFT, q' = (cos |d|, sin |d| d / |d|) * q, so d is HALF a rotation vector and it is expressed in the world frame (R(q') = Exp(2 d) R(q)).  The
 * 3 x 3 rotation block is therefore a quarter of the covariance of the world-frame rotation vector; glio::pose3Covariance / sliding.pose3_covariance
 * map a slot's 6 x 6 pose block to GTSAM's Pose3 order and chart.
 *
 * FREE COLUMNS.  A column k with H_kk == 0 exactly has a zero column in J, so row and column k of H are zero.  It is left out of the system, as a
 * constant parameter block would be (the speed and biases of a front-end context: window = 1, LiDAR factors only; an epoch no Doppler row touches).  If
 * such a column is asked for, its diagonal entry is +INFINITY and its off-diagonal entries are 0 -- "no information", never "certain" -- and it is counted
 * in n_free_asked.
 *
 * NOT POSITIVE DEFINITE.  The remaining matrix is factored H = L L^T in fp64 with no regularisation.  A pivot that is not positive and finite gives
 * GLIO_E_NUMERIC, bad_pivot names its column (in the coordinates above) and `out` is untouched.
 *
 * REFUSALS.  GLIO_E_ARG for m outside [1, n], a column outside [0, n), a column listed twice, a slot outside [0, W) or listed twice, a null pointer.  A
 * refusal leaves `out` and every device buffer another entry point reads untouched.
 *
 * BITS.  Sigma_SS = Y^T Y with Y = L^-1 E_S: one forward substitution per asked column and one fixed-order sum per entry, no atomic anywhere.  The result
 * is bit-identical from run to run, symmetric to the bit, and the bits of entry (i, j) depend on H, i and j only -- not on which other columns were asked
 * or in what order.
 *
 * NO SIDE EFFECT.  The call finishes a pending asynchronous marginalization and pending searches exactly as glio_linearize does and, like it, linearises
 * into the context's scratch; a glio_solve, glio_marginalize_keep or glio_linearize after it returns the bits it returns without it.  ONE host wait, at
 * the end; H never leaves the device.  The workspace (a copy of H, its factor, Y and the result) is allocated at the first call: a context that never
 * asks allocates nothing.  Not thread-safe against other calls on the same context. */
#ifndef GLIO_COV_H_
#define GLIO_COV_H_
#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct glio_cov_info {
    int32_t n;             /* 15 W + n_ddt */
    int32_t n_free;        /* columns no factor touches, left out of the system */
    int32_t n_free_asked;  /* how many of the asked columns are free */
    int32_t bad_pivot;     /* -1, or the first column whose pivot was not positive and finite */
    double  min_pivot, max_pivot;   /* of L's diagonal squared, over the columns factored (0, 0 when none was) */
} glio_cov_info;

/* sizeof() of glio_cov_info; returns how many there are (1) */
int glio_cov_struct_sizes(int32_t* out, int n);
/* out [m][m] row major: rows and columns cols[0..m-1] of H^-1 at `state`, H exactly the matrix glio_linearize gives.  info may be null. */
int glio_covariance_columns(glio_ctx* ctx, const glio_state* state, int m, const int32_t* cols, double* out, glio_cov_info* info);
/* convenience: the columns 15 s .. 15 s + 14 of every listed slot, in list order; out [15 n_slots][15 n_slots] */
int glio_covariance_slots(glio_ctx* ctx, const glio_state* state, int n_slots, const int32_t* slots, double* out, glio_cov_info* info);
/* device time of the last covariance call from the start of the linearisation to the result's copy (HIP events), ms; GLIO_E_STATE before the first */
int glio_covariance_last_device_ms(glio_ctx* ctx, float* ms);
/* for tests and timing, like glio_debug_chol_solve: the same kernels on a caller's matrix (n x n row major, only the lower triangle is read,
 * n <= the context's 15 W + max_ddt_epochs) */
int glio_debug_covariance_of(glio_ctx* ctx, int n, const double* H, int m, const int32_t* cols, double* out, glio_cov_info* info);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_COV_H_ */

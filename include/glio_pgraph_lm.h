/* glio_pgraph_lm.h -- the damped solve of the pose graph (glio_pgraph, include/glio_hip.h).  Included by glio_hip.h, inside its extern "C"; include that.
 * (A header of its own because the list of glio_pgraph_* entry points that glio_hip.h itself declares is pinned by tests/test_pose_graph_abi.py.)
 *
 * glio_pgraph_solve is undamped Gauss-Newton: a step that raises the error ends it CONVERGED with the worse estimate kept.  glio_pgraph_solve_damped is the
 * same batch estimate with a globalisation strategy: Ceres 1.14's LevenbergMarquardtStrategy in its monotonic trust-region loop (UNPINNED: restated from the
 * published behaviour), on the pose graph's own normal equations, retraction and error E = 1/2 |r|^2, without Jacobi scaling.  Per trial at the estimate x, with
 * H = J^T J, g = J^T r and the radius rho:
 *   step        d_i = clamp(H_ii, min_diagonal, max_diagonal) from the COMPLETE diagonal of a node (chain factors, prior, GPS factors, every loop edge that ends
 *               there); (H + diag(d) / rho) delta = -g by the same exact Cholesky in the same fixed order as glio_pgraph_solve
 *   model       m = -(g^T delta + 1/2 delta^T H delta) = 1/2 sum_i delta_i (d_i delta_i / rho - g_i)
 *   invalid     a non-positive pivot, or m that is not positive and finite: the trial counts as rejected
 *   candidate   x_c = x [+] delta, E_c its error, gain = (E - E_c) / m
 *   accept      gain > min_relative_decrease: x = x_c; rho = min(max_radius, rho / max(1/3, 1 - (2 gain - 1)^3)); the decrease factor back to 2; then the object's
 *               error test on this decrease: E_c <= 0, or (E - E_c) / E <= relative_error_tol, or E - E_c <= absolute_error_tol ends the solve CONVERGED
 *   reject      x untouched; rho /= decrease factor; decrease factor *= 2; rho <= min_radius ends the solve GLIO_PGRAPH_MIN_RADIUS
 *   limit       every trial counts; at max_trials the termination is ITERATION_LIMIT
 * Every solve starts from initial_radius with the decrease factor 2.  CONTRACT: final_error <= initial_error, always; the pose table after the call is the last
 * accepted estimate (the estimate the solve started from when no trial was accepted).  The trial loop is decided on the device and enqueued ahead as the
 * Gauss-Newton loop is (one host wait, or two); no atomic takes part in a sum: two runs give the same bits.  glio_pgraph_marginal_covariance stays undamped. */
#ifndef GLIO_PGRAPH_LM_H_
#define GLIO_PGRAPH_LM_H_

void glio_pgraph_lm_opts_default(glio_pgraph_lm_opts* o);
/* sizeof() of glio_pgraph_lm_opts, glio_pgraph_lm_info; returns how many there are (2) */
int glio_pgraph_lm_struct_sizes(int32_t* out, int n);
/* lm_opts null: the defaults.  info and lm_info may be null.  info is filled as by glio_pgraph_solve: iterations = trials, stage_ms = the first trial.
 * GLIO_E_ARG, and nothing changes: a radius or a diagonal bound that is not finite and positive; min_radius > initial_radius or initial_radius > max_radius;
 * min_diagonal > max_diagonal; min_relative_decrease outside [0, 1); max_trials < 0; no node; neither a prior nor a GPS factor.
 * A solve whose every trial is invalid ends MIN_RADIUS or ITERATION_LIMIT with the estimate it started from in place. */
int glio_pgraph_solve_damped(glio_pgraph* pg, const glio_pgraph_lm_opts* lm_opts, glio_pgraph_info* info, glio_pgraph_lm_info* lm_info);
/* rows [first, first + n) of the last damped solve's per-trial history: E tried (E itself for an invalid trial), the radius used, m, and 1 accepted /
 * 0 rejected / -1 invalid.  GLIO_E_ARG for a range outside [0, trials). */
int glio_pgraph_lm_history(glio_pgraph* pg, int first, int n, double* out /* [n][4] */);

#endif /* GLIO_PGRAPH_LM_H_ */

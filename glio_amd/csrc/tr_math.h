// tr_math.h -- the scalar rule of Ceres 1.14's trust-region minimiser (trust_region_minimizer.cc, dogleg_strategy.cc, levenberg_marquardt_strategy.cc),
// one definition each: its defaults as named constants and its formulas.  Formulas only: who calls them, with how many lanes and through which memory,
// is the caller's business (the window's state machine and tails in solver_kernels.hip, the batch stage's k_bt_* kernels, the trajectory's loop in
// k_traj_gap, the pose graph's k_pg_lm_decide).  Every function takes the including file's FMA-contraction setting.  Compiles for the device and, without
// any HIP header, with a plain host compiler (glio_amd/host/host_tr_math_test.cpp); what needs device code is in tr_math_device.h.  The oracle and the
// tests' restatements do NOT include this file.
// Scalars go in and come out by value wherever one result is enough: a reference into a caller's status record moved that kernel's register allocation.
#pragma once
#include <math.h>
#ifdef __HIPCC__
#define TR_FN __host__ __device__ __forceinline__
#else
#define TR_FN inline
#endif

// ---- ceres::Solver::Options defaults (1.14) and the strategies' own constants
constexpr double TR_INITIAL_RADIUS = 1e4, TR_MAX_RADIUS = 1e16, TR_MIN_RADIUS = 1e-32, TR_MIN_RELATIVE_DECREASE = 1e-3;
constexpr double TR_FUNCTION_TOLERANCE = 1e-6, TR_GRADIENT_TOLERANCE = 1e-10, TR_PARAMETER_TOLERANCE = 1e-8;
constexpr double TR_MIN_MU = 1e-8, TR_MAX_MU = 1.0, TR_MU_INCREASE = 10.0;               // DoglegStrategy: mu of (Hs + mu D^2), x 10 on a failed solve
constexpr double TR_MU_DECREASE_NUM = 2.0, TR_MU_DECREASE_DEN = 10.0;                    //   and mu = max(min_mu, 2 mu / 10) on an accepted step
constexpr double TR_SHRINK_BELOW = 0.25, TR_SHRINK = 0.5, TR_GROW_ABOVE = 0.75, TR_GROW = 3.0;          // the dogleg's radius rule
constexpr double TR_MIN_DIAGONAL = 1e-6, TR_MAX_DIAGONAL = 1e32;                         // the clip of diag(Hs)
constexpr double TR_LM_DECREASE_FACTOR = 2.0, TR_LM_DECREASE_GROWTH = 2.0;               // LevenbergMarquardtStrategy: reset on acceptance, x 2 per rejection
constexpr int TR_MAX_INVALID_STEPS = 5;                                                  // max_num_consecutive_invalid_steps
// termination codes: GLIO_TERM_* and GLIO_TRAJ_* 0 .. 5 (asserted where those headers are visible); TR_GO_ON: the next iteration starts
enum { TR_GO_ON = -1, TR_NO_CONVERGENCE = 0, TR_FUNCTION_TOL = 1, TR_PARAMETER_TOL = 2, TR_GRADIENT_TOL = 3, TR_MIN_RADIUS_REACHED = 4, TR_FAILURE = 5 };

// ---- Jacobi scale and the diagonal clip.  The ternary lets a NaN through, the min/max form (the trajectory's) turns it into the lower bound.
TR_FN double tr_jacobi_scale(const double h) { return 1.0 / (1.0 + sqrt(h)); }
TR_FN double tr_clip_diagonal(const double d, const double lo = TR_MIN_DIAGONAL, const double hi = TR_MAX_DIAGONAL) { return d < lo ? lo : (d > hi ? hi : d); }
TR_FN double tr_clip_diagonal_minmax(const double d) { return fmin(fmax(d, TR_MIN_DIAGONAL), TR_MAX_DIAGONAL); }

// ---- step selection: step (D-space) = ca * grad + cb * gn, from gg = |grad|^2, nn = |gn|^2, gd = grad . gn (gnorm, gnn: their roots) and the Cauchy
// step length alpha.  snorm: the step's norm where it is known in closed form, -1 where the caller takes it from the step itself.
// squared_roots: the trajectory's arithmetic -- gnorm * gnorm and gnn * gnn, the squares of the rounded roots, stand where the others use the sums gg, nn
// (formed here, where they are used, and not at the call: that keeps the instruction order of its kernel).
TR_FN void tr_dogleg_coeffs(const bool lm, const double gg, const double nn, const double gd, const double gnorm, const double gnn,
                            const double radius, const double alpha, double& ca, double& cb, double& snorm, const bool squared_roots = false) {
    if (lm) { ca = 0.0; cb = 1.0; snorm = gnn; }        // Levenberg-Marquardt: the damped step itself
    else if (gnn <= radius) { ca = 0.0; cb = 1.0; snorm = gnn; }
    else if (gnorm * alpha >= radius) { ca = -(radius / gnorm); cb = 0.0; snorm = radius; }
    else {
        const double b_dot_a = -alpha * gd;
        const double a_sq = alpha * alpha * (squared_roots ? gnorm * gnorm : gg);
        const double b_minus_a_sq = (squared_roots ? gnn * gnn : nn) - 2 * b_dot_a + a_sq;
        const double c = b_dot_a - a_sq;
        const double d = sqrt(c * c + b_minus_a_sq * (radius * radius - a_sq));
        const double beta = (c <= 0) ? (d - c) / b_minus_a_sq : (radius * radius - a_sq) / (d + c);
        ca = -alpha * (1.0 - beta); cb = beta; snorm = -1.0;
    }
}
// one element of the step and of the model cost change -(gs . step_s + step_s^T Hs step_s / 2):  sv the D-space step, step_s = sv / D, w = S step_s;
// Hs step_s = ca * Hs (g~/D) - cb * Hs y with Hs (g~/D) = S H u = S t and Hs y = S g - mu D^2 y -- no other matrix pass.  lin, quad: the element's terms.
TR_FN void tr_step_element(const double ca, const double cb, const double grad, const double gn, const double diag, const double scale, const double g,
                           const double t, const double y, const double mu, double& sv, double& step_s, double& w, double& lin, double& quad) {
    sv = ca * grad + cb * gn;
    step_s = sv / diag;
    w = scale * step_s;
    const double gs = scale * g;
    const double hs_step = ca * (scale * t) - cb * (gs - mu * diag * diag * y);
    lin = gs * step_s;
    quad = step_s * hs_step;
}

// ---- the candidate's verdict (TrustRegionMinimizer): the two convergence tests, then the step quality against min_relative_decrease
TR_FN bool tr_parameter_converged(const double step_norm, const double x_norm, const double ptol) { return step_norm <= ptol * (x_norm + ptol); }
TR_FN bool tr_function_converged(const double cost, const double ccost, const double ftol) { return fabs(cost - ccost) <= ftol * cost; }
TR_FN double tr_step_quality(const double cost, const double ccost, const double mcc) { return (cost - ccost) / mcc; }
TR_FN bool tr_step_accepted(const double quality, const double min_relative_decrease) { return quality > min_relative_decrease; }     // (a NaN is rejected)
// DoglegStrategy::StepAccepted / StepRejected: the new radius and the new mu
TR_FN double tr_dogleg_accepted_radius(const double quality, const double step_norm, double radius) {
    if (quality < TR_SHRINK_BELOW) radius *= TR_SHRINK;
    if (quality > TR_GROW_ABOVE) radius = fmax(radius, TR_GROW * step_norm);
    return radius;
}
TR_FN double tr_mu_accepted(const double mu) { return fmax(TR_MIN_MU, TR_MU_DECREASE_NUM * mu / TR_MU_DECREASE_DEN); }
TR_FN double tr_dogleg_rejected_radius(const double radius) { return radius * TR_SHRINK; }
// LevenbergMarquardtStrategy::StepAccepted (the decrease factor goes back to TR_LM_DECREASE_FACTOR) / StepRejected.  cube = (2 quality - 1)^3 in the
// caller's own spelling, the window's pow or the pose graph's products: two named variants, their device results have not been shown equal
TR_FN double tr_cube_pow(const double c) { return pow(c, 3); }
TR_FN double tr_cube_mul(const double c) { return c * c * c; }
TR_FN double tr_lm_accepted_radius(double radius, const double cube, const double max_radius) {
    radius = radius / fmax(1.0 / 3.0, 1.0 - cube);
    return fmin(max_radius, radius);
}
TR_FN void tr_lm_rejected(double& radius, double& decrease_factor) { radius /= decrease_factor; decrease_factor *= TR_LM_DECREASE_GROWTH; }
// an invalid step (failed linear solve or model cost change <= 0) is counted by the caller; true: it is the fifth in a row, the solve ends with FAILURE.
// What else the step costs (mu x 10, or the LM rejection) and whether the fifth still pays it is the caller's record.
TR_FN bool tr_invalid_limit(const int invalid_in_a_row) { return invalid_in_a_row >= TR_MAX_INVALID_STEPS; }
// FinalizeIterationAndCheckIfMinimizerCanContinue in Ceres' order: time / max_iterations, gradient tolerance, min radius; on TR_GO_ON the caller
// counts the iteration (++iteration)
TR_FN int tr_iteration_gate(const int iteration, const int max_iterations, const bool out_of_time, const double grad_max, const double gtol, const double radius,
                            const double min_radius) {
    if (iteration >= max_iterations || out_of_time) return TR_NO_CONVERGENCE;
    if (grad_max <= gtol) return TR_GRADIENT_TOL;
    if (radius <= min_radius) return TR_MIN_RADIUS_REACHED;
    return TR_GO_ON;
}

// tr_math_device.h -- the device-only part of the trust-region rule (tr_math.h): what needs the device's quaternion routines or the C-ABI's codes.
// Included by the kernel files only; tr_math.h itself stays free of HIP headers for every host program that includes it.
#pragma once
#include "glio_device.h"
#include "tr_math.h"
static_assert(GLIO_TERM_NO_CONVERGENCE == TR_NO_CONVERGENCE && GLIO_TERM_FUNCTION_TOL == TR_FUNCTION_TOL && GLIO_TERM_PARAMETER_TOL == TR_PARAMETER_TOL &&
              GLIO_TERM_GRADIENT_TOL == TR_GRADIENT_TOL && GLIO_TERM_MIN_RADIUS == TR_MIN_RADIUS_REACHED && GLIO_TERM_FAILURE == TR_FAILURE, "one set of codes");
// device only: the rotation part of the gradient max norm | q - Plus(q, -g_rot) |_inf, joined to the running maximum m
__device__ __forceinline__ double tr_grad_max_rot(const double q[4], const double g_rot[3], double m) {
    const double d[3] = {-g_rot[0], -g_rot[1], -g_rot[2]};
    double qn[4];
    d_quat_plus(q, d, qn);
    for (int c = 0; c < 4; ++c) m = fmax(m, fabs(q[c] - qn[c]));
    return m;
}

// factor_math.h -- the reference's factor formulas, one device definition each.  Formulas only: who calls them, with how many lanes and through
// which memory, is the caller's business (the window's roles in factor_kernels.hip, the batch stage's k_small_eval, the single-factor evaluators of
// eval_kernels.hip).  The GNSS formulas round like the reference's scalar build (no FMA contraction: they difference ranges of ~2.6e7 m), so each of
// them carries the pragma in its own body; the prior and the quaternion-difference formulas take the including file's setting.
#pragma once
#include "glio_device.h"

// ------------------------------------------------------------------------------------------------
// DD pseudorange, dd_psr_factor_20::Evaluate (dd_psr_factor.hpp:25-171)
// ------------------------------------------------------------------------------------------------
// the receiver's ECEF position between the two keyframes: R_ecef_local (ratio Pi + (1 - ratio) Pj) + anchor
__device__ __forceinline__ void fm_dd_position(const double ratio, const double Pi[3], const double Pj[3], const double R[9], const double anc[3], double Pe[3]) {
#pragma clang fp contract(off)
    double lp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lp[k] = ratio * Pi[k] + (1.0 - ratio) * Pj[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Pe[k] = R[3 * k] * lp[0] + R[3 * k + 1] * lp[1] + R[3 * k + 2] * lp[2] + anc[k];
}
// satellite i seen from Pe: |d_u|, |d_r|, psr_u - psr_r and the line of sight in the local frame, e^T R
__device__ __forceinline__ void fm_dd_satellite(const glio_dd_psr& F, const int i, const double Pe[3], const double R[9], double& r_u, double& r_r, double& obs, double e[3]) {
#pragma clang fp contract(off)
    double d_u[3], d_r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d_u[k] = F.user_sat_pos[i][k] - Pe[k]; d_r[k] = F.ref_sat_pos[i][k] - F.station[k]; }
    const double ru = sqrt(d_dot3_nc(d_u, d_u));          // (a local: the outputs may be in LDS)
    r_u = ru; r_r = sqrt(d_dot3_nc(d_r, d_r));
    obs = F.user_psr[i] - F.ref_psr[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[c] = (d_u[0] * R[c] + d_u[1] * R[3 + c] + d_u[2] * R[6 + c]) / ru;
}
// the row of satellite i against the master m, before the whitening: the down-weighted residual (:99-102) and its Jacobians wrt Pi, Pj
__device__ __forceinline__ void fm_dd_row(const double ratio, const double threshold, const double ru_i, const double rr_i, const double obs_i, const double e_i[3],
                                          const double ru_m, const double rr_m, const double obs_m, const double e_m[3], double& raw, double Jri[3], double Jrj[3]) {
#pragma clang fp contract(off)
    const double est = (ru_i - rr_i) - (ru_m - rr_m);
    const double obs = obs_i - obs_m;
    const double wgt = fabs(est - obs) > threshold ? 0.05 : 1.0;
    raw = wgt * (est - obs);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double ei = e_i[c], em = e_m[c];
        Jri[c] = (-ei * wgt * ratio) - (-em * wgt * ratio);
        Jrj[c] = (-ei * wgt * (1.0 - ratio)) - (-em * wgt * (1.0 - ratio));
    }
}
// row i of residual = W r, J = W J (:151-167), W the nw x nw whitening matrix
__device__ __forceinline__ void fm_dd_whiten(const double* W, const int i, const int nw, const double* raw, const double* Jri, const double* Jrj, double& sr, double si[3], double sj[3]) {
#pragma clang fp contract(off)
    sr = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { si[k] = 0; sj[k] = 0; }
    for (int b = 0; b < nw; ++b) {
        const double wv = W[i * nw + b];
        sr += wv * raw[b];
#pragma unroll
        for (int k = 0; k < 3; ++k) { si[k] += wv * Jri[b * 3 + k]; sj[k] += wv * Jrj[b * 3 + k]; }
    }
}

// ------------------------------------------------------------------------------------------------
// Doppler row, tcdopplerFactor with its analytic Jacobians (dopp_factor.hpp:24-75): the residual, 1 / var and the gradients wrt the interpolated
// position and velocity in the local frame.  The callers scale them by ratio / (1 - ratio) and 1 / var, and apply the loss.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fm_doppler_row(const double ratio, const double var, const double sat_pos[3], const double sat_vel[3], const double lever_arm[3],
                                               const double sv_ddt, const double doppler, const double lamda, const double Rf[9], const double Pi[3], const double Vi[3],
                                               const double Pj[3], const double Vj[3], const double anc[3], const double ddt,
                                               double& res, double& iv, double gPl[3], double gVl[3]) {
#pragma clang fp contract(off)
    const double OMG = 7.2921151467e-5, CLIGHT = 2.99792458e8;
    double lp[3], lv[3], Pe[3], Ve[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lp[k] = ratio * Pi[k] + (1.0 - ratio) * Pj[k] + lever_arm[k];
        lv[k] = ratio * Vi[k] + (1.0 - ratio) * Vj[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Pe[k] = Rf[3 * k] * lp[0] + Rf[3 * k + 1] * lp[1] + Rf[3 * k + 2] * lp[2] + anc[k];
        Ve[k] = Rf[3 * k] * lv[0] + Rf[3 * k + 1] * lv[1] + Rf[3 * k + 2] * lv[2];
    }
    const double d[3] = {sat_pos[0] - Pe[0], sat_pos[1] - Pe[1], sat_pos[2] - Pe[2]};
    const double rho = sqrt(d_dot3_nc(d, d));
    const double eh[3] = {d[0] / rho, d[1] / rho, d[2] / rho};
    const double sag = OMG / CLIGHT * (sat_vel[0] * Pe[1] + sat_pos[0] * Ve[1] - sat_vel[1] * Pe[0] - sat_pos[1] * Ve[0]);
    const double av[3] = {sat_vel[0] - Ve[0], sat_vel[1] - Ve[1], sat_vel[2] - Ve[2]};
    const double ae = d_dot3_nc(av, eh);
    res = (ae + sag + ddt - sv_ddt + doppler * lamda) / var;
    double gP[3], gV[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { gP[k] = -(av[k] - ae * eh[k]) / rho; gV[k] = -eh[k]; }
    gP[0] += OMG / CLIGHT * (-sat_vel[1]); gP[1] += OMG / CLIGHT * sat_vel[0];
    gV[0] += OMG / CLIGHT * (-sat_pos[1]); gV[1] += OMG / CLIGHT * sat_pos[0];
    iv = 1.0 / var;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gPl[c] = gP[0] * Rf[c] + gP[1] * Rf[3 + c] + gP[2] * Rf[6 + c];
        gVl[c] = gV[0] * Rf[c] + gV[1] * Rf[3 + c] + gV[2] * Rf[6 + c];
    }
}

// ------------------------------------------------------------------------------------------------
// Prior, quaternion block (MarginalizationFactor.cpp:246-252, 276-281): dx = s (q0^-1 (x) q).vec / |q0^-1 (x) q| with s = +-2 by the sign of w;
// returns s, L = Qleft(q0^-1) (its rows 1..3 carry the Jacobian)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fm_prior_quat(const double q0[4], const double q[4], double dx[3], double L[16]) {
    double q0inv[4], dq[4];
    d_qinv(q0, q0inv);
    d_qmul(q0inv, q, dq);
    const double s = dq[0] >= 0 ? 2.0 : -2.0;
    d_qnormalize(dq);
    for (int k = 0; k < 3; ++k) dx[k] = s * dq[1 + k];
    d_qleft(q0inv, L);
    return s;
}

// ------------------------------------------------------------------------------------------------
// SpeedBiasPriorFactorAutoDiff (PriorFactor.h:10-40), entry k of the 9: r = w (x - target) with w = 8 for the two horizontal velocities and 1 for the
// rest, no loss; returns w (the factor's only Jacobian entry in row k).  H_kk += w w, g_k += w r, cost += r r / 2.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double fm_speed_bias_prior(const int k, const double x, const double target, double& r) {
    const double w = k < 2 ? 8.0 : 1.0;
    r = w * (x - target);
    return w;
}

// ------------------------------------------------------------------------------------------------
// The quaternion part shared by delta_q_factor_auto (LidarKeyframeFactor.h:283-303) and LidarPoseFactorBatchRelativeAutoDiff (LidarPoseFactor.h:55-97):
// p = dq^-1 (x) qi^-1 (x) qj with Eigen's inverse() = conjugate / |q|^2, as the reference's Jets differentiate it
// ------------------------------------------------------------------------------------------------
// A = dq^-1, u = qi^-1, Au = A (x) u, p = Au (x) qj
__device__ __forceinline__ void fm_qdiff_products(const double dq[4], const double qi[4], const double qj[4], double A[4], double u[4], double Au[4], double p[4]) {
    d_qinv(dq, A); d_qinv(qi, u);
    d_qmul(A, u, Au); d_qmul(Au, qj, p);
}
// a row G of d r / d u taken through u = qi^-1 = conj(qi) / |qi|^2:  d u_m / d qi_c = ((m == c ? +-1 : 0) - 2 conj(qi)_m qi_c / n2) / n2
__device__ __forceinline__ void fm_qinv_chain(const double G[4], const double qi[4], double Jg[4]) {
    const double n2 = qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3];
    const double Cq[4] = {qi[0], -qi[1], -qi[2], -qi[3]};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) s += G[m] * (((m == c ? (m == 0 ? 1.0 : -1.0) : 0.0) - 2.0 * Cq[m] * qi[c] / n2) / n2);
        Jg[c] = s;
    }
}
// a global 1x4 quaternion Jacobian row through Ceres' QuaternionParameterization at q: Jg d_plus_jac(q)
__device__ __forceinline__ void fm_quat_local(const double Jg[4], const double q[4], double Jl[3]) {
    double P[12];
    d_plus_jac(q, P);
#pragma unroll
    for (int c = 0; c < 3; ++c) Jl[c] = Jg[0] * P[c] + Jg[1] * P[3 + c] + Jg[2] * P[6 + c] + Jg[3] * P[9 + c];
}

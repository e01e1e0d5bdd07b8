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
// The frame the DD rows live in (include/glio_align.h): R_ecef_enu at an anchor, and the DD row with its derivatives wrt the frame
// ------------------------------------------------------------------------------------------------
// the device twin of window_tables.h's ecef2rotation_host (gnss_utility.cpp:347-390, 738-748, closed form): the same expressions in the same order
__device__ __forceinline__ void fm_ecef2rotation(const double xyz[3], double R[9]) {
#pragma clang fp contract(off)
    const double PI = 3.14159265358979323846;
    const double e2 = 6.69437999014e-3, a = 6378137.0, R2D = 180.0 / PI, D2R = PI / 180.0;
    const double a2 = a * a, b2 = a2 * (1 - e2), b = sqrt(b2), ep2 = (a2 - b2) / b2;
    const double p = sqrt(xyz[0] * xyz[0] + xyz[1] * xyz[1]);
    double s1 = xyz[2] * a, s2 = p * b;
    const double h = sqrt(s1 * s1 + s2 * s2);
    const double st = s1 / h, ct = s2 / h;
    s1 = xyz[2] + ep2 * b * pow(st, 3.0);
    s2 = p - a * e2 * pow(ct, 3.0);
    const double lat = (atan(s1 / s2) * R2D) * D2R, lon = (atan2(xyz[1], xyz[0]) * R2D) * D2R;
    const double sl = sin(lat), cl = cos(lat), so = sin(lon), co = cos(lon);
    R[0] = -so; R[1] = -sl * co; R[2] = cl * co;
    R[3] = co;  R[4] = -sl * so; R[5] = cl * so;
    R[6] = 0;   R[7] = cl;       R[8] = sl;
}
// R_ecef_local = R_ecef_enu Rz(yaw), the product as glio_host_ecef_local forms it; c, s = cos, sin of the yaw
__device__ __forceinline__ void fm_ecef_local(const double Ree[9], const double c, const double s, double R[9]) {
#pragma clang fp contract(off)
    const double Rel[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double acc = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc += Ree[i * 3 + k] * Rel[k * 3 + j];
            R[i * 3 + j] = acc;
        }
}
// Row i of factor F against its master at the frame (psi, anc), R = ecef2rotation(anc) Rz(psi), before the whitening: the down-weighted residual and
// its derivatives wrt the step (d_e, d_n, d_u, d_psi) with anc <- anc + ecef2rotation(anc) d_enu, psi <- psi + d_psi.  With g = -wgt (e_i - e_m) -- the
// position Jacobian of fm_dd_row at ratio 1 -- and lp the interpolated local position: d r / d psi = g . (-lp_y, lp_x, 0), d r / d enu = Rz(psi) g.  The
// dependence of ecef2rotation(anc) on anc is left out (|lp| / 6.4e6).  Jb is (d / d psi, 0, 0): the pair (Jenu, Jb) is whitened by fm_dd_whiten like
// (Jri, Jrj).  down = the row was down-weighted.
__device__ __forceinline__ void fm_align_row(const glio_dd_psr& F, const int i, const double threshold, const double Pi[3], const double Pj[3], const double R[9],
                                             const double anc[3], const double c, const double s, double& raw, double Jenu[3], double Jb[3], int& down) {
#pragma clang fp contract(off)
    double Pe[3], lp[3], ru_i, rr_i, obs_i, e_i[3], ru_m, rr_m, obs_m, e_m[3], g[3], z[3], full, gf[3];
    fm_dd_position(F.ratio, Pi, Pj, R, anc, Pe);
#pragma unroll
    for (int k = 0; k < 3; ++k) lp[k] = F.ratio * Pi[k] + (1.0 - F.ratio) * Pj[k];
    fm_dd_satellite(F, i, Pe, R, ru_i, rr_i, obs_i, e_i);
    fm_dd_satellite(F, F.master, Pe, R, ru_m, rr_m, obs_m, e_m);
    fm_dd_row(1.0, threshold, ru_i, rr_i, obs_i, e_i, ru_m, rr_m, obs_m, e_m, raw, g, z);
    fm_dd_row(1.0, INFINITY, ru_i, rr_i, obs_i, e_i, ru_m, rr_m, obs_m, e_m, full, gf, z);     // weight 1: est - obs itself
    down = fabs(full) > threshold ? 1 : 0;
    Jenu[0] = c * g[0] - s * g[1];
    Jenu[1] = s * g[0] + c * g[1];
    Jenu[2] = g[2];
    Jb[0] = g[1] * lp[0] - g[0] * lp[1];
    Jb[1] = 0; Jb[2] = 0;
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

// ------------------------------------------------------------------------------------------------
// Row `row` (0..5) of the relative-pose functor shared by LidarPoseFactorBatchRelativeAutoDiff (LidarPoseFactor.h:55-97, weights 10 and 20) and by
// LidarPoseFactorAutoDiff / LidarPoseLeftFactorAutoDiff / LidarPoseRightFactorAutoDiff (:11-52, :128-221, both weights 0.2):
//   r[0:3] = wq * 2 (dq^-1 q1^-1 q2).vec,  r[3:6] = wp (q1^-1 (p2 - p1) - dp),  Eigen's inverse() = conjugate / |q|^2 and Eigen's q * v on the
//   NON-normalised inverse -- what the reference's Jets differentiate; global Jacobians, then Ceres' QuaternionParameterization.
// cst = dq (w, x, y, z), dp; pa, pb = t, q (w first) of the two poses.  Ja, Jb: this row's six local columns (t, then the rotation) of either pose;
// the left / right factors are this row with Ja / Jb dropped by the caller.  wq * 2 is an exact doubling, so 10 * (2 x) and 20 x give the same bits.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fm_relative_pose_row(const int row, const double wq, const double wp, const double* cst, const double* pa, const double* pb,
                                                     double& r, double* Ja, double* Jb) {
    const double* q1 = pa + 3;
    const double* q2 = pb + 3;
    const double wt = row < 3 ? 2.0 * wq : wp;
    double A[4], u[4], Au[4], p[4], v[3];
    fm_qdiff_products(cst, q1, q2, A, u, Au, p);
    for (int k = 0; k < 3; ++k) v[k] = pb[k] - pa[k];
    const int k = row < 3 ? row : row - 3;
    double Jg1[4], Jg2[4] = {0, 0, 0, 0}, Jp[3] = {0, 0, 0};        // this row's global Jacobians wrt q1, q2 and wrt p2 (= - wrt p1)
    double G[4];                                                       // the row of d r / d u (u = q1^-1), before d u / d q1
    double res;
    if (row < 3) {
        double LA[16], Rv[16], LAu[16];
        d_qleft(A, LA); d_qright(q2, Rv); d_qleft(Au, LAu);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            double sM = 0;
#pragma unroll
            for (int x = 0; x < 4; ++x) sM += (k == 0 ? LA[4 + x] : (k == 1 ? LA[8 + x] : LA[12 + x])) * Rv[x * 4 + m];
            G[m] = sM;
            Jg2[m] = wt * (k == 0 ? LAu[4 + m] : (k == 1 ? LAu[8 + m] : LAu[12 + m]));
        }
        res = wt * (k == 0 ? p[1] : (k == 1 ? p[2] : p[3]));
    } else {
        // M(u) v = v + 2 w (q x v) + 2 q x (q x v);  d/dw = 2 (q x v),  d/dq = -2 w [v]x + 2 ((q.v) I + q v^T - 2 v q^T);  d/dv = M(u)
        const double w = u[0], qx = u[1], qy = u[2], qz = u[3];
        const double cx = qy * v[2] - qz * v[1], cy = qz * v[0] - qx * v[2], cz = qx * v[1] - qy * v[0];          // q x v
        const double ccx = qy * cz - qz * cy, ccy = qz * cx - qx * cz, ccz = qx * cy - qy * cx;                  // q x (q x v)
        const double rv = k == 0 ? v[0] + 2.0 * w * cx + 2.0 * ccx : (k == 1 ? v[1] + 2.0 * w * cy + 2.0 * ccy : v[2] + 2.0 * w * cz + 2.0 * ccz);
        res = wt * (rv - cst[4 + k]);
        const double qv = qx * v[0] + qy * v[1] + qz * v[2];
        const double qk = k == 0 ? qx : (k == 1 ? qy : qz), vk = k == 0 ? v[0] : (k == 1 ? v[1] : v[2]);
        const double qq[3] = {qx, qy, qz};
        // row k of [v]x: (0, -v2, v1), (v2, 0, -v0), (-v1, v0, 0)
        const double sv[3] = {k == 0 ? 0.0 : (k == 1 ? v[2] : -v[1]), k == 0 ? -v[2] : (k == 1 ? 0.0 : v[0]), k == 0 ? v[1] : (k == 1 ? -v[0] : 0.0)};
        // row k of [q]x and of [q]x [q]x = q q^T - (q.q) I
        const double sq[3] = {k == 0 ? 0.0 : (k == 1 ? qz : -qy), k == 0 ? -qz : (k == 1 ? 0.0 : qx), k == 0 ? qy : (k == 1 ? -qx : 0.0)};
        const double q2n = qx * qx + qy * qy + qz * qz;
        G[0] = 2.0 * (k == 0 ? cx : (k == 1 ? cy : cz));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            G[1 + c] = -2.0 * w * sv[c] + 2.0 * ((k == c ? qv : 0.0) + qk * v[c] - 2.0 * vk * qq[c]);
            Jp[c] = wt * ((k == c ? 1.0 : 0.0) + 2.0 * w * sq[c] + 2.0 * (qk * qq[c] - (k == c ? q2n : 0.0)));
        }
    }
    fm_qinv_chain(G, q1, Jg1);
#pragma unroll
    for (int c = 0; c < 4; ++c) Jg1[c] = wt * Jg1[c];
    r = res;
#pragma unroll
    for (int c = 0; c < 3; ++c) { Ja[c] = -Jp[c]; Jb[c] = Jp[c]; }
    fm_quat_local(Jg1, q1, Ja + 3);
    fm_quat_local(Jg2, q2, Jb + 3);
}

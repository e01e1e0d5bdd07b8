// imu_kernels.hip -- IMU pre-integration from raw samples on the device: class Preintegration (GLIO/include/factors/Preintegration.h:29-194)
// restated, one wavefront per edge, and the digest of the finished edge into the form the ImuFactor kernels read (capi.hip: digest_edge).
// The store (glio_imu) is the reference's pre_integrations vector (Estimator.cpp:1582-1600) kept on the device.
//
// How one wavefront integrates one edge.  The sample loop is a sequential recurrence (each push_back multiplies the 15x15 jacobian_ and
// covariance_ from the left by that step's F), so the parallelism is inside a step:
//   * delta_p/q/v and the two rotation matrices are the same for every lane (uniform values in registers; the four divisions of the normalisation
//     are made by four lanes and read back with v_readlane);
//   * the 3x3 blocks of F and V are formed once per step: lane 3 i + j computes element (i, j) of every block (its row of the left factor and its
//     column of the skew matrix picked with selects, rows of an intermediate product fetched from the neighbour lanes) and leaves it in LDS;
//   * F is used block-wise.  Of its 25 blocks only F01 F03 F04 F11 F21 F23 F24 are dense, the rest are 0, I, dt I or -dt I, and rows 9-14 are the
//     identity.  y = F x for one 15-vector x is then a fixed sequence of 3x3 products with every index known at compile time;
//   * jacobian_ = F * jacobian_ acts on the COLUMNS of jacobian_: lane 16 + c keeps column c in registers for the whole edge;
//   * covariance_ = F * covariance_ * F^T + V * noise_ * V^T: lane c takes column c of covariance_ (from LDS) to column c of M = F * covariance_,
//     M goes through LDS, lane c takes ROW c of M to row c of M * F^T (the same y = F x), adds row c of V noise_ V^T and writes the row back.
// The sums run over the same terms in the same order as the dense products of the reference, minus terms that are exactly zero.
// The file is compiled without contraction of products into FMAs, as the other reference-parity files are: the digest below then gives, bit for
// bit, what the host's digest_edge gives for the same covariance.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include <vector>

#include "glio_device.h"

namespace {

#define IMU_CHUNK 64          // samples staged in LDS per pass
#define FB_STRIDE 10          // doubles per 3x3 block in LDS (9 used: keeps every block 16-byte aligned)

struct ImuNoise2 { double an2, gn2, aw2, gw2; };

__device__ __forceinline__ double sel3(double a, double b, double c, int idx) { return idx == 0 ? a : (idx == 1 ? b : c); }
// element (i, j) of (s A) * B from row i of A and column j of B, summed as the dense product sums it
__device__ __forceinline__ double row_col(double s, const double a[3], const double b[3]) { return ((s * a[0]) * b[0] + (s * a[1]) * b[1]) + (s * a[2]) * b[2]; }
// a value of lane `lane` (a compile-time constant) for every lane: two v_readlane, no LDS
__device__ __forceinline__ double from_lane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
// the dense blocks of one step's F (Preintegration.h:132-147)
struct FBlocks { double F01[9], F03[9], F04[9], F11[9], F21[9], F23[9], F24[9], dt; };
// y = F x
__device__ __forceinline__ void apply_F(const FBlocks& f, const double x[15], double y[15]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double s = x[r];
        s = s + f.F01[r * 3 + 0] * x[3]; s = s + f.F01[r * 3 + 1] * x[4]; s = s + f.F01[r * 3 + 2] * x[5];
        s = s + f.dt * x[6 + r];
        s = s + f.F03[r * 3 + 0] * x[9]; s = s + f.F03[r * 3 + 1] * x[10]; s = s + f.F03[r * 3 + 2] * x[11];
        s = s + f.F04[r * 3 + 0] * x[12]; s = s + f.F04[r * 3 + 1] * x[13]; s = s + f.F04[r * 3 + 2] * x[14];
        y[r] = s;
        double u = f.F11[r * 3 + 0] * x[3];
        u = u + f.F11[r * 3 + 1] * x[4]; u = u + f.F11[r * 3 + 2] * x[5];
        u = u + (-f.dt) * x[12 + r];
        y[3 + r] = u;
        double w = f.F21[r * 3 + 0] * x[3];
        w = w + f.F21[r * 3 + 1] * x[4]; w = w + f.F21[r * 3 + 2] * x[5];
        w = w + x[6 + r];
        w = w + f.F23[r * 3 + 0] * x[9]; w = w + f.F23[r * 3 + 1] * x[10]; w = w + f.F23[r * 3 + 2] * x[11];
        w = w + f.F24[r * 3 + 0] * x[12]; w = w + f.F24[r * 3 + 1] * x[13]; w = w + f.F24[r * 3 + 2] * x[14];
        y[6 + r] = w;
    }
#pragma unroll
    for (int r = 9; r < 15; ++r) y[r] = x[r];
}

// One workgroup of one wavefront per edge.  offsets [n_edges + 1] (relative to `samples`), start [n_edges][12], samples [.][7] = dt acc gyr.
__global__ __launch_bounds__(64) void k_imu_integrate(const int* __restrict__ offsets, const double* __restrict__ start, const double* __restrict__ samples,
                                                      int first_edge, int max_samples, ImuNoise2 nz, glio_preint* __restrict__ pre,
                                                      ImuEdgeDev* __restrict__ dig, int* __restrict__ flag) {
    __shared__ double Pm[225];          // covariance_, row-major; later the left half of the Gauss-Jordan tableau
    __shared__ double Mm[225];          // F * covariance_; later the inverse and its Cholesky factor
    __shared__ __align__(16) double Fb[13 * FB_STRIDE];      // this step's 3x3 blocks, element (i, j) of every block made by lane 3 i + j: F01 F03 F04 F11 F21 F23 F24 V00 V01 V02 V20 V21 V22
    __shared__ double smp[IMU_CHUNK * 7];
    __shared__ double fcol[15];
    const int lane = threadIdx.x, e = blockIdx.x, edge = first_edge + e;
    const bool isP = lane < 15, isJ = lane >= 16 && lane < 31;
    const int c = isP ? lane : (isJ ? lane - 16 : 0);
    const int off0 = offsets[e];
    int n = offsets[e + 1] - off0;
    n = n < 0 ? 0 : (n > max_samples ? max_samples : n);          // the host has refused anything else; a bound all the same

    double acc0[3], gyr0[3], ba[3], bg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc0[k] = start[e * 12 + k]; gyr0[k] = start[e * 12 + 3 + k]; ba[k] = start[e * 12 + 6 + k]; bg[k] = start[e * 12 + 9 + k]; }
    double dp[3] = {0, 0, 0}, dq[4] = {1, 0, 0, 0}, dv[3] = {0, 0, 0}, sum_dt = 0.0;
    double jx[15];                      // J lanes: column c of jacobian_ (identity at the start); the other lanes carry zeros
#pragma unroll
    for (int k = 0; k < 15; ++k) jx[k] = (isJ && k == c) ? 1.0 : 0.0;
    for (int i = lane; i < 225; i += 64) Pm[i] = (i / 15 == i % 15) ? 0.001 : 0.0;          // Preintegration.h:56
    __syncthreads();

    for (int base = 0; base < n; base += IMU_CHUNK) {
        const int cnt = n - base < IMU_CHUNK ? n - base : IMU_CHUNK;
        if (lane < cnt) {
            const double* src = samples + (size_t)(off0 + base + lane) * 7;
#pragma unroll
            for (int t = 0; t < 7; ++t) smp[lane * 7 + t] = src[t];
        }
        __syncthreads();
        for (int si = 0; si < cnt; ++si) {
            const double dt = smp[si * 7 + 0];
            const double acc1[3] = {smp[si * 7 + 1], smp[si * 7 + 2], smp[si * 7 + 3]};
            const double gyr1[3] = {smp[si * 7 + 4], smp[si * 7 + 5], smp[si * 7 + 6]};
            // ---- MidPointIntegration (Preintegration.h:106-114)
            double a0[3], a1[3], w[3], un0[3], un1[3], rq[4], rp[3], rv[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a0[k] = acc0[k] - ba[k]; a1[k] = acc1[k] - ba[k]; w[k] = 0.5 * (gyr0[k] + gyr1[k]) - bg[k]; }
            d_qrot_nc(dq, a0, un0);
            {
                const double bx = w[0] * dt / 2, by = w[1] * dt / 2, bz = w[2] * dt / 2;      // Quaterniond(1, ...): not normalised here (:108)
                rq[0] = dq[0] * 1.0 - dq[1] * bx - dq[2] * by - dq[3] * bz;
                rq[1] = dq[0] * bx + dq[1] * 1.0 + dq[2] * bz - dq[3] * by;
                rq[2] = dq[0] * by + dq[2] * 1.0 + dq[3] * bx - dq[1] * bz;
                rq[3] = dq[0] * bz + dq[3] * 1.0 + dq[1] * by - dq[2] * bx;
            }
            d_qrot_nc(rq, a1, un1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double un = 0.5 * (un0[k] + un1[k]);
                rp[k] = dp[k] + dv[k] * dt + 0.5 * un * dt * dt;
                rv[k] = dv[k] + un * dt;
            }
            // ---- F and V (Preintegration.h:117-163): lane 3 i + j forms element (i, j) of every 3x3 block (the lanes above 8 repeat lanes 0-8 and write nothing)
            double Rq[9], Rr[9];
            d_q2R_nc(dq, Rq); d_q2R_nc(rq, Rr);
            const double wd0 = w[0] * dt, wd1 = w[1] * dt, wd2 = w[2] * dt;
            const double hdt = 0.5 * dt;
            {
                const int el = lane % 9, bi = el / 3, bj = el % 3;
                const double rqi[3] = {sel3(Rq[0], Rq[3], Rq[6], bi), sel3(Rq[1], Rq[4], Rq[7], bi), sel3(Rq[2], Rq[5], Rq[8], bi)};          // row i of delta_q's matrix
                const double rri[3] = {sel3(Rr[0], Rr[3], Rr[6], bi), sel3(Rr[1], Rr[4], Rr[7], bi), sel3(Rr[2], Rr[5], Rr[8], bi)};          // ... of result_delta_q's
                const double s0[3] = {sel3(0.0, -a0[2], a0[1], bj), sel3(a0[2], 0.0, -a0[0], bj), sel3(-a0[1], a0[0], 0.0, bj)};              // column j of R_a_0_x
                const double s1[3] = {sel3(0.0, -a1[2], a1[1], bj), sel3(a1[2], 0.0, -a1[0], bj), sel3(-a1[1], a1[0], 0.0, bj)};              // column j of R_a_1_x
                const double im[3] = {sel3(1.0, wd2, -wd1, bj), sel3(-wd2, 1.0, wd0, bj), sel3(wd1, -wd0, 1.0, bj)};                          // column j of I - R_w_x * dt
                const double A25 = row_col(-0.25, rqi, s0), A50 = row_col(-0.5, rqi, s0);          // -0.25 / -0.5 * delta_q.toRotationMatrix() * R_a_0_x
                const double B25 = row_col(0.25, rri, s1), B50 = row_col(0.5, rri, s1);            // +-0.25 / +-0.5 * result_delta_q.toRotationMatrix() * R_a_1_x (the sign is exact)
                const double B16 = row_col(-0.1667, rri, s1);
                // (.. * R_a_1_x) * (I - R_w_x * dt): row i of the left factor sits in lanes 3 i .. 3 i + 2
                const double b25[3] = {-__shfl(B25, 3 * bi + 0), -__shfl(B25, 3 * bi + 1), -__shfl(B25, 3 * bi + 2)};
                const double b50[3] = {-__shfl(B50, 3 * bi + 0), -__shfl(B50, 3 * bi + 1), -__shfl(B50, 3 * bi + 2)};
                const double C25 = (b25[0] * im[0] + b25[1] * im[1]) + b25[2] * im[2];
                const double C50 = (b50[0] * im[0] + b50[1] * im[1]) + b50[2] * im[2];
                const double rq_e = sel3(rqi[0], rqi[1], rqi[2], bj), rr_e = sel3(rri[0], rri[1], rri[2], bj);
                if (lane < 9) {
                    Fb[0 * FB_STRIDE + el] = A25 * dt * dt + C25 * dt * dt;                 // F01
                    Fb[1 * FB_STRIDE + el] = -0.25 * (rq_e + rr_e) * dt * dt;               // F03
                    Fb[2 * FB_STRIDE + el] = B16 * dt * dt * -dt;                           // F04
                    Fb[3 * FB_STRIDE + el] = sel3(im[0], im[1], im[2], bi);                 // F11 = I - R_w_x * dt
                    Fb[4 * FB_STRIDE + el] = A50 * dt + C50 * dt;                           // F21
                    Fb[5 * FB_STRIDE + el] = -0.5 * (rq_e + rr_e) * dt;                     // F23
                    Fb[6 * FB_STRIDE + el] = -B50 * dt * -dt;                               // F24
                    Fb[7 * FB_STRIDE + el] = 0.5 * rq_e * dt * dt;                          // V00
                    Fb[8 * FB_STRIDE + el] = B25 * dt * dt * 0.5 * dt;                      // V01 (= V03)
                    Fb[9 * FB_STRIDE + el] = 0.5 * rr_e * dt * dt;                          // V02
                    Fb[10 * FB_STRIDE + el] = 0.5 * rq_e * dt;                              // V20
                    Fb[11 * FB_STRIDE + el] = -B50 * dt * 0.5 * dt;                         // V21 (= V23)
                    Fb[12 * FB_STRIDE + el] = 0.5 * rr_e * dt;                              // V22
                }
            }
            __syncthreads();
            FBlocks f;
            f.dt = dt;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                f.F01[k] = Fb[0 * FB_STRIDE + k]; f.F03[k] = Fb[1 * FB_STRIDE + k]; f.F04[k] = Fb[2 * FB_STRIDE + k]; f.F11[k] = Fb[3 * FB_STRIDE + k];
                f.F21[k] = Fb[4 * FB_STRIDE + k]; f.F23[k] = Fb[5 * FB_STRIDE + k]; f.F24[k] = Fb[6 * FB_STRIDE + k];
            }
            // ---- jacobian_ = F * jacobian_ (J lanes, registers) and M = F * covariance_ (P lanes, column c)
            double x[15], y[15];
#pragma unroll
            for (int k = 0; k < 15; ++k) x[k] = isP ? Pm[k * 15 + c] : jx[k];
            apply_F(f, x, y);
#pragma unroll
            for (int k = 0; k < 15; ++k) {
                if (isP) Mm[k * 15 + c] = y[k];
                else jx[k] = y[k];
            }
            __syncthreads();
            // ---- covariance_ = M * F^T + V * noise_ * V^T (P lanes, row c)
            if (isP) {
#pragma unroll
                for (int k = 0; k < 15; ++k) x[k] = Mm[c * 15 + k];
                apply_F(f, x, y);
                if (c < 9) {
                    double V00[9], V01[9], V02[9], V20[9], V21[9], V22[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        V00[k] = Fb[7 * FB_STRIDE + k]; V01[k] = Fb[8 * FB_STRIDE + k]; V02[k] = Fb[9 * FB_STRIDE + k];
                        V20[k] = Fb[10 * FB_STRIDE + k]; V21[k] = Fb[11 * FB_STRIDE + k]; V22[k] = Fb[12 * FB_STRIDE + k];
                    }
                    // row c of V (columns 0-11; the rest of rows 0-8 is zero) times noise_: rows 0-2 [V00 V01 V02 V01], rows 3-5 [0 dt/2 I 0 dt/2 I], rows 6-8 [V20 V21 V22 V21]
                    const int rb = c / 3, rr = c % 3;
                    const double* vb = &Fb[(rb == 0 ? 7 : 10) * FB_STRIDE + rr * 3];
                    double vn[12];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double h = rr == k ? hdt : 0.0;
                        vn[k] = (rb == 1 ? 0.0 : vb[k]) * nz.an2;
                        vn[3 + k] = (rb == 1 ? h : vb[FB_STRIDE + k]) * nz.gn2;
                        vn[6 + k] = (rb == 1 ? 0.0 : vb[2 * FB_STRIDE + k]) * nz.an2;
                        vn[9 + k] = vn[3 + k];
                    }
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        double q0 = vn[0] * V00[r * 3 + 0];
                        q0 = q0 + vn[1] * V00[r * 3 + 1]; q0 = q0 + vn[2] * V00[r * 3 + 2];
                        q0 = q0 + vn[3] * V01[r * 3 + 0]; q0 = q0 + vn[4] * V01[r * 3 + 1]; q0 = q0 + vn[5] * V01[r * 3 + 2];
                        q0 = q0 + vn[6] * V02[r * 3 + 0]; q0 = q0 + vn[7] * V02[r * 3 + 1]; q0 = q0 + vn[8] * V02[r * 3 + 2];
                        q0 = q0 + vn[9] * V01[r * 3 + 0]; q0 = q0 + vn[10] * V01[r * 3 + 1]; q0 = q0 + vn[11] * V01[r * 3 + 2];
                        y[r] = y[r] + q0;
                        double q1 = vn[3 + r] * hdt;
                        q1 = q1 + vn[9 + r] * hdt;
                        y[3 + r] = y[3 + r] + q1;
                        double q2 = vn[0] * V20[r * 3 + 0];
                        q2 = q2 + vn[1] * V20[r * 3 + 1]; q2 = q2 + vn[2] * V20[r * 3 + 2];
                        q2 = q2 + vn[3] * V21[r * 3 + 0]; q2 = q2 + vn[4] * V21[r * 3 + 1]; q2 = q2 + vn[5] * V21[r * 3 + 2];
                        q2 = q2 + vn[6] * V22[r * 3 + 0]; q2 = q2 + vn[7] * V22[r * 3 + 1]; q2 = q2 + vn[8] * V22[r * 3 + 2];
                        q2 = q2 + vn[9] * V21[r * 3 + 0]; q2 = q2 + vn[10] * V21[r * 3 + 1]; q2 = q2 + vn[11] * V21[r * 3 + 2];
                        y[6 + r] = y[6 + r] + q2;
                    }
                } else {
                    const double qd = (dt * (c < 12 ? nz.aw2 : nz.gw2)) * dt;          // rows 9-14 of V: dt I against acc_w / gyr_w (:162-163)
#pragma unroll
                    for (int k = 9; k < 15; ++k) y[k] = y[k] + (k == c ? qd : 0.0);
                }
#pragma unroll
                for (int k = 0; k < 15; ++k) Pm[c * 15 + k] = y[k];
            }
            // ---- Propagate (Preintegration.h:185-193)
            {
                const double nrm = sqrt(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
                const double part = ((lane & 3) == 0 ? rq[0] : sel3(rq[1], rq[2], rq[3], (lane & 3) - 1)) / nrm;          // lanes 0-3 divide one coefficient each
#pragma unroll
                for (int k = 0; k < 4; ++k) dq[k] = from_lane(part, k);
#pragma unroll
                for (int k = 0; k < 3; ++k) { dp[k] = rp[k]; dv[k] = rv[k]; acc0[k] = acc1[k]; gyr0[k] = gyr1[k]; }
                sum_dt += dt;
            }
            __syncthreads();
        }
    }

    // ---- the host view (glio_preint) and the non-finite flag
    bool ok = isfinite(sum_dt);
#pragma unroll
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(dp[k]) && isfinite(dv[k]) && isfinite(ba[k]) && isfinite(bg[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) ok = ok && isfinite(dq[k]);
#pragma unroll
    for (int k = 0; k < 15; ++k) ok = ok && isfinite(jx[k]);
    glio_preint* po = pre + edge;
    ImuEdgeDev* eo = dig + edge;
    for (int i = lane; i < 225; i += 64) { const double v = Pm[i]; po->covariance[i] = v; ok = ok && isfinite(v); }
    if (isJ) {
#pragma unroll
        for (int k = 0; k < 15; ++k) po->jacobian[k * 15 + c] = jx[k];
        // the five bias-Jacobian blocks of ImuEdgeDev (capi.hip: digest_edge)
        if (c >= 9 && c < 12) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { eo->dp_dba[r * 3 + c - 9] = jx[r]; eo->dv_dba[r * 3 + c - 9] = jx[6 + r]; }
        } else if (c >= 12) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { eo->dp_dbg[r * 3 + c - 12] = jx[r]; eo->dq_dbg[r * 3 + c - 12] = jx[3 + r]; eo->dv_dbg[r * 3 + c - 12] = jx[6 + r]; }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            po->delta_p[k] = dp[k]; po->delta_v[k] = dv[k]; po->linearized_ba[k] = ba[k]; po->linearized_bg[k] = bg[k];
            eo->delta_p[k] = dp[k]; eo->delta_v[k] = dv[k]; eo->lin_ba[k] = ba[k]; eo->lin_bg[k] = bg[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { po->delta_q[k] = dq[k]; eo->delta_q[k] = dq[k]; }
        po->sum_dt = sum_dt; eo->sum_dt = sum_dt; eo->slot_i = 0; eo->pad_ = 0;
    }
    int fail = __any(!ok) ? GLIO_IMU_FLAG_NONFINITE : 0;

    // ---- digest: sqrt_info = LLT(covariance^-1).L^T (ImuFactor.h:44-45), capi.hip's inv15 + Cholesky with lane j owning column j of [A | A^-1]
    for (int i = lane; i < 225; i += 64) Mm[i] = (i / 15 == i % 15) ? 1.0 : 0.0;
    __syncthreads();
    double* col = lane < 15 ? &Pm[lane] : &Mm[lane < 30 ? lane - 15 : 0];
    for (int cc = 0; cc < 15 && !fail; ++cc) {
        int piv = cc;
        double best = fabs(Pm[cc * 15 + cc]);
        for (int r = cc + 1; r < 15; ++r) { const double v = fabs(Pm[r * 15 + cc]); if (v > best) { best = v; piv = r; } }
        if (best == 0.0) { fail = GLIO_IMU_FLAG_SINGULAR; break; }
        __syncthreads();
        if (lane < 30 && piv != cc) { const double t = col[cc * 15]; col[cc * 15] = col[piv * 15]; col[piv * 15] = t; }
        __syncthreads();
        if (lane < 15) fcol[lane] = Pm[lane * 15 + cc];
        __syncthreads();
        if (lane < 30) {
            const double vc = col[cc * 15] / fcol[cc];
            col[cc * 15] = vc;
            for (int r = 0; r < 15; ++r) {
                if (r == cc) continue;
                const double fr = fcol[r];
                if (fr == 0.0) continue;
                col[r * 15] = col[r * 15] - fr * vc;
            }
        }
        __syncthreads();
    }
    for (int j = 0; j < 15 && !fail; ++j) {          // lower Cholesky of the (lower triangle of the) inverse, lane i owning row i
        double d = Mm[j * 15 + j];
        for (int k = 0; k < j; ++k) d = d - Mm[j * 15 + k] * Mm[j * 15 + k];
        if (!(d > 0.0)) { fail = GLIO_IMU_FLAG_SINGULAR; break; }
        d = sqrt(d);
        __syncthreads();
        if (lane == j) Mm[j * 15 + j] = d;
        if (lane > j && lane < 15) {
            double s = Mm[lane * 15 + j];
            for (int k = 0; k < j; ++k) s = s - Mm[lane * 15 + k] * Mm[j * 15 + k];
            Mm[lane * 15 + j] = s / d;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = lane; i < 225; i += 64) {
        const int r = i / 15, cj = i % 15;
        eo->sqrt_info[i] = (!fail && cj >= r) ? Mm[cj * 15 + r] : 0.0;
    }
    if (lane == 0) flag[edge] = fail;
}

struct GatherList { int edge[GLIO_MAX_WINDOW]; int slot[GLIO_MAX_WINDOW]; };
__device__ __forceinline__ void copy_edge(const ImuEdgeDev* __restrict__ src, ImuEdgeDev* __restrict__ dst, int slot) {
    static_assert(sizeof(ImuEdgeDev) % 8 == 0, "ImuEdgeDev is copied by 8-byte words");
    const unsigned long long* s = reinterpret_cast<const unsigned long long*>(src);
    unsigned long long* d = reinterpret_cast<unsigned long long*>(dst);
    const int words = (int)(sizeof(ImuEdgeDev) / 8);
    for (int i = threadIdx.x; i < words; i += blockDim.x) d[i] = s[i];
    __syncthreads();
    if (threadIdx.x == 0) { dst->slot_i = slot; dst->pad_ = 0; }
}
__global__ __launch_bounds__(64) void k_imu_gather_list(const ImuEdgeDev* __restrict__ src, ImuEdgeDev* __restrict__ dst, GatherList g) {
    copy_edge(src + g.edge[blockIdx.x], dst + blockIdx.x, g.slot[blockIdx.x]);
}
__global__ __launch_bounds__(64) void k_imu_gather_range(const ImuEdgeDev* __restrict__ src, ImuEdgeDev* __restrict__ dst, int first) {
    copy_edge(src + first + blockIdx.x, dst + blockIdx.x, (int)blockIdx.x);
}

size_t round64(size_t v) { return (v + 63) & ~(size_t)63; }

}  // namespace

void glio_imu_launch_gather_list(hipStream_t stream, const glio_imu* s, int n, const int32_t* edge, const int32_t* slot, ImuEdgeDev* dst) {
    if (n <= 0) return;
    GatherList g;
    memset(&g, 0, sizeof g);
    for (int k = 0; k < n && k < GLIO_MAX_WINDOW; ++k) { g.edge[k] = edge[k]; g.slot[k] = slot[k]; }
    hipLaunchKernelGGL(k_imu_gather_list, dim3(n), dim3(64), 0, stream, s->d_dig, dst, g);
}
void glio_imu_launch_gather_range(hipStream_t stream, const glio_imu* s, int first, int n, ImuEdgeDev* dst) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_imu_gather_range, dim3(n), dim3(64), 0, stream, s->d_dig, dst, first);
}
int glio_imu_known_flag(const glio_imu* s, int first, int n, const int32_t* list) {
    for (int k = 0; k < n; ++k) {
        const int e = list ? list[k] : first + k;
        if (e >= 0 && e < s->max_edges && s->h_flag[e]) return e;
    }
    return -1;
}

extern "C" {

void glio_imu_noise_default(glio_imu_noise* n) {          // config_urban_hk.yaml:7-10
    n->acc_n = 3.9939570888238808e-03; n->gyr_n = 1.5636343949698187e-03; n->acc_w = 6.4356659353532566e-05; n->gyr_w = 3.5640318696367613e-05;
}
int glio_imu_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_imu_noise), (int32_t)sizeof(glio_imu_sample)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

static int imu_create_body(glio_imu* s) {
    GLIO_HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipEventCreate(&s->ev_t0));
    GLIO_HIP_CHECK(hipEventCreate(&s->ev_t1));
    GLIO_HIP_CHECK(hipMalloc((void**)&s->d_pre, (size_t)s->max_edges * sizeof(glio_preint)));
    GLIO_HIP_CHECK(hipMalloc((void**)&s->d_dig, (size_t)s->max_edges * sizeof(ImuEdgeDev)));
    GLIO_HIP_CHECK(hipMalloc((void**)&s->d_flag, (size_t)s->max_edges * sizeof(int)));
    GLIO_HIP_CHECK(hipMemset(s->d_pre, 0, (size_t)s->max_edges * sizeof(glio_preint)));
    GLIO_HIP_CHECK(hipMemset(s->d_dig, 0, (size_t)s->max_edges * sizeof(ImuEdgeDev)));
    GLIO_HIP_CHECK(hipMemset(s->d_flag, 0, (size_t)s->max_edges * sizeof(int)));
    GLIO_HIP_CHECK(hipHostMalloc((void**)&s->h_flag, (size_t)s->max_edges * sizeof(int)));
    memset(s->h_flag, 0, (size_t)s->max_edges * sizeof(int));
    return GLIO_OK;
}
int glio_imu_create(int device, int max_edges, int max_samples_per_edge, const glio_imu_noise* noise, glio_imu** out) {
    if (!out || !noise || max_edges < 1 || max_samples_per_edge < 0 || max_edges > (1 << 24) || max_samples_per_edge > (1 << 24)) {
        glio_set_error("glio_imu_create: bad argument"); return GLIO_E_ARG;
    }
    if (!(std::isfinite(noise->acc_n) && std::isfinite(noise->gyr_n) && std::isfinite(noise->acc_w) && std::isfinite(noise->gyr_w))) {
        glio_set_error("glio_imu_create: non-finite noise density"); return GLIO_E_ARG;
    }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { glio_set_error("no HIP device visible: the IMU store has no CPU fallback"); return GLIO_E_HIP; }
    if (device < 0 || device >= nd) { glio_set_error("glio_imu_create: device %d of %d", device, nd); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(device));
    glio_imu* s = new glio_imu();
    memset(s, 0, sizeof *s);
    s->device = device; s->max_edges = max_edges; s->max_samples = max_samples_per_edge; s->noise = *noise;
    const int rc = imu_create_body(s);
    if (rc != GLIO_OK) { glio_imu_destroy(s); return rc; }
    *out = s;
    return GLIO_OK;
}
void glio_imu_destroy(glio_imu* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();          // a consumer's stream may still be reading the digested edges
    if (s->d_pre) (void)hipFree(s->d_pre);
    if (s->d_dig) (void)hipFree(s->d_dig);
    if (s->d_flag) (void)hipFree(s->d_flag);
    if (s->d_up) (void)hipFree(s->d_up);
    if (s->h_up) (void)hipHostFree(s->h_up);
    if (s->h_flag) (void)hipHostFree(s->h_flag);
    if (s->ev_done) (void)hipEventDestroy(s->ev_done);
    if (s->ev_copied) (void)hipEventDestroy(s->ev_copied);
    if (s->ev_t0) (void)hipEventDestroy(s->ev_t0);
    if (s->ev_t1) (void)hipEventDestroy(s->ev_t1);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int glio_imu_integrate(glio_imu* s, int first_edge, int n_edges, const int32_t* sample_offset, const glio_imu_sample* samples, const double* start) {
    static_assert(sizeof(glio_imu_sample) == 56, "a sample is 7 doubles");
    if (!s || n_edges < 0 || first_edge < 0) { glio_set_error("glio_imu_integrate: negative count"); return GLIO_E_ARG; }
    if ((long long)first_edge + n_edges > s->max_edges) { glio_set_error("glio_imu_integrate: edges %d .. %d of a store of %d", first_edge, first_edge + n_edges - 1, s->max_edges); return GLIO_E_ARG; }
    if (n_edges == 0) return GLIO_OK;
    if (!sample_offset || !start) { glio_set_error("glio_imu_integrate: null argument"); return GLIO_E_ARG; }
    if (sample_offset[0] < 0) { glio_set_error("glio_imu_integrate: negative sample offset"); return GLIO_E_ARG; }
    for (int e = 0; e < n_edges; ++e) {
        const long long len = (long long)sample_offset[e + 1] - sample_offset[e];
        if (len < 0) { glio_set_error("glio_imu_integrate: sample offsets decrease at edge %d", first_edge + e); return GLIO_E_ARG; }
        if (len > s->max_samples) { glio_set_error("glio_imu_integrate: edge %d has %lld samples, the store takes %d per edge", first_edge + e, len, s->max_samples); return GLIO_E_ARG; }
    }
    const int s0 = sample_offset[0];
    const size_t total = (size_t)(sample_offset[n_edges] - s0);
    if (total > 0 && !samples) { glio_set_error("glio_imu_integrate: null samples"); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(s->device));
    const size_t off_b = round64((size_t)(n_edges + 1) * 4), start_b = round64((size_t)n_edges * 12 * 8), smp_b = round64(total * sizeof(glio_imu_sample) + 8);
    const size_t need = off_b + start_b + smp_b;
    if (s->copying) { GLIO_HIP_CHECK(hipEventSynchronize(s->ev_copied)); s->copying = false; }
    if (need > s->up_cap) {
        GLIO_HIP_CHECK(hipStreamSynchronize(s->stream));
        if (s->h_up) (void)hipHostFree(s->h_up);
        if (s->d_up) (void)hipFree(s->d_up);
        s->h_up = nullptr; s->d_up = nullptr; s->up_cap = 0;
        const size_t cap = need + need / 2 + 4096;
        GLIO_HIP_CHECK(hipHostMalloc((void**)&s->h_up, cap));
        GLIO_HIP_CHECK(hipMalloc((void**)&s->d_up, cap));
        s->up_cap = cap;
    }
    int32_t* ho = reinterpret_cast<int32_t*>(s->h_up);
    for (int e = 0; e <= n_edges; ++e) ho[e] = sample_offset[e] - s0;
    memcpy(s->h_up + off_b, start, (size_t)n_edges * 12 * 8);
    if (total) memcpy(s->h_up + off_b + start_b, samples + s0, total * sizeof(glio_imu_sample));
    // the kernel that reads the mirror is ordered behind the copy on the same stream; the previous kernel that read it is ahead of the copy
    GLIO_HIP_CHECK(hipMemcpyAsync(s->d_up, s->h_up, need, hipMemcpyHostToDevice, s->stream));
    GLIO_HIP_CHECK(hipEventRecord(s->ev_copied, s->stream));
    s->copying = true;
    ImuNoise2 nz;
    nz.an2 = s->noise.acc_n * s->noise.acc_n; nz.gn2 = s->noise.gyr_n * s->noise.gyr_n;
    nz.aw2 = s->noise.acc_w * s->noise.acc_w; nz.gw2 = s->noise.gyr_w * s->noise.gyr_w;
    GLIO_HIP_CHECK(hipEventRecord(s->ev_t0, s->stream));
    hipLaunchKernelGGL(k_imu_integrate, dim3(n_edges), dim3(64), 0, s->stream, reinterpret_cast<const int*>(s->d_up),
                       reinterpret_cast<const double*>(s->d_up + off_b), reinterpret_cast<const double*>(s->d_up + off_b + start_b), first_edge, s->max_samples, nz,
                       s->d_pre, s->d_dig, s->d_flag);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(s->ev_t1, s->stream));
    GLIO_HIP_CHECK(hipEventRecord(s->ev_done, s->stream));
    s->timed = 1;
    return GLIO_OK;
}

int glio_imu_read(glio_imu* s, int first_edge, int n_edges, glio_preint* out) {
    if (!s || n_edges < 0 || first_edge < 0 || (long long)first_edge + n_edges > s->max_edges || (n_edges > 0 && !out)) {
        glio_set_error("glio_imu_read: bad edge range"); return GLIO_E_ARG;
    }
    GLIO_HIP_CHECK(hipSetDevice(s->device));
    GLIO_HIP_CHECK(hipMemcpyAsync(s->h_flag, s->d_flag, (size_t)s->max_edges * sizeof(int), hipMemcpyDeviceToHost, s->stream));
    if (n_edges) GLIO_HIP_CHECK(hipMemcpyAsync(out, s->d_pre + first_edge, (size_t)n_edges * sizeof(glio_preint), hipMemcpyDeviceToHost, s->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(s->stream));
    const int bad = glio_imu_known_flag(s, first_edge, n_edges, nullptr);
    if (bad >= 0) {
        glio_set_error("IMU edge %d: %s", bad, s->h_flag[bad] == GLIO_IMU_FLAG_NONFINITE ? "non-finite sample or start value" : "covariance not invertible / not SPD");
        return GLIO_E_NUMERIC;
    }
    return GLIO_OK;
}

int glio_imu_last_device_ms(glio_imu* s, float* ms) {
    if (!s || !ms) return GLIO_E_ARG;
    if (!s->timed) { glio_set_error("glio_imu_integrate first"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(s->device));
    GLIO_HIP_CHECK(hipEventSynchronize(s->ev_t1));
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, s->ev_t0, s->ev_t1));
    return GLIO_OK;
}

}  // extern "C"

// trajectory_kernels.hip -- the every-frame trajectory (include/glio_traj.h): the IMU fill-in between two keyframes, the relative measurements and
// optimizeLocalGraph (GLIO/src/Estimator.cpp:4273-4557, :3452-3527) in ONE launch, one wavefront per gap.
//
// How one wavefront works one gap.
//   * Dead reckoning and measurements are a serial recurrence over ~40 sample rows: every lane carries the same P, V, R in registers (the loads are
//     uniform), lane 0 writes the rows out.  Nothing here is worth spreading over lanes; what the device buys is the stream of its own and the batch form.
//   * The local graph's normal equations are block tridiagonal in 6 x 6 blocks: Hd[k] (diagonal) and Ho[k] = H(k, k + 1) live in LDS, twice (the iterate's
//     and the candidate's).  A pass evaluates ten factors, lane 6 f + r taking row r of factor f through fm_relative_pose_row (factor_math.h, the definition
//     the batch stage's k_small_eval uses with weights 10 / 20), and then forms the blocks of nine poses, one lane per entry, each entry one sum over the
//     rows of factor k then of factor k + 1 -- a fixed order, no atomics, no "+=" into shared entries.
//   * The Gauss-Newton step factorises Hs + mu D^2 as a band matrix of half-width 11 -- the block-tridiagonal fill, column j holding rows j .. j + 11 --
//     in the LDS of the candidate's blocks, which are free between a rejected or accepted candidate and the next evaluation.  Column by column: lanes
//     0-11 scale the column, then the 66 (column, row) pairs of the trailing 11 x 11 corner are updated, one lane each in two sweeps.  The two triangular solves walk
//     the same band.
//   * The trust-region loop (tests/np_ceres.py::minimize with Options(max_iterations=15, strategy="dogleg", dogleg="traditional", nonmonotonic=False)) runs
//     in uniform scalars; every dot product is lane-strided partial sums joined by the fixed butterfly of wave_sum.  Monotonic steps only lower the cost,
//     so the minimum-cost iterate Ceres returns is always the current one: no third copy of the poses.
#pragma clang fp contract(off)
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/glio_traj.h"
#include "factor_math.h"
#include "glio_device.h"
#include "tr_math.h"
#include "tr_math_device.h"

namespace {
static_assert(GLIO_TRAJ_NO_CONVERGENCE == TR_NO_CONVERGENCE && GLIO_TRAJ_FUNCTION_TOLERANCE == TR_FUNCTION_TOL && GLIO_TRAJ_PARAMETER_TOLERANCE == TR_PARAMETER_TOL &&
              GLIO_TRAJ_GRADIENT_TOLERANCE == TR_GRADIENT_TOL && GLIO_TRAJ_MIN_RADIUS == TR_MIN_RADIUS_REACHED && GLIO_TRAJ_FAILURE == TR_FAILURE, "GLIO_TRAJ_* = GLIO_TERM_* on 0 .. 5");

#define TJ_F GLIO_TRAJ_MAX_FRAMES
#define TJ_N (6 * TJ_F)            // unknowns at most
#define TJ_BW 12                   // band: rows j .. j + 11 of column j
#define TJ_ROW 13                  // r, Ja[6], Jb[6] of one factor row
#define TJ_HDR 39                  // P V R g prev_row anchor_left anchor_right

struct TrajStore {
    double* dr;                    // [max_gaps][F + 1][7]
    double* meas;                  // [max_gaps][F + 1][7]
    double* sol;                   // [max_gaps][F][7]
    glio_traj_summary* sum;        // [max_gaps]
    int max_frames, max_iterations;
};

// Eigen 3.3 quaternionbase_assign_impl<Matrix3d> (Quaterniond(Matrix3d)): the trace branch and the three diagonal branches, not normalised
__device__ __forceinline__ void quat_from_matrix(const double m[9], double q[4]) {
    double t = m[0] + m[4] + m[8], w, x, y, z;          // scalars, stored once at the end: stores sunk into a phi of pointers would put q into scratch
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        w = 0.5 * t;
        t = 0.5 / t;
        x = (m[7] - m[5]) * t; y = (m[2] - m[6]) * t; z = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
        if (i == 0) {                       // j = 1, k = 2
            t = sqrt(m[0] - m[4] - m[8] + 1.0);
            x = 0.5 * t; t = 0.5 / t;
            w = (m[7] - m[5]) * t; y = (m[3] + m[1]) * t; z = (m[6] + m[2]) * t;
        } else if (i == 1) {                // j = 2, k = 0
            t = sqrt(m[4] - m[8] - m[0] + 1.0);
            y = 0.5 * t; t = 0.5 / t;
            w = (m[2] - m[6]) * t; z = (m[7] + m[5]) * t; x = (m[1] + m[3]) * t;
        } else {                            // j = 0, k = 1
            t = sqrt(m[8] - m[0] - m[4] + 1.0);
            z = 0.5 * t; t = 0.5 / t;
            w = (m[3] - m[1]) * t; x = (m[2] + m[6]) * t; y = (m[5] + m[7]) * t;
        }
    }
    q[0] = w; q[1] = x; q[2] = y; q[3] = z;
}
// measurement row (dq, dp) from pose row a to pose row b (:4500-4527)
__device__ __forceinline__ void measure(const double ta[3], const double qa[4], const double tb[3], const double qb[4], double m[7]) {
    double qi[4], d[3], o[3], dq[4];
    d_qinv(qa, qi);
    for (int k = 0; k < 3; ++k) d[k] = tb[k] - ta[k];
    d_qrot_nc(qi, d, o);
    d_qmul(qi, qb, dq);
    for (int k = 0; k < 4; ++k) m[k] = dq[k];
    for (int k = 0; k < 3; ++k) m[4 + k] = o[k];
}
// pose row b = pose row a (+) measurement m
__device__ __forceinline__ void compose(const double a[7], const double m[7], double b[7]) {
    double o[3];
    d_qrot_nc(a + 3, m + 4, o);
    for (int k = 0; k < 3; ++k) b[k] = a[k] + o[k];
    d_qmul(a + 3, m, b + 3);
}
__device__ __forceinline__ double vdot(const double* a, const double* b, int n, int lane) {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += a[i] * b[i];
    return wave_sum(s);
}
// entry (i, j), i >= j, of the block-tridiagonal matrix
__device__ __forceinline__ double h_entry(const double* Hd, const double* Ho, int i, int j) {
    const int bi = i / 6, bj = j / 6;
    if (bi == bj) return Hd[bi * 36 + (i % 6) * 6 + j % 6];
    if (bi == bj + 1) return Ho[bj * 36 + (j % 6) * 6 + i % 6];
    return 0.0;
}
// out = S H S v (S = diag(scale)); out != v
__device__ __forceinline__ void hs_mul(const double* Hd, const double* Ho, const double* scale, const double* v, double* out, int N, int lane) {
    for (int i = lane; i < 6 * N; i += 64) {
        const int b = i / 6, r = i % 6;
        double s = 0.0;
        if (b > 0) for (int c = 0; c < 6; ++c) s += (scale[i] * Ho[(b - 1) * 36 + c * 6 + r] * scale[(b - 1) * 6 + c]) * v[(b - 1) * 6 + c];
        for (int c = 0; c < 6; ++c) s += (scale[i] * Hd[b * 36 + r * 6 + c] * scale[b * 6 + c]) * v[b * 6 + c];
        if (b + 1 < N) for (int c = 0; c < 6; ++c) s += (scale[i] * Ho[b * 36 + r * 6 + c] * scale[(b + 1) * 6 + c]) * v[(b + 1) * 6 + c];
        out[i] = s;
    }
    GLIO_WAVE_LDS_SYNC();
}

// cost, blocks and gradient of the chain x [N][7] between the anchors: LidarPoseLeftFactor (measurement 0), LidarPoseFactor i -> i + 1 (measurement i, as
// written at :3490), LidarPoseRightFactor (measurement N)
__device__ __forceinline__ double evaluate(const double* x, const double* anc, const double* meas, double* Jr, double* Hd, double* Ho, double* g, int N, int lane) {
    double c2 = 0.0;
    for (int k0 = 0; k0 < N; k0 += 9) {
        const int fl = lane / 6, row = lane % 6, f = k0 + fl;
        if (lane < 60 && f <= N) {
            const double* pa = f == 0 ? anc : x + 7 * (f - 1);
            const double* pb = f == N ? anc + 7 : x + 7 * f;
            const double* cst = meas + 7 * (f == 0 ? 0 : (f == N ? N : f - 1));
            double r;
            fm_relative_pose_row(row, 0.2, 0.2, cst, pa, pb, r, Jr + lane * TJ_ROW + 1, Jr + lane * TJ_ROW + 7);
            Jr[lane * TJ_ROW] = r;
            if (fl < 9 || f == N) c2 += r * r;          // factor k0 + 9 comes again as the next pass's first
        }
        GLIO_WAVE_LDS_SYNC();
        const int np = N - k0 < 9 ? N - k0 : 9;          // poses k0 .. k0 + np - 1: factor k (its Jb) and factor k + 1 (its Ja)
        for (int e = lane; e < np * 78; e += 64) {
            const int kl = e / 78, w = e % 78, k = k0 + kl;
            const double* Fb = Jr + (kl * 6) * TJ_ROW;           // rows of factor k
            const double* Fa = Jr + ((kl + 1) * 6) * TJ_ROW;     // rows of factor k + 1
            double s = 0.0;
            if (w < 36) {
                const int u = w / 6, v = w % 6;
                for (int q = 0; q < 6; ++q) s += Fb[q * TJ_ROW + 7 + u] * Fb[q * TJ_ROW + 7 + v];
                for (int q = 0; q < 6; ++q) s += Fa[q * TJ_ROW + 1 + u] * Fa[q * TJ_ROW + 1 + v];
                Hd[k * 36 + w] = s;
            } else if (w < 72) {
                const int u = (w - 36) / 6, v = (w - 36) % 6;
                if (k + 1 < N) {
                    for (int q = 0; q < 6; ++q) s += Fa[q * TJ_ROW + 1 + u] * Fa[q * TJ_ROW + 7 + v];
                    Ho[k * 36 + (w - 36)] = s;
                }
            } else {
                const int u = w - 72;
                for (int q = 0; q < 6; ++q) s += Fb[q * TJ_ROW + 7 + u] * Fb[q * TJ_ROW];
                for (int q = 0; q < 6; ++q) s += Fa[q * TJ_ROW + 1 + u] * Fa[q * TJ_ROW];
                g[k * 6 + u] = s;
            }
        }
        GLIO_WAVE_LDS_SYNC();
    }
    return 0.5 * wave_sum(c2);
}
// max |x - Plus(x, -g)| over all coordinates: Ceres' gradient max norm through the parameterisation
__device__ __forceinline__ double gradient_max(const double* x, const double* g, int N, int lane) {
    double m = 0.0;
    for (int k = lane; k < N; k += 64) {
        for (int c = 0; c < 3; ++c) m = fmax(m, fabs(x[7 * k + c] - (x[7 * k + c] + -g[6 * k + c])));
        const double d[3] = {-g[6 * k + 3], -g[6 * k + 4], -g[6 * k + 5]};          // (tr_grad_max_rot, written out: through the helper this kernel's schedule moved)
        double o[4];
        d_quat_plus(x + 7 * k + 3, d, o);
        for (int c = 0; c < 4; ++c) m = fmax(m, fabs(x[7 * k + 3 + c] - o[c]));
    }
    return wave_max(m);
}

// mode 0: push (hdr, offs, samples; grid 1, gap = first_gap).  mode 1: resolve (kf [grid + 1][7]; gap = first_gap + block).
__global__ __launch_bounds__(64) void k_traj_gap(const int mode, const int first_gap, const int n_push, const double* __restrict__ hdr, const int* __restrict__ offs,
                                                 const double* __restrict__ samples, const double* __restrict__ kf, const TrajStore st) {
    __shared__ double Hbuf[2][2 * TJ_F * 36];          // [which][Hd | Ho]; the other one doubles as the band of the factorisation (TJ_N * TJ_BW = the same size)
    __shared__ double gbuf[2][TJ_N];
    __shared__ double scale[TJ_N], Dd[TJ_N], grad[TJ_N], gn[TJ_N], step[TJ_N], tmp[TJ_N];
    __shared__ double xbuf[2][TJ_F * 7];
    __shared__ double meas[(TJ_F + 1) * 7];
    __shared__ double Jr[60 * TJ_ROW];
    __shared__ double anc[14];
    static_assert(TJ_N * TJ_BW == 2 * TJ_F * 36, "the band fits the blocks' buffer");
    const int lane = threadIdx.x, gap = first_gap + blockIdx.x;
    const int F1 = st.max_frames + 1;
    double* g_dr = st.dr + (size_t)gap * F1 * 7;
    double* g_meas = st.meas + (size_t)gap * F1 * 7;
    double* g_sol = st.sol + (size_t)gap * st.max_frames * 7;
    glio_traj_summary* g_sum = st.sum + gap;
    int N;
    bool finite = true;

    if (mode == 0) {
        N = n_push;
        N = N < 0 ? 0 : (N > st.max_frames ? st.max_frames : N);          // the host has refused anything else; a bound all the same
        double P[3], V[3], R[9], gv[3], pt[3], pq[4];
        for (int k = 0; k < 3; ++k) { P[k] = hdr[k]; V[k] = hdr[3 + k]; gv[k] = hdr[15 + k]; }
        for (int k = 0; k < 9; ++k) R[k] = hdr[6 + k];
        for (int k = 0; k < 3; ++k) pt[k] = hdr[18 + k];
        for (int k = 0; k < 4; ++k) pq[k] = hdr[21 + k];
        if (lane < 14) anc[lane] = hdr[25 + lane];
        for (int seg = 0; seg <= N; ++seg) {
            const int s0 = offs[seg], s1 = offs[seg + 1];
            double a0[3] = {0, 0, 0}, w0[3] = {0, 0, 0};
            for (int si = s0; si < s1; ++si) {
                const double* sp = samples + (size_t)si * 7;
                const double dt = sp[0];
                const double a1[3] = {sp[1], sp[2], sp[3]}, w1[3] = {sp[4], sp[5], sp[6]};
                if (si > s0) {
                    // :4330-4336
                    double un0[3], un1[3], Dm[9], Rn[9];
                    for (int i = 0; i < 3; ++i) un0[i] = R[3 * i] * a0[0] + R[3 * i + 1] * a0[1] + R[3 * i + 2] * a0[2] - gv[i];
                    const double ug[3] = {0.5 * (w0[0] + w1[0]), 0.5 * (w0[1] + w1[1]), 0.5 * (w0[2] + w1[2])};
                    const double dq[4] = {1.0, ug[0] * dt / 2.0, ug[1] * dt / 2.0, ug[2] * dt / 2.0};
                    d_q2R_nc(dq, Dm);
                    for (int i = 0; i < 3; ++i)
                        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = R[3 * i] * Dm[j] + R[3 * i + 1] * Dm[3 + j] + R[3 * i + 2] * Dm[6 + j];
                    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
                    for (int i = 0; i < 3; ++i) un1[i] = R[3 * i] * a1[0] + R[3 * i + 1] * a1[1] + R[3 * i + 2] * a1[2] - gv[i];
                    for (int k = 0; k < 3; ++k) {
                        const double un = 0.5 * (un0[k] + un1[k]);
                        P[k] = P[k] + (dt * V[k] + 0.5 * dt * dt * un);
                        V[k] = V[k] + dt * un;
                    }
                }
                for (int k = 0; k < 3; ++k) { a0[k] = a1[k]; w0[k] = w1[k]; }
            }
            double q[4], m[7];
            quat_from_matrix(R, q);
            measure(pt, pq, P, q, m);
            for (int k = 0; k < 3; ++k) { finite = finite && isfinite(P[k]); pt[k] = P[k]; }
            for (int k = 0; k < 4; ++k) { finite = finite && isfinite(q[k]); pq[k] = q[k]; }
            for (int k = 0; k < 7; ++k) finite = finite && isfinite(m[k]);
            if (lane < 7) {
                const double rv = lane == 0 ? P[0] : lane == 1 ? P[1] : lane == 2 ? P[2] : lane == 3 ? q[0] : lane == 4 ? q[1] : lane == 5 ? q[2] : q[3];
                const double mv = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : lane == 3 ? m[3] : lane == 4 ? m[4] : lane == 5 ? m[5] : m[6];
                g_dr[seg * 7 + lane] = rv;
                g_meas[seg * 7 + lane] = mv;
                meas[seg * 7 + lane] = mv;
                if (seg < N) xbuf[0][seg * 7 + lane] = rv;
            }
        }
        GLIO_WAVE_LDS_SYNC();
    } else {
        N = g_sum->n_frames;
        N = N < 0 ? 0 : (N > st.max_frames ? st.max_frames : N);
        if (lane < 14) anc[lane] = kf[(size_t)blockIdx.x * 7 + lane];
        for (int i = lane; i < (N + 1) * 7; i += 64) { const double v = g_meas[i]; meas[i] = v; finite = finite && isfinite(v); }
        GLIO_WAVE_LDS_SYNC();
        // the chain composed from the left anchor with the measurements the left and between factors use (uniform; lanes 0-6 write)
        double cur[7], nxt[7];
        for (int k = 0; k < 7; ++k) cur[k] = anc[k];
        for (int i = 0; i < N; ++i) {
            compose(cur, meas + 7 * (i == 0 ? 0 : i - 1), nxt);
            for (int k = 0; k < 7; ++k) cur[k] = nxt[k];
            if (lane < 7) {
                const double rv = lane == 0 ? cur[0] : lane == 1 ? cur[1] : lane == 2 ? cur[2] : lane == 3 ? cur[3] : lane == 4 ? cur[4] : lane == 5 ? cur[5] : cur[6];
                xbuf[0][i * 7 + lane] = rv;
            }
        }
        GLIO_WAVE_LDS_SYNC();
    }

    // ---------------------------------------------------------------- optimizeLocalGraph
    int term = GLIO_TRAJ_NOT_SOLVED, it = 0, ok_steps = 0, cur = 0;
    unsigned mask = 0;
    double cost = 0.0, initial = 0.0;
    if (N > 0) {
        const int n = 6 * N;
        double* x = xbuf[0];
        double* xc = xbuf[1];
        cost = evaluate(x, anc, meas, Jr, Hbuf[0], Hbuf[0] + TJ_F * 36, gbuf[0], N, lane);
        initial = cost;
        for (int i = lane; i < n; i += 64) scale[i] = tr_jacobi_scale(Hbuf[0][(i / 6) * 36 + (i % 6) * 7]);
        GLIO_WAVE_LDS_SYNC();
        double radius = TR_INITIAL_RADIUS, mu = TR_MIN_MU, alpha = 0.0, step_norm = 0.0, gn_norm = 0.0, g_norm = 0.0, g_dot_gn = 0.0;
        bool reuse = false;
        int invalid = 0;
        term = GLIO_TRAJ_NO_CONVERGENCE;
        if (!isfinite(cost)) term = GLIO_TRAJ_FAILURE;
        while (term == GLIO_TRAJ_NO_CONVERGENCE) {
            const double* Hd = Hbuf[cur];
            const double* Ho = Hbuf[cur] + TJ_F * 36;
            const double* g = gbuf[cur];
            double* band = Hbuf[cur ^ 1];
            const double gmax = gradient_max(x, g, N, lane);
            // (tr_iteration_gate's order, written out: through the function the loop's scalar code moved -- four more spilled SGPRs)
            if (it >= st.max_iterations) break;
            if (gmax <= TR_GRADIENT_TOLERANCE) { term = GLIO_TRAJ_GRADIENT_TOLERANCE; break; }
            if (radius <= TR_MIN_RADIUS) { term = GLIO_TRAJ_MIN_RADIUS; break; }
            ++it;
            bool have_step = true;
            if (!reuse) {
                // D = sqrt(clip(diag Hs)), grad = gs / D, alpha = |grad|^2 / (u^T Hs u) with u = grad / D
                for (int i = lane; i < n; i += 64) {
                    const double hs = (scale[i] * Hd[(i / 6) * 36 + (i % 6) * 7]) * scale[i];          // (s h) s here, s s h in the window and the batch stage
                    const double d = sqrt(tr_clip_diagonal_minmax(hs));                                // min/max: a NaN becomes the lower bound here
                    Dd[i] = d;
                    grad[i] = (scale[i] * g[i]) / d;
                    step[i] = grad[i] / d;              // u, for now
                }
                GLIO_WAVE_LDS_SYNC();
                hs_mul(Hd, Ho, scale, step, tmp, N, lane);
                const double gg = vdot(grad, grad, n, lane);
                alpha = gg / vdot(step, tmp, n, lane);
                g_norm = sqrt(gg);
                bool solved = false;
                while (mu < TR_MAX_MU) {
                    // band = Hs + mu D^2, column j rows j .. j + 11
                    for (int e = lane; e < n * TJ_BW; e += 64) {
                        const int j = e / TJ_BW, r = e % TJ_BW, i = j + r;
                        double v = 0.0;
                        if (i < n) {
                            v = (scale[i] * h_entry(Hd, Ho, i, j)) * scale[j];
                            if (r == 0) v = v + (mu * Dd[j]) * Dd[j];
                        }
                        band[e] = v;
                    }
                    for (int i = lane; i < n; i += 64) tmp[i] = scale[i] * g[i];
                    GLIO_WAVE_LDS_SYNC();
                    bool good = true;
                    for (int j = 0; j < n; ++j) {
                        double d = band[j * TJ_BW];
                        if (!(d > 0.0)) { good = false; break; }
                        d = sqrt(d);
                        if (lane < TJ_BW) band[j * TJ_BW + lane] = lane == 0 ? d : band[j * TJ_BW + lane] / d;
                        GLIO_WAVE_LDS_SYNC();
                        for (int e = lane; e < 121; e += 64) {          // (c, r), 1 <= c <= r <= 11: entry (j + r, j + c) -= L(j + r, j) L(j + c, j)
                            const int c = 1 + e / 11, r = 1 + e % 11;
                            if (c <= r && j + c < n) band[(j + c) * TJ_BW + (r - c)] -= band[j * TJ_BW + r] * band[j * TJ_BW + c];
                        }
                        GLIO_WAVE_LDS_SYNC();
                    }
                    if (good) {
                        for (int j = 0; j < n; ++j) {          // L y = gs
                            const double yj = tmp[j] / band[j * TJ_BW];
                            GLIO_WAVE_LDS_SYNC();
                            if (lane == 0) tmp[j] = yj;
                            else if (lane < TJ_BW && j + lane < n) tmp[j + lane] -= band[j * TJ_BW + lane] * yj;
                            GLIO_WAVE_LDS_SYNC();
                        }
                        for (int j = n - 1; j >= 0; --j) {     // L^T y' = y
                            double s = tmp[j];
                            for (int r = 1; r < TJ_BW; ++r) if (j + r < n) s -= band[j * TJ_BW + r] * tmp[j + r];
                            s = s / band[j * TJ_BW];
                            GLIO_WAVE_LDS_SYNC();
                            if (lane == 0) tmp[j] = s;
                            GLIO_WAVE_LDS_SYNC();
                        }
                        bool fin = true;
                        for (int i = lane; i < n; i += 64) fin = fin && isfinite(tmp[i]);
                        good = !__any(!fin);
                    }
                    if (good) { solved = true; break; }
                    mu *= TR_MU_INCREASE;
                }
                if (solved) {
                    for (int i = lane; i < n; i += 64) gn[i] = -Dd[i] * tmp[i];
                    GLIO_WAVE_LDS_SYNC();
                    gn_norm = sqrt(vdot(gn, gn, n, lane));
                    g_dot_gn = vdot(grad, gn, n, lane);
                    reuse = true;
                } else have_step = false;
            }
            double mcc = -1.0;
            if (have_step) {
                // the traditional dogleg in the D-scaled variables: step = c_g grad + c_n gn
                // (the squared norms go in as the squares of the rounded roots, not as the sums: this loop's bits)
                double c_g, c_n, sn;
                tr_dogleg_coeffs(false, 0.0, 0.0, g_dot_gn, g_norm, gn_norm, radius, alpha, c_g, c_n, sn, true);
                step_norm = sn;
                for (int i = lane; i < n; i += 64) {
                    const double s = c_n == 0.0 ? c_g * grad[i] : (c_g == 0.0 ? gn[i] : c_g * grad[i] + c_n * gn[i]);
                    tmp[i] = s;                          // D-space, for its norm
                    step[i] = s / Dd[i];
                }
                GLIO_WAVE_LDS_SYNC();
                if (step_norm < 0.0) step_norm = sqrt(vdot(tmp, tmp, n, lane));
                hs_mul(Hd, Ho, scale, step, tmp, N, lane);
                double lin = 0.0;
                for (int i = lane; i < n; i += 64) lin += (scale[i] * g[i]) * step[i];
                lin = wave_sum(lin);
                mcc = -(lin + 0.5 * vdot(step, tmp, n, lane));
            }
            if (!have_step || !(mcc > 0.0)) {
                if (tr_invalid_limit(++invalid)) { term = GLIO_TRAJ_FAILURE; break; }
                mu *= TR_MU_INCREASE; reuse = false;
                continue;
            }
            invalid = 0;
            // candidate = Plus(x, step * scale)
            for (int k = lane; k < N; k += 64) {
                for (int c = 0; c < 3; ++c) xc[7 * k + c] = x[7 * k + c] + step[6 * k + c] * scale[6 * k + c];
                const double d[3] = {step[6 * k + 3] * scale[6 * k + 3], step[6 * k + 4] * scale[6 * k + 4], step[6 * k + 5] * scale[6 * k + 5]};
                double o[4];
                d_quat_plus(x + 7 * k + 3, d, o);
                for (int c = 0; c < 4; ++c) xc[7 * k + 3 + c] = o[c];
            }
            GLIO_WAVE_LDS_SYNC();
            const double ccost = evaluate(xc, anc, meas, Jr, Hbuf[cur ^ 1], Hbuf[cur ^ 1] + TJ_F * 36, gbuf[cur ^ 1], N, lane);
            if (!isfinite(ccost)) { radius = tr_dogleg_rejected_radius(radius); reuse = true; continue; }
            double dx2 = 0.0, xn2 = 0.0;
            for (int i = lane; i < 7 * N; i += 64) { const double d = x[i] - xc[i]; dx2 += d * d; xn2 += x[i] * x[i]; }
            const double dx = sqrt(wave_sum(dx2)), xn = sqrt(wave_sum(xn2));
            if (tr_parameter_converged(dx, xn, TR_PARAMETER_TOLERANCE)) { term = GLIO_TRAJ_PARAMETER_TOLERANCE; break; }
            if (tr_function_converged(cost, ccost, TR_FUNCTION_TOLERANCE)) { term = GLIO_TRAJ_FUNCTION_TOLERANCE; break; }
            const double q = tr_step_quality(cost, ccost, mcc);
            if (tr_step_accepted(q, TR_MIN_RELATIVE_DECREASE)) {
                double* t = x; x = xc; xc = t;
                cur ^= 1;
                ++ok_steps;
                if (it <= 32) mask |= 1u << (it - 1);
                radius = tr_dogleg_accepted_radius(q, step_norm, radius);
                mu = tr_mu_accepted(mu);
                reuse = false;
                cost = ccost;
            } else {
                radius = tr_dogleg_rejected_radius(radius); reuse = true;
            }
        }
        for (int i = lane; i < 7 * N; i += 64) { const double v = x[i]; g_sol[i] = v; finite = finite && isfinite(v); }
        finite = finite && isfinite(cost) && isfinite(initial);
    }
    const bool bad = __any(!finite);
    if (lane == 0) {
        g_sum->termination = term; g_sum->iterations = it; g_sum->successful_steps = ok_steps; g_sum->n_frames = N;
        g_sum->accepted_mask = mask; g_sum->flag = bad ? 1 : 0; g_sum->initial_cost = initial; g_sum->final_cost = cost;
    }
}

size_t round64(size_t v) { return (v + 63) & ~(size_t)63; }
bool finite_n(const double* p, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false; return true; }
bool zero_quat(const double* row) { return row[3] * row[3] + row[4] * row[4] + row[5] * row[5] + row[6] * row[6] == 0.0; }

}  // namespace

struct glio_traj {
    int device;
    glio_traj_opts o;
    hipStream_t stream, rd_stream;
    hipEvent_t ev_t0, ev_t1, ev_copied, ev_resolve;
    bool copying;
    int timed;
    TrajStore st;
    std::vector<int32_t>* h_n;          // N per gap, -1 = never pushed
    std::vector<hipEvent_t>* ev_gap;    // the end of the gap's last push (created at its first push)
    std::vector<uint8_t>* by_resolve;   // the gap's last launch was the resolve behind ev_resolve
    char* h_up; char* d_up; size_t up_cap;
    glio_traj_summary* h_sum;           // pinned, one summary
};

static int traj_upload_room(glio_traj* t, size_t need) {
    if (t->copying) { GLIO_HIP_CHECK(hipEventSynchronize(t->ev_copied)); t->copying = false; }
    if (need > t->up_cap) {
        GLIO_HIP_CHECK(hipStreamSynchronize(t->stream));
        if (t->h_up) (void)hipHostFree(t->h_up);
        if (t->d_up) (void)hipFree(t->d_up);
        t->h_up = nullptr; t->d_up = nullptr; t->up_cap = 0;
        const size_t cap = need + need / 2 + 4096;
        GLIO_HIP_CHECK(hipHostMalloc((void**)&t->h_up, cap));
        GLIO_HIP_CHECK(hipMalloc((void**)&t->d_up, cap));
        t->up_cap = cap;
    }
    return GLIO_OK;
}

extern "C" {

void glio_traj_opts_default(glio_traj_opts* o) {
    if (!o) return;
    o->max_gaps = 4096; o->max_frames_per_gap = GLIO_TRAJ_MAX_FRAMES; o->max_samples_per_gap = 4096; o->max_iterations = 15;
}
int glio_traj_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_traj_opts), (int32_t)sizeof(glio_traj_summary)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

static int traj_create_body(glio_traj* t) {
    const size_t G = (size_t)t->o.max_gaps, F = (size_t)t->o.max_frames_per_gap;
    GLIO_HIP_CHECK(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    GLIO_HIP_CHECK(hipStreamCreateWithFlags(&t->rd_stream, hipStreamNonBlocking));
    GLIO_HIP_CHECK(hipEventCreate(&t->ev_t0));
    GLIO_HIP_CHECK(hipEventCreate(&t->ev_t1));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&t->ev_copied, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&t->ev_resolve, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipMalloc((void**)&t->st.dr, G * (F + 1) * 7 * 8));
    GLIO_HIP_CHECK(hipMalloc((void**)&t->st.meas, G * (F + 1) * 7 * 8));
    GLIO_HIP_CHECK(hipMalloc((void**)&t->st.sol, (G * F * 7 + 1) * 8));
    GLIO_HIP_CHECK(hipMalloc((void**)&t->st.sum, G * sizeof(glio_traj_summary)));
    GLIO_HIP_CHECK(hipMemset(t->st.dr, 0, G * (F + 1) * 7 * 8));
    GLIO_HIP_CHECK(hipMemset(t->st.meas, 0, G * (F + 1) * 7 * 8));
    GLIO_HIP_CHECK(hipMemset(t->st.sol, 0, (G * F * 7 + 1) * 8));
    GLIO_HIP_CHECK(hipMemset(t->st.sum, 0, G * sizeof(glio_traj_summary)));
    GLIO_HIP_CHECK(hipHostMalloc((void**)&t->h_sum, sizeof(glio_traj_summary)));
    return GLIO_OK;
}
int glio_traj_create(int device, const glio_traj_opts* opts, glio_traj** out) {
    glio_traj_opts o;
    if (opts) o = *opts; else glio_traj_opts_default(&o);
    if (!out || o.max_gaps < 1 || o.max_gaps > (1 << 20) || o.max_samples_per_gap < 1 || o.max_samples_per_gap > (1 << 24) || o.max_iterations < 0 || o.max_iterations > 32) {
        glio_set_error("glio_traj_create: bad argument (max_gaps 1 .. 2^20, max_samples_per_gap 1 .. 2^24, max_iterations 0 .. 32)"); return GLIO_E_ARG;
    }
    if (o.max_frames_per_gap < 0 || o.max_frames_per_gap > GLIO_TRAJ_MAX_FRAMES) {
        glio_set_error("glio_traj_create: max_frames_per_gap %d, the kernel's LDS holds %d", o.max_frames_per_gap, GLIO_TRAJ_MAX_FRAMES); return GLIO_E_ARG;
    }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { glio_set_error("no HIP device visible: the trajectory has no CPU fallback"); return GLIO_E_HIP; }
    if (device < 0 || device >= nd) { glio_set_error("glio_traj_create: device %d of %d", device, nd); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(device));
    glio_traj* t = new glio_traj();
    memset(t, 0, sizeof *t);
    t->device = device; t->o = o;
    t->st.max_frames = o.max_frames_per_gap; t->st.max_iterations = o.max_iterations;
    t->h_n = new std::vector<int32_t>((size_t)o.max_gaps, -1);
    t->ev_gap = new std::vector<hipEvent_t>((size_t)o.max_gaps, nullptr);
    t->by_resolve = new std::vector<uint8_t>((size_t)o.max_gaps, 0);
    const int rc = traj_create_body(t);
    if (rc != GLIO_OK) { glio_traj_destroy(t); return rc; }
    *out = t;
    return GLIO_OK;
}
void glio_traj_destroy(glio_traj* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->rd_stream) (void)hipStreamSynchronize(t->rd_stream);
    if (t->st.dr) (void)hipFree(t->st.dr);
    if (t->st.meas) (void)hipFree(t->st.meas);
    if (t->st.sol) (void)hipFree(t->st.sol);
    if (t->st.sum) (void)hipFree(t->st.sum);
    if (t->d_up) (void)hipFree(t->d_up);
    if (t->h_up) (void)hipHostFree(t->h_up);
    if (t->h_sum) (void)hipHostFree(t->h_sum);
    if (t->ev_gap) { for (hipEvent_t e : *t->ev_gap) if (e) (void)hipEventDestroy(e); delete t->ev_gap; }
    if (t->ev_t0) (void)hipEventDestroy(t->ev_t0);
    if (t->ev_t1) (void)hipEventDestroy(t->ev_t1);
    if (t->ev_copied) (void)hipEventDestroy(t->ev_copied);
    if (t->ev_resolve) (void)hipEventDestroy(t->ev_resolve);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    if (t->rd_stream) (void)hipStreamDestroy(t->rd_stream);
    delete t->h_n; delete t->by_resolve;
    delete t;
}

int glio_traj_push_gap(glio_traj* t, int gap, int n_frames, const int32_t* seg_offset, const glio_imu_sample* samples, const double* start_state,
                       const double* gravity, const double* prev_row, const double* anchor_left, const double* anchor_right) {
    static_assert(sizeof(glio_imu_sample) == 56, "a sample is 7 doubles");
    if (!t || !seg_offset || !start_state || !gravity || !prev_row || !anchor_left || !anchor_right) { glio_set_error("glio_traj_push_gap: null argument"); return GLIO_E_ARG; }
    if (gap < 0 || gap >= t->o.max_gaps) { glio_set_error("glio_traj_push_gap: gap %d of a store of %d", gap, t->o.max_gaps); return GLIO_E_ARG; }
    if (n_frames < 0 || n_frames > t->o.max_frames_per_gap) { glio_set_error("glio_traj_push_gap: gap %d has %d frames, the store takes %d per gap", gap, n_frames, t->o.max_frames_per_gap); return GLIO_E_ARG; }
    const int n_seg = n_frames + 1;
    if (seg_offset[0] < 0) { glio_set_error("glio_traj_push_gap: negative sample offset"); return GLIO_E_ARG; }
    for (int s = 0; s < n_seg; ++s)
        if (seg_offset[s + 1] <= seg_offset[s]) { glio_set_error("glio_traj_push_gap: gap %d segment %d has no start row (or its offsets decrease)", gap, s); return GLIO_E_ARG; }
    const int s0 = seg_offset[0];
    const long long total = (long long)seg_offset[n_seg] - s0;
    if (total > t->o.max_samples_per_gap) { glio_set_error("glio_traj_push_gap: gap %d has %lld sample rows, the store takes %d per gap", gap, total, t->o.max_samples_per_gap); return GLIO_E_ARG; }
    if (!samples) { glio_set_error("glio_traj_push_gap: null samples"); return GLIO_E_ARG; }
    if (!finite_n(start_state, 15) || !finite_n(gravity, 3) || !finite_n(prev_row, 7) || !finite_n(anchor_left, 7) || !finite_n(anchor_right, 7) ||
        !finite_n(reinterpret_cast<const double*>(samples + s0), (int)total * 7)) {
        glio_set_error("glio_traj_push_gap: gap %d: non-finite input", gap); return GLIO_E_ARG;
    }
    if (zero_quat(prev_row) || zero_quat(anchor_left) || zero_quat(anchor_right)) { glio_set_error("glio_traj_push_gap: gap %d: zero quaternion", gap); return GLIO_E_ARG; }
    for (long long i = 0; i < total; ++i)
        if (samples[s0 + i].dt < 0) { glio_set_error("glio_traj_push_gap: gap %d: row %lld has dt < 0", gap, i); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(t->device));
    const size_t hdr_b = round64(TJ_HDR * 8), off_b = round64((size_t)(n_seg + 1) * 4), smp_b = round64((size_t)total * 56 + 8);
    const size_t need = hdr_b + off_b + smp_b;
    { const int rc = traj_upload_room(t, need); if (rc != GLIO_OK) return rc; }
    if (!(*t->ev_gap)[gap]) GLIO_HIP_CHECK(hipEventCreateWithFlags(&(*t->ev_gap)[gap], hipEventDisableTiming));
    double* hh = reinterpret_cast<double*>(t->h_up);
    memcpy(hh, start_state, 15 * 8); memcpy(hh + 15, gravity, 3 * 8); memcpy(hh + 18, prev_row, 7 * 8);
    memcpy(hh + 25, anchor_left, 7 * 8); memcpy(hh + 32, anchor_right, 7 * 8);
    int32_t* ho = reinterpret_cast<int32_t*>(t->h_up + hdr_b);
    for (int s = 0; s <= n_seg; ++s) ho[s] = seg_offset[s] - s0;
    memcpy(t->h_up + hdr_b + off_b, samples + s0, (size_t)total * 56);
    GLIO_HIP_CHECK(hipMemcpyAsync(t->d_up, t->h_up, need, hipMemcpyHostToDevice, t->stream));
    GLIO_HIP_CHECK(hipEventRecord(t->ev_copied, t->stream));
    t->copying = true;
    GLIO_HIP_CHECK(hipEventRecord(t->ev_t0, t->stream));
    hipLaunchKernelGGL(k_traj_gap, dim3(1), dim3(64), 0, t->stream, 0, gap, n_frames, reinterpret_cast<const double*>(t->d_up),
                       reinterpret_cast<const int*>(t->d_up + hdr_b), reinterpret_cast<const double*>(t->d_up + hdr_b + off_b), (const double*)nullptr, t->st);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(t->ev_t1, t->stream));
    GLIO_HIP_CHECK(hipEventRecord((*t->ev_gap)[gap], t->stream));
    (*t->h_n)[gap] = n_frames; (*t->by_resolve)[gap] = 0;
    t->timed = 1;
    return GLIO_OK;
}

int glio_traj_resolve(glio_traj* t, int first_gap, int n_gaps, const double* keyframe_poses, glio_traj_summary* summaries) {
    if (!t || first_gap < 0 || n_gaps < 0 || (long long)first_gap + n_gaps > t->o.max_gaps) { glio_set_error("glio_traj_resolve: bad gap range"); return GLIO_E_ARG; }
    if (n_gaps == 0) return GLIO_OK;
    if (!keyframe_poses) { glio_set_error("glio_traj_resolve: null poses"); return GLIO_E_ARG; }
    if (!finite_n(keyframe_poses, (n_gaps + 1) * 7)) { glio_set_error("glio_traj_resolve: non-finite pose"); return GLIO_E_ARG; }
    for (int k = 0; k <= n_gaps; ++k)
        if (zero_quat(keyframe_poses + 7 * k)) { glio_set_error("glio_traj_resolve: pose %d has a zero quaternion", k); return GLIO_E_ARG; }
    for (int k = 0; k < n_gaps; ++k)
        if ((*t->h_n)[first_gap + k] < 0) { glio_set_error("glio_traj_resolve: gap %d was never pushed", first_gap + k); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(t->device));
    const size_t need = round64((size_t)(n_gaps + 1) * 56);
    { const int rc = traj_upload_room(t, need); if (rc != GLIO_OK) return rc; }
    memcpy(t->h_up, keyframe_poses, (size_t)(n_gaps + 1) * 56);
    GLIO_HIP_CHECK(hipMemcpyAsync(t->d_up, t->h_up, need, hipMemcpyHostToDevice, t->stream));
    GLIO_HIP_CHECK(hipEventRecord(t->ev_copied, t->stream));
    t->copying = true;
    GLIO_HIP_CHECK(hipEventRecord(t->ev_t0, t->stream));
    hipLaunchKernelGGL(k_traj_gap, dim3(n_gaps), dim3(64), 0, t->stream, 1, first_gap, 0, (const double*)nullptr, (const int*)nullptr, (const double*)nullptr,
                       reinterpret_cast<const double*>(t->d_up), t->st);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(t->ev_t1, t->stream));
    GLIO_HIP_CHECK(hipEventRecord(t->ev_resolve, t->stream));
    // an earlier resolve's gaps are behind this event too: the stream is in order
    for (int k = 0; k < n_gaps; ++k) (*t->by_resolve)[first_gap + k] = 1;
    t->timed = 1;
    if (summaries) {
        GLIO_HIP_CHECK(hipMemcpyAsync(summaries, t->st.sum + first_gap, (size_t)n_gaps * sizeof(glio_traj_summary), hipMemcpyDeviceToHost, t->stream));
        GLIO_HIP_CHECK(hipStreamSynchronize(t->stream));
    }
    return GLIO_OK;
}

int glio_traj_read(glio_traj* t, int gap, glio_traj_summary* summary, double* dead_reckoned, double* measurements, double* solved) {
    if (!t || gap < 0 || gap >= t->o.max_gaps) { glio_set_error("glio_traj_read: gap %d out of range", gap); return GLIO_E_ARG; }
    const int N = (*t->h_n)[gap];
    if (N < 0) { glio_set_error("glio_traj_read: gap %d was never pushed", gap); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(t->device));
    const size_t F = (size_t)t->o.max_frames_per_gap;
    GLIO_HIP_CHECK(hipStreamWaitEvent(t->rd_stream, (*t->by_resolve)[gap] ? t->ev_resolve : (*t->ev_gap)[gap], 0));
    GLIO_HIP_CHECK(hipMemcpyAsync(t->h_sum, t->st.sum + gap, sizeof(glio_traj_summary), hipMemcpyDeviceToHost, t->rd_stream));
    if (dead_reckoned) GLIO_HIP_CHECK(hipMemcpyAsync(dead_reckoned, t->st.dr + (size_t)gap * (F + 1) * 7, (size_t)(N + 1) * 56, hipMemcpyDeviceToHost, t->rd_stream));
    if (measurements) GLIO_HIP_CHECK(hipMemcpyAsync(measurements, t->st.meas + (size_t)gap * (F + 1) * 7, (size_t)(N + 1) * 56, hipMemcpyDeviceToHost, t->rd_stream));
    if (solved && N > 0) GLIO_HIP_CHECK(hipMemcpyAsync(solved, t->st.sol + (size_t)gap * F * 7, (size_t)N * 56, hipMemcpyDeviceToHost, t->rd_stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(t->rd_stream));
    if (summary) *summary = *t->h_sum;
    if (t->h_sum->flag) { glio_set_error("trajectory gap %d: a non-finite value arose on the device", gap); return GLIO_E_NUMERIC; }
    return GLIO_OK;
}

int glio_traj_last_device_ms(glio_traj* t, float* ms) {
    if (!t || !ms) return GLIO_E_ARG;
    if (!t->timed) { glio_set_error("glio_traj_push_gap first"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(t->device));
    GLIO_HIP_CHECK(hipEventSynchronize(t->ev_t1));
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, t->ev_t0, t->ev_t1));
    return GLIO_OK;
}

}  // extern "C"

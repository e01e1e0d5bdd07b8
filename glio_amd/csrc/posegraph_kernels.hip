// posegraph_kernels.hip -- the pose graph on the device (glio_pgraph_*): the global graph (reference GLIO/src/Estimator.cpp:4586-4652, :5251-5256) and the
// local graph (:4561-4581, addLIOFactor :1999-2043, addGNSSFactor :1915-1997) that the reference keeps in one gtsam::ISAM2.  The factor definitions, the
// retraction and the termination are stated in include/glio_hip.h; everything here is fp64.
//
// One Gauss-Newton iteration:
//   k_pg_lin_nodes    one thread per node i: the chain edge (i-1, i), the chain edge (i, i+1) and the node's unary factors (prior first, then GPS factors in
//                     insertion order) are evaluated with analytic Jacobians and summed IN THAT ORDER into the node's diagonal block D_i, its coupling
//                     C_i = H[i][i+1] and its gradient g_i; the node's share of the error is the edge (i, i+1) and its unary factors.  No atomics.
//   k_pg_lin_loops    one thread per loop edge: its own 12x12 contribution (H_ii, H_ij, H_jj, g_i, g_j) and error
//   k_pg_error        one workgroup: the total error in a fixed order (strided partial sums, an LDS tree, the loops one after the other), and the
//                     termination test of the iteration that just ended (gtsam::checkConvergence on the error, never on the step)
//   k_pg_segments     one wavefront per segment (the chain strictly between two separators): block elimination from the left, the spike E to the left
//                     separator carried along.  Thirteen lanes each factor the 6x6 pivot block redundantly in registers and solve one of the columns of
//                     [C_i | E_i | g_i]; 36 + 6 lanes then form the next pivot block, the next spike and the Schur sums.  What the back-substitution needs
//                     (D^-1 C, D^-1 E, D^-1 g: 78 numbers per node) is kept.
//   k_pg_sep_zero / k_pg_sep_assemble    the separator system: per separator its diagonal block, its coupling to the previous separator and its gradient
//                     are gathered per destination (own block, left segment, right segment, the loops in insertion order)
//   k_pg_sep_factor   ONE workgroup: right-looking Cholesky of the separator system in its own storage -- a band of two 6x6 blocks per row, and full rows
//                     for the separators that are the later end of a loop (fill stays inside: eliminating column k touches the rest of its block, the
//                     next block and the full rows that have begun) -- with the right-hand sides carried as extra rows (the forward substitution), then the
//                     backward substitution, one wavefront per right-hand side
//   k_pg_backsub      one wavefront per segment, right to left: x_i = -D^-1 g - D^-1 C x_{i+1} - D^-1 E x_left
//   k_pg_update       x [+] delta per node; unit quaternions with w >= 0
// Interior nodes first, separators last, each in index order: one exact Cholesky in one fixed order.  Every kernel returns at once when the device has
// decided that the solve is over, so glio_pgraph_solve enqueues its iterations ahead (the first 12, then -- for a solve that needs them -- all the rest) and
// waits once for each of the two batches.
//
// One trial of the damped solve (glio_pgraph_solve_damped, include/glio_pgraph_lm.h), enqueued ahead the same way:
//   k_pg_lin_nodes / k_pg_lin_loops at x -- skipped while the tables still hold that linearisation (the start of a solve, and after an accepted trial)
//   k_pg_damping      d_i / rho from the node's complete diagonal, and its complete gradient: the one definition the next three use
//   the linear solve above with d / rho on the diagonal blocks of k_pg_segments and k_pg_sep_assemble; k_pg_backsub
//   k_pg_update       into the candidate table, with the node's share of the model decrease
//   k_pg_lin_nodes / k_pg_lin_loops at the candidate
//   k_pg_lm_decide    one workgroup: the candidate's error and the model decrease in k_pg_error's fixed order, the gain, the radius, the history, the termination
//   k_pg_lm_commit    the accepted candidate becomes x
//
// The covariance of every node (glio_pgraph_covariance_all, include/glio_pgraph_cov.h): one factorisation with the plan of a solve and no right-hand side, then
// the Takahashi recurrence over that factor's own pattern:
//   k_pg_segments<true>   the segment kernel's second instantiation: beside Y it keeps D~_i^-1 (six more lanes solve for the unit vectors), the segment's
//                     smallest and largest squared pivot and the node of a failed one
//   k_pg_sep_inverse  ONE workgroup, behind k_pg_sep_factor: Z = (L L^T)^-1 on L's pattern, columns n - 1 .. 0 over pg_rowset's row sets
//   k_pg_cov_sweep    one wavefront per separator: its diagonal block of Z, then down the segment to its right from the blocks of Z at both ends:
//                     Sigma_{i,N} = -Y' Sigma_{N,N}, Sigma_ii = D~_i^-1 - Sigma_{i,N} Y'^T with N(i) = {i + 1, the left separator}
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "glio_device.h"
#include "../../include/glio_pgraph_cov.h"
#include "tr_math.h"
#include "tr_math_device.h"

#define PG_MAX_LOOPS 1024
#define PG_SEP_THREADS 1024
#define PG_COV_LDS 512          /* k_pg_sep_inverse: the longest column (rows below the diagonal) it keeps in LDS */
#define PG_AHEAD 12               /* iterations enqueued before the first wait of a solve */
#define PG_YS 78                /* per interior node: D^-1 C (36), D^-1 E (36), D^-1 g (6) */
#define PG_SEGS 120             /* per segment: S_LL (36), S_LR (36), S_RR (36), g_L (6), g_R (6) */
#define PG_LOOP_OUT 121         /* per loop: H_ii, H_ij, H_jj (36 each), g_i, g_j (6 each), error */
#define PG_UNARY_PRIOR 0
#define PG_UNARY_GPS 1

struct PgCtl {
    double err;                 // the last k_pg_error's sum
    double err_cur, err0;
    int done, reason, iterations, pivot_fail;
    double cov[36];
    // the damped solve (k_pg_lm_decide): the radius the NEXT trial uses, the factor its rejection divides by, the counters; lin_fresh: D, C, g, lp_out are the
    // linearisation at x (the start of a solve, and after an accepted trial, whose candidate they were evaluated at); commit_trial: the trial whose candidate
    // k_pg_lm_commit copies into x
    double radius, decrease_factor;
    int accepted, rejected, invalid, lin_fresh, commit_trial, pad_;
    // glio_pgraph_covariance_all (k_pg_sep_inverse): the squared diagonal of the factor, the node of the first pivot that failed
    double min_pivot, max_pivot;
    int bad_node, pad2_;
};
// glio_pgraph_lm_opts as the decision kernel takes it
struct PgLm { double max_radius, min_radius, min_relative_decrease, min_diagonal, max_diagonal; int max_trials; };

// ------------------------------------------------------------------------------------------------------------------------------------ small algebra
__host__ __device__ static inline void pg_qmul(const double* a, const double* b, double* o) {
    const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    const double y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    const double z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
__host__ __device__ static inline void pg_qconj(const double* a, double* o) { o[0] = a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = -a[3]; }
// row major R of a unit quaternion
__host__ __device__ static inline void pg_qmat(const double* q, double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - w * z);     R[2] = 2 * (x * z + w * y);
    R[3] = 2 * (x * y + w * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - w * x);
    R[6] = 2 * (x * z - w * y);     R[7] = 2 * (y * z + w * x);     R[8] = 1 - 2 * (x * x + y * y);
}
__host__ __device__ static inline void pg_mtv(const double* R, const double* v, double* o) {      // R^T v
    const double a = R[0] * v[0] + R[3] * v[1] + R[6] * v[2], b = R[1] * v[0] + R[4] * v[1] + R[7] * v[2], c = R[2] * v[0] + R[5] * v[1] + R[8] * v[2];
    o[0] = a; o[1] = b; o[2] = c;
}
__host__ __device__ static inline void pg_mv(const double* R, const double* v, double* o) {
    const double a = R[0] * v[0] + R[1] * v[1] + R[2] * v[2], b = R[3] * v[0] + R[4] * v[1] + R[5] * v[2], c = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
    o[0] = a; o[1] = b; o[2] = c;
}
// Log of a unit quaternion (include/glio_hip.h)
__host__ __device__ static inline void pg_log(const double* qin, double* phi) {
    double w = qin[0], x = qin[1], y = qin[2], z = qin[3];
    if (w < 0) { w = -w; x = -x; y = -y; z = -z; }
    const double s = sqrt(x * x + y * y + z * z);
    double k;
    if (s < 1e-3) { const double u = s / w, u2 = u * u; k = 2.0 / w * (1.0 - u2 / 3.0 + u2 * u2 / 5.0); }
    else k = 2.0 * atan2(s, w) / s;
    phi[0] = k * x; phi[1] = k * y; phi[2] = k * z;
}
// the inverse right Jacobian of SO(3), row major
__host__ __device__ static inline void pg_jrinv(const double* p, double* J) {
    const double t2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    double c;
    if (t2 < 1e-4) c = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
    else { const double t = sqrt(t2); c = 1.0 / t2 - (1.0 + cos(t)) / (2.0 * t * sin(t)); }
    const double x = p[0], y = p[1], z = p[2];
    // [p]x^2 = p p^T - |p|^2 I
    J[0] = 1 + c * (x * x - t2);     J[1] = -0.5 * z + c * x * y;     J[2] = 0.5 * y + c * x * z;
    J[3] = 0.5 * z + c * x * y;      J[4] = 1 + c * (y * y - t2);     J[5] = -0.5 * x + c * y * z;
    J[6] = -0.5 * y + c * x * z;     J[7] = 0.5 * x + c * y * z;      J[8] = 1 + c * (z * z - t2);
}
// Exp as a unit quaternion
__host__ __device__ static inline void pg_exp(const double* d, double* q) {
    const double t2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    double k;
    if (t2 < 1e-6) k = 0.5 - t2 / 48.0 + t2 * t2 / 3840.0;
    else { const double t = sqrt(t2); k = sin(0.5 * t) / t; }
    q[0] = cos(0.5 * sqrt(t2)); q[1] = k * d[0]; q[2] = k * d[1]; q[3] = k * d[2];
}

// between factor (xi, xj; meas; w = 1 / sqrt(var)): whitened residual and Jacobians (row major 6x6, tangent rotation first)
__device__ static inline void pg_between(const double* xi, const double* xj, const double* m, const double* w, double* r, double* Ji, double* Jj) {
    double qi_c[4], qm_c[4], qij[4], qe[4];
    pg_qconj(xi + 3, qi_c); pg_qconj(m + 3, qm_c);
    pg_qmul(qi_c, xj + 3, qij);
    pg_qmul(qm_c, qij, qe);
    double phi[3];
    pg_log(qe, phi);
    double Ri[9], Rm[9], Rij[9], E[9], Jr[9];
    pg_qmat(xi + 3, Ri); pg_qmat(m + 3, Rm); pg_qmat(qij, Rij); pg_qmat(qe, E);
    pg_jrinv(phi, Jr);
    const double dt[3] = {xj[0] - xi[0], xj[1] - xi[1], xj[2] - xi[2]};
    double u[3], e[3];
    pg_mtv(Ri, dt, u);
    const double um[3] = {u[0] - m[0], u[1] - m[1], u[2] - m[2]};
    pg_mtv(Rm, um, e);
    for (int k = 0; k < 3; ++k) { r[k] = w[k] * phi[k]; r[3 + k] = w[3 + k] * e[k]; }
    for (int k = 0; k < 36; ++k) { Ji[k] = 0; Jj[k] = 0; }
    // [u]x
    const double ux[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s1 = 0, s2 = 0;
            for (int k = 0; k < 3; ++k) { s1 += Jr[3 * a + k] * Rij[3 * b + k]; s2 += Rm[3 * k + a] * ux[3 * k + b]; }
            Ji[6 * a + b] = -w[a] * s1;                         // -Jr^-1 Rij^T
            Ji[6 * (3 + a) + b] = w[3 + a] * s2;                // Rm^T [u]x
            Ji[6 * (3 + a) + 3 + b] = -w[3 + a] * Rm[3 * b + a];    // -Rm^T
            Jj[6 * a + b] = w[a] * Jr[3 * a + b];
            Jj[6 * (3 + a) + 3 + b] = w[3 + a] * E[3 * a + b];
        }
}
// prior (x; meas; w)
__device__ static inline void pg_prior(const double* x, const double* m, const double* w, double* r, double* J) {
    double qm_c[4], qe[4], phi[3], Rm[9], E[9], Jr[9], e[3];
    pg_qconj(m + 3, qm_c);
    pg_qmul(qm_c, x + 3, qe);
    pg_log(qe, phi);
    pg_qmat(m + 3, Rm); pg_qmat(qe, E);
    pg_jrinv(phi, Jr);
    const double dt[3] = {x[0] - m[0], x[1] - m[1], x[2] - m[2]};
    pg_mtv(Rm, dt, e);
    for (int k = 0; k < 3; ++k) { r[k] = w[k] * phi[k]; r[3 + k] = w[3 + k] * e[k]; }
    for (int k = 0; k < 36; ++k) J[k] = 0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { J[6 * a + b] = w[a] * Jr[3 * a + b]; J[6 * (3 + a) + 3 + b] = w[3 + a] * E[3 * a + b]; }
}
// H += J^T J (6x6), g += J^T r
__device__ static inline void pg_acc_self(const double* J, const double* r, double* H, double* g) {
    for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < 6; ++b) {
            double s = 0;
            for (int k = 0; k < 6; ++k) s += J[6 * k + a] * J[6 * k + b];
            H[6 * a + b] += s;
        }
        double s = 0;
        for (int k = 0; k < 6; ++k) s += J[6 * k + a] * r[k];
        g[a] += s;
    }
}
__device__ static inline void pg_cross(const double* Ja, const double* Jb, double* H) {        // H = Ja^T Jb
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0;
            for (int k = 0; k < 6; ++k) s += Ja[6 * k + a] * Jb[6 * k + b];
            H[6 * a + b] = s;
        }
}

// ------------------------------------------------------------------------------------------------------------------------------------ tables
struct PgGraph {
    int N, U, L;
    const double* x;            // [N][7] t, q
    const double* cm;           // [N][7] measurement of the chain edge INTO node i (i >= 1)
    const double* cw;           // [N][6] its 1 / sqrt(var)
    const int* un_node;         // [U] sorted by node, insertion order within a node (the prior of node 0 first)
    const int* un_type;
    const double* un_m;         // [U][7]
    const double* un_w;         // [U][6]
    const int* lp_i; const int* lp_j;
    const double* lp_m;         // [L][7]
    const double* lp_w;         // [L][6]
};
struct PgLin { double* D; double* C; double* g; double* nerr; double* lp_out; };
// the elimination's plan (host) and storage
struct PgPlan {
    int S, nW, nrhs, n;         // separators, full-row separators, right-hand sides, n = 6 S
    int cov_sep;                // the separator whose block of the inverse is asked (nrhs == 6), else -1
    const int* sep_node;        // [S] ascending
    const int* sep_w;           // [S] index among the full-row separators, or -1
    const int* w_blk;           // [nW] ascending separator index
    const int* w_lo;            // [nW] the earliest separator it is linked to
    const int* lp_si; const int* lp_sj;     // [L] separator index of either end
    const int* sl_off;          // [S + 1] the loops at a separator, insertion order ...
    const int* sl_idx;          // ... 2 * loop + (0: the separator is the loop's i, 1: its j)
    double* Y;                  // [N][PG_YS]
    double* seg;                // [S - 1][PG_SEGS]
    double* band;               // [n][12]
    double* wide;               // [6 nW + nrhs][n]
    double* ldiag;              // [n]
    double* delta;              // [N][6]
    const double* dr;           // [N][6] the damping d_i / rho of a damped trial (k_pg_damping), null for an undamped solve
};

// what the covariance of every node keeps of the forward pass (k_pg_segments<true>)
struct PgCovSeg {
    double* dinv;               // [N][36] D~_i^-1 of every interior node
    double* piv;                // [S - 1][2] the smallest and the largest squared pivot of the segment's 6x6 factors
    int* bad;                   // [S - 1] the node whose pivot was not positive and finite, or -1 (set by the host before the launch)
};

__device__ static inline double* pg_A(const PgPlan& p, int r, int c) {
    if (r >= p.n) return p.wide + (size_t)(6 * p.nW + (r - p.n)) * p.n + c;
    const int b = r / 6, w = p.sep_w[b];
    if (w >= 0) return p.wide + (size_t)(6 * w + (r - 6 * b)) * p.n + c;
    return p.band + (size_t)r * 12 + (c - 6 * (b - 1));
}

// ------------------------------------------------------------------------------------------------------------------------------------ linearise
// skip_fresh (both linearisation kernels): the launch at the start of a damped trial, which has nothing to do when the tables already hold the linearisation at x
__global__ void __launch_bounds__(64) k_pg_lin_nodes(PgGraph G, PgLin out, const PgCtl* ctl, int skip_fresh) {
    if (ctl->done || ctl->pivot_fail || (skip_fresh && ctl->lin_fresh)) return;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= G.N) return;
    double D[36], g[6], r[6], Ji[36], Jj[36];
    for (int k = 0; k < 36; ++k) D[k] = 0;
    for (int k = 0; k < 6; ++k) g[k] = 0;
    double err = 0;
    double xi[7];
    for (int k = 0; k < 7; ++k) xi[k] = G.x[(size_t)7 * i + k];
    if (i > 0) {
        pg_between(G.x + (size_t)7 * (i - 1), xi, G.cm + (size_t)7 * i, G.cw + (size_t)6 * i, r, Ji, Jj);
        pg_acc_self(Jj, r, D, g);
    }
    double* C = out.C + (size_t)36 * i;
    if (i + 1 < G.N) {
        pg_between(xi, G.x + (size_t)7 * (i + 1), G.cm + (size_t)7 * (i + 1), G.cw + (size_t)6 * (i + 1), r, Ji, Jj);
        pg_acc_self(Ji, r, D, g);
        double Cc[36];
        pg_cross(Ji, Jj, Cc);
        for (int k = 0; k < 36; ++k) C[k] = Cc[k];
        double s = 0;
        for (int k = 0; k < 6; ++k) s += r[k] * r[k];
        err += 0.5 * s;
    } else {
        for (int k = 0; k < 36; ++k) C[k] = 0;
    }
    // the node's unary factors: the first entry of the sorted table with un_node >= i
    int lo = 0, hi = G.U;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (G.un_node[mid] < i) lo = mid + 1; else hi = mid; }
    for (int u = lo; u < G.U && G.un_node[u] == i; ++u) {
        const double* m = G.un_m + (size_t)7 * u;
        const double* w = G.un_w + (size_t)6 * u;
        if (G.un_type[u] == PG_UNARY_PRIOR) {
            pg_prior(xi, m, w, r, Ji);
            pg_acc_self(Ji, r, D, g);
            double s = 0;
            for (int k = 0; k < 6; ++k) s += r[k] * r[k];
            err += 0.5 * s;
        } else {
            // GPS: r = t - p, J = [0 R]: J^T J = diag-weighted R^T W R in the translation block
            double R[9];
            pg_qmat(xi + 3, R);
            double rr[3], s = 0;
            for (int k = 0; k < 3; ++k) { rr[k] = w[k] * (xi[k] - m[k]); s += rr[k] * rr[k]; }
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) {
                    double h = 0;
                    for (int k = 0; k < 3; ++k) h += (w[k] * R[3 * k + a]) * (w[k] * R[3 * k + b]);
                    D[6 * (3 + a) + 3 + b] += h;
                }
                double h = 0;
                for (int k = 0; k < 3; ++k) h += (w[k] * R[3 * k + a]) * rr[k];
                g[3 + a] += h;
            }
            err += 0.5 * s;
        }
    }
    for (int k = 0; k < 36; ++k) out.D[(size_t)36 * i + k] = D[k];
    for (int k = 0; k < 6; ++k) out.g[(size_t)6 * i + k] = g[k];
    out.nerr[i] = err;
}

__global__ void __launch_bounds__(64) k_pg_lin_loops(PgGraph G, PgLin out, const PgCtl* ctl, int skip_fresh) {
    if (ctl->done || ctl->pivot_fail || (skip_fresh && ctl->lin_fresh)) return;
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= G.L) return;
    double r[6], Ji[36], Jj[36];
    pg_between(G.x + (size_t)7 * G.lp_i[l], G.x + (size_t)7 * G.lp_j[l], G.lp_m + (size_t)7 * l, G.lp_w + (size_t)6 * l, r, Ji, Jj);
    double* o = out.lp_out + (size_t)PG_LOOP_OUT * l;
    double H[36], g[6];
    for (int k = 0; k < 36; ++k) H[k] = 0;
    for (int k = 0; k < 6; ++k) g[k] = 0;
    pg_acc_self(Ji, r, H, g);
    for (int k = 0; k < 36; ++k) o[k] = H[k];
    for (int k = 0; k < 6; ++k) o[108 + k] = g[k];
    pg_cross(Ji, Jj, H);
    for (int k = 0; k < 36; ++k) o[36 + k] = H[k];
    for (int k = 0; k < 36; ++k) H[k] = 0;
    for (int k = 0; k < 6; ++k) g[k] = 0;
    pg_acc_self(Jj, r, H, g);
    for (int k = 0; k < 36; ++k) o[72 + k] = H[k];
    for (int k = 0; k < 6; ++k) o[114 + k] = g[k];
    double s = 0;
    for (int k = 0; k < 6; ++k) s += r[k] * r[k];
    o[120] = 0.5 * s;
}

// the sum of v[0 .. n) by one workgroup of 1024 threads in a fixed order: strided partial sums, an LDS tree.  Every thread calls it; every thread gets the sum.
__device__ static inline double pg_block_sum(int n, const double* v, double* sh) {
    const int t = threadIdx.x;
    double s = 0;
    for (int i = t; i < n; i += 1024) s += v[i];
    __syncthreads();                            // a second call: nobody still reads sh[0]
    sh[t] = s;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (t < h) sh[t] += sh[t + h];
        __syncthreads();
    }
    return sh[0];
}
// the convergence test on a decrease of the error from cur to e (gtsam::checkConvergence, unpinned)
__device__ static inline bool pg_error_converged(double cur, double e, double rel_tol, double abs_tol) {
    const double dec = cur - e;
    return (e <= 0.0) || (rel_tol != 0.0 && dec / cur <= rel_tol) || (dec <= abs_tol);
}

// phase -1: the sum only; 0: the start of a solve; 1: the end of an iteration (gtsam::checkConvergence, unpinned)
__global__ void __launch_bounds__(1024) k_pg_error(int N, int L, const double* nerr, const double* lp_out, PgCtl* ctl, int phase, int max_iter, double rel_tol, double abs_tol) {
    if (ctl->done) return;
    __shared__ double sh[1024];
    const int t = threadIdx.x;
    if (ctl->pivot_fail) {
        if (t == 0) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_NONPOSITIVE_PIVOT; }
        return;
    }
    double e = pg_block_sum(N, nerr, sh);
    if (t != 0) return;
    for (int l = 0; l < L; ++l) e += lp_out[(size_t)PG_LOOP_OUT * l + 120];
    ctl->err = e;
    if (phase < 0) return;
    if (phase == 0) {
        ctl->err0 = e; ctl->err_cur = e; ctl->iterations = 0;
        if (max_iter <= 0) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_ITERATION_LIMIT; }
        return;
    }
    const double cur = ctl->err_cur;
    const int it = ctl->iterations + 1;
    ctl->iterations = it;
    ctl->err_cur = e;
    if (pg_error_converged(cur, e, rel_tol, abs_tol)) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_CONVERGED; }
    else if (it >= max_iter) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_ITERATION_LIMIT; }
}

// ------------------------------------------------------------------------------------------------------------------------------------ segments
// in-register Cholesky of the symmetric 6x6 A (lower part read), then A^-1 b; returns false on a non-positive (or NaN) pivot
__device__ static inline bool pg_chol6(const double* A, double* Lm) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= Lm[6 * j + k] * Lm[6 * j + k];
        if (!(d > 0.0)) { ok = false; d = 1.0; }
        const double sd = sqrt(d), inv = 1.0 / sd;
        Lm[6 * j + j] = sd;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double s = A[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= Lm[6 * i + k] * Lm[6 * j + k];
            Lm[6 * i + j] = s * inv;
        }
    }
    return ok;
}
__device__ static inline void pg_chol6_solve(const double* Lm, double* b) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= Lm[6 * i + k] * b[k];
        b[i] = s / Lm[6 * i + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= Lm[6 * k + i] * b[k];
        b[i] = s / Lm[6 * i + i];
    }
}

// COV: the instantiation of glio_pgraph_covariance_all, which also fills cv; the solves' instantiation never touches cv
// (COV: a segment does not leave because ANOTHER one failed -- each runs to its own first failure, so that the node named afterwards, the first segment's,
// does not depend on which wavefront ran first)
template <bool COV>
__global__ void __launch_bounds__(64) k_pg_segments(PgPlan P, PgLin lin, PgCtl* ctl, PgCovSeg cv) {
    if (ctl->done || (!COV && ctl->pivot_fail)) return;
    const int k = blockIdx.x;                 // segment between separators k and k + 1
    const int lane = threadIdx.x;
    const int sL = P.sep_node[k], sR = P.sep_node[k + 1];
    const int a = sL + 1, b = sR - 1;
    double* so = P.seg + (size_t)PG_SEGS * k;
    if (b < a) {                                // no interior node: the chain edge couples the two separators directly
        if (lane < 36) { so[lane] = 0; so[36 + lane] = lin.C[(size_t)36 * sL + lane]; so[72 + lane] = 0; }
        else if (lane < 48) so[108 + lane - 36] = 0;
        if (COV && lane == 48) { cv.piv[2 * k] = DBL_MAX; cv.piv[2 * k + 1] = 0.0; }       // no pivot: neutral for the minimum and the maximum
        return;
    }
    __shared__ double sD[36], sE[36], sg[6], sC[36], sY[PG_YS];
    const int r6 = lane < 36 ? lane / 6 : (lane < 42 ? lane - 36 : 0), c6 = lane < 36 ? lane % 6 : 0;
    const bool damp = P.dr != nullptr && lane < 36 && r6 == c6;        // a damped trial: d / rho onto the diagonal of every node's block as it enters
    if (lane < 36) {
        double v = lin.D[(size_t)36 * a + lane];
        if (damp) v += P.dr[(size_t)6 * a + r6];
        sD[lane] = v; sE[lane] = lin.C[(size_t)36 * sL + 6 * c6 + r6];
    }
    else if (lane < 42) sg[lane - 36] = lin.g[(size_t)6 * a + lane - 36];
    double acc = 0;                             // lanes < 36: S_LL entry; lanes 36 .. 41: g_L entry
    double pmin = DBL_MAX, pmax = 0.0;          // COV: over the squared diagonal of the 6x6 factors (the same in every lane)
    for (int i = a; i <= b; ++i) {
        if (lane < 36) sC[lane] = lin.C[(size_t)36 * i + lane];
        __syncthreads();
        // thirteen lanes: column `lane` of D^-1 [C | E | g]
        {
            double A[36], Lm[36], col[6];
#pragma unroll
            for (int q = 0; q < 36; ++q) A[q] = sD[q];
            bool ok = pg_chol6(A, Lm);
            if (COV) {
#pragma unroll
                for (int q = 0; q < 6; ++q) { const double d2 = Lm[7 * q] * Lm[7 * q]; pmin = fmin(pmin, d2); pmax = fmax(pmax, d2); }
                ok = ok && pmax <= DBL_MAX;
            }
            if (!ok) {                          // every lane sees the same block: the whole wavefront leaves
                if (lane == 0) { ctl->pivot_fail = 1; if (COV) cv.bad[k] = i; }
                return;
            }
            if (COV && lane >= 13 && lane < 19) {       // column lane - 13 of D~_i^-1
#pragma unroll
                for (int q = 0; q < 6; ++q) col[q] = q == lane - 13 ? 1.0 : 0.0;
                pg_chol6_solve(Lm, col);
#pragma unroll
                for (int q = 0; q < 6; ++q) cv.dinv[(size_t)36 * i + 6 * q + lane - 13] = col[q];
            }
            if (lane < 13) {
#pragma unroll
                for (int q = 0; q < 6; ++q) col[q] = lane < 6 ? sC[6 * q + lane] : (lane < 12 ? sE[6 * q + lane - 6] : sg[q]);
                pg_chol6_solve(Lm, col);
                double* Yg = P.Y + (size_t)PG_YS * i;
#pragma unroll
                for (int q = 0; q < 6; ++q) {
                    const int at = lane < 6 ? 6 * q + lane : (lane < 12 ? 36 + 6 * q + lane - 6 : 72 + q);
                    sY[at] = col[q]; Yg[at] = col[q];
                }
            }
        }
        __syncthreads();
        double nD = 0, nE = 0;
        if (i < b) {
            if (lane < 36) {
                double s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { s1 += sC[6 * q + r6] * sY[6 * q + c6]; s2 += sC[6 * q + r6] * sY[36 + 6 * q + c6]; s3 += sE[6 * q + r6] * sY[36 + 6 * q + c6]; }
                double dn = lin.D[(size_t)36 * (i + 1) + lane];
                if (damp) dn += P.dr[(size_t)6 * (i + 1) + r6];
                nD = dn - s1; nE = -s2; acc -= s3;
            } else if (lane < 42) {
                double s1 = 0, s3 = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { s1 += sC[6 * q + r6] * sY[72 + q]; s3 += sE[6 * q + r6] * sY[72 + q]; }
                nD = lin.g[(size_t)6 * (i + 1) + r6] - s1; acc -= s3;
            }
        } else {
            if (lane < 36) {
                double s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { s1 += sC[6 * q + r6] * sY[6 * q + c6]; s2 += sE[6 * q + r6] * sY[6 * q + c6]; s3 += sE[6 * q + r6] * sY[36 + 6 * q + c6]; }
                acc -= s3;
                so[lane] = acc; so[36 + lane] = -s2; so[72 + lane] = -s1;
            } else if (lane < 42) {
                double s1 = 0, s3 = 0;
#pragma unroll
                for (int q = 0; q < 6; ++q) { s1 += sC[6 * q + r6] * sY[72 + q]; s3 += sE[6 * q + r6] * sY[72 + q]; }
                acc -= s3;
                so[108 + r6] = acc; so[114 + r6] = -s1;
            }
        }
        __syncthreads();
        if (i < b) {
            if (lane < 36) { sD[lane] = nD; sE[lane] = nE; }
            else if (lane < 42) sg[lane - 36] = nD;
        }
    }
    if (COV && lane == 0) { cv.piv[2 * k] = pmin; cv.piv[2 * k + 1] = pmax; }
}

__global__ void __launch_bounds__(64) k_pg_backsub(PgPlan P, const PgCtl* ctl) {
    if (ctl->done || ctl->pivot_fail) return;
    const int k = blockIdx.x, lane = threadIdx.x, r = lane % 6;
    const int sL = P.sep_node[k], sR = P.sep_node[k + 1];
    const double xl = P.delta[(size_t)6 * sL + r];
    double xn = P.delta[(size_t)6 * sR + r];
    for (int i = sR - 1; i > sL; --i) {
        const double* Y = P.Y + (size_t)PG_YS * i;
        double s = -Y[72 + r];
#pragma unroll
        for (int c = 0; c < 6; ++c) s -= Y[6 * r + c] * __shfl(xn, c);
#pragma unroll
        for (int c = 0; c < 6; ++c) s -= Y[36 + 6 * r + c] * __shfl(xl, c);
        xn = s;
        if (lane < 6) P.delta[(size_t)6 * i + r] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ separator system
__global__ void k_pg_sep_zero(PgPlan P, const PgCtl* ctl) {
    if (ctl->done || ctl->pivot_fail) return;
    const size_t nb = (size_t)P.n * 12, nw = (size_t)(6 * P.nW + P.nrhs) * P.n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb + nw; i += (size_t)gridDim.x * blockDim.x) {
        if (i < nb) P.band[i] = 0; else P.wide[i - nb] = 0;
    }
}

__global__ void __launch_bounds__(64) k_pg_sep_assemble(PgPlan P, PgLin lin, const PgCtl* ctl) {
    if (ctl->done || ctl->pivot_fail) return;
    const int k = blockIdx.x, e = threadIdx.x;
    if (e >= 42) return;
    const int s = P.sep_node[k];
    const double* segl = k > 0 ? P.seg + (size_t)PG_SEGS * (k - 1) : nullptr;
    const double* segr = k + 1 < P.S ? P.seg + (size_t)PG_SEGS * k : nullptr;
    if (e < 36) {
        const int r = e / 6, c = e % 6;
        double v = lin.D[(size_t)36 * s + e];
        if (segl) v += segl[72 + e];
        if (segr) v += segr[e];
        for (int q = P.sl_off[k]; q < P.sl_off[k + 1]; ++q) {
            const int l = P.sl_idx[q] >> 1, end = P.sl_idx[q] & 1;
            v += lin.lp_out[(size_t)PG_LOOP_OUT * l + (end ? 72 : 0) + e];
        }
        if (P.dr && c == r) v += P.dr[(size_t)6 * s + r];
        if (c <= r) *pg_A(P, 6 * k + r, 6 * k + c) = v;
        if (segl) *pg_A(P, 6 * k + r, 6 * (k - 1) + c) = segl[36 + 6 * c + r];       // H[k][k-1] = S_LR^T
        for (int q = P.sl_off[k]; q < P.sl_off[k + 1]; ++q) {
            const int l = P.sl_idx[q] >> 1, end = P.sl_idx[q] & 1;
            const int other = end ? P.lp_si[l] : P.lp_sj[l];
            if (other > k) continue;            // stored in the later separator's rows
            const double* Hij = lin.lp_out + (size_t)PG_LOOP_OUT * l + 36;
            *pg_A(P, 6 * k + r, 6 * other + c) += end ? Hij[6 * c + r] : Hij[6 * r + c];
        }
    } else {
        const int r = e - 36;
        double v = lin.g[(size_t)6 * s + r];
        if (segl) v += segl[114 + r];
        if (segr) v += segr[108 + r];
        for (int q = P.sl_off[k]; q < P.sl_off[k + 1]; ++q) {
            const int l = P.sl_idx[q] >> 1, end = P.sl_idx[q] & 1;
            v += lin.lp_out[(size_t)PG_LOOP_OUT * l + (end ? 114 : 108) + r];
        }
        if (P.cov_sep < 0) { if (P.nrhs) *pg_A(P, P.n, 6 * k + r) = -v; }       // (no right-hand side: the covariance of every node)
        else if (k == P.cov_sep) *pg_A(P, P.n + r, 6 * k + r) = 1.0;
    }
}

// the rows that eliminating a column of block b touches: block b itself, block b + 1, the full-row separators from b + 2 on that have begun, the right-hand sides
__device__ static inline int pg_rowset(const PgPlan& P, int b, int* rows, int* wtot) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int base = 6 + (b + 1 < P.S ? 6 : 0);
    if (t < 6) rows[t] = 6 * b + t;
    else if (t < base) rows[t] = 6 * (b + 1) + t - 6;
    bool on = false;
    if (t < P.nW) on = P.w_blk[t] >= b + 2 && P.w_lo[t] <= b;
    const unsigned long long m = __ballot(on);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = 0, total = 0;
    for (int w = 0; w < PG_SEP_THREADS / 64; ++w) { if (w < wave) off += wtot[w]; total += wtot[w]; }
    if (on) {
        const int at = base + 6 * (off + __popcll(m & ((1ull << lane) - 1ull)));
        for (int q = 0; q < 6; ++q) rows[at + q] = 6 * P.w_blk[t] + q;
    }
    const int m0 = base + 6 * total;
    if (t < P.nrhs) rows[m0 + t] = P.n + t;
    __syncthreads();
    return m0 + P.nrhs;
}

__global__ void __launch_bounds__(PG_SEP_THREADS) k_pg_sep_factor(PgPlan P, PgCtl* ctl) {
    if (ctl->done || ctl->pivot_fail) return;
    __shared__ int rows[12 + 6 * PG_MAX_LOOPS + 6];
    __shared__ int wtot[PG_SEP_THREADS / 64];
    const int t = threadIdx.x;
    int m = 0;
    for (int k = 0; k < P.n; ++k) {
        const int b = k / 6;
        if (k == 6 * b) m = pg_rowset(P, b, rows, wtot);
        const double piv = *pg_A(P, k, k);
        if (!(piv > 0.0)) {                     // uniform: every thread reads the same number
            if (t == 0) ctl->pivot_fail = 1;
            return;
        }
        const double d = sqrt(piv);
        const int start = k - 6 * b + 1, mm = m - start;
        if (t == 0) P.ldiag[k] = d;
        for (int q = t; q < mm; q += PG_SEP_THREADS) { double* p = pg_A(P, rows[start + q], k); *p = *p / d; }
        __syncthreads();
        for (int q = t; q < mm * mm; q += PG_SEP_THREADS) {
            const int ri = q / mm, ci = q - ri * mm;
            if (ci > ri) continue;
            const int r = rows[start + ri], c = rows[start + ci];
            if (c >= P.n) continue;
            *pg_A(P, r, c) -= *pg_A(P, r, k) * *pg_A(P, c, k);
        }
        __syncthreads();
    }
    // backward substitution, one wavefront per right-hand side, in place of the forward result in the right-hand side's row
    const int wave = t >> 6, lane = t & 63;
    for (int b = P.S - 1; b >= 0; --b) {
        m = pg_rowset(P, b, rows, wtot);
        const int mrows = m - P.nrhs;           // without the right-hand sides
        if (wave < P.nrhs) {
            double* x = P.wide + (size_t)(6 * P.nW + wave) * P.n;
            for (int k = 6 * b + 5; k >= 6 * b; --k) {
                const int start = k - 6 * b + 1;
                double s = 0;
                for (int q = start + lane; q < mrows; q += 64) { const int r = rows[q]; s += *pg_A(P, r, k) * x[r]; }
                for (int h = 32; h > 0; h >>= 1) s += __shfl_xor(s, h);
                if (lane == 0) x[k] = (x[k] - s) / P.ldiag[k];
                __threadfence_block();
            }
        }
        __syncthreads();
    }
    if (P.nrhs == 0) return;
    if (P.cov_sep < 0) {
        const double* x = P.wide + (size_t)(6 * P.nW) * P.n;
        for (int q = t; q < P.n; q += PG_SEP_THREADS) P.delta[(size_t)6 * P.sep_node[q / 6] + q % 6] = x[q];
    } else if (t < 36) {
        const int r = t / 6, c = t % 6, hi = r > c ? r : c, lo = r > c ? c : r;      // the lower triangle, mirrored: symmetric to the bit
        ctl->cov[t] = P.wide[(size_t)(6 * P.nW + lo) * P.n + 6 * P.cov_sep + hi];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ every node's covariance
// ONE workgroup, behind k_pg_sep_factor with no right-hand side: Z = (L L^T)^-1 on L's own pattern (Zp: the plan with Z's band and wide buffer, laid out as
// L's are).  Columns k = n - 1 .. 0; with I the rows below k of pg_rowset's set:  Z[I, k] = -Z[I, I] L[I, k] / L_kk,  Z_kk = 1 / L_kk^2 - L[I, k]^T Z[I, k] / L_kk.
// The pattern is closed under fill, so every Z[r, c] with r, c in I was written by a later column.  One thread per entry, one sum in ascending row order.
// Per block the rows' places in the storage are worked out once (code[]: where pg_A would look, without its load of sep_w per access): in both systems the
// wide buffer follows the band, so entry (r, c) is at band[pg_cov_at(code of r, c)].
// Before that: the factor's squared diagonal (min, max) over the separators and the segments, and -- after a failed pivot -- the node it belongs to.
__device__ static inline size_t pg_cov_at(int code, int c, int n) {
    return code >= 0 ? (size_t)n * 12 + (size_t)code * n + c : (size_t)(-1 - code) + c;
}
__global__ void __launch_bounds__(PG_SEP_THREADS) k_pg_sep_inverse(PgPlan P, PgPlan Zp, PgCovSeg cv, PgCtl* ctl) {
    __shared__ int rows[12 + 6 * PG_MAX_LOOPS + 6], code[12 + 6 * PG_MAX_LOOPS + 6];
    __shared__ int wtot[PG_SEP_THREADS / 64];
    __shared__ double smin[PG_SEP_THREADS / 64], smax[PG_SEP_THREADS / 64], sd[6];
    __shared__ double lk[2][PG_COV_LDS], zk[PG_COV_LDS];
    const int t = threadIdx.x;
    if (!ctl->pivot_fail) {
        double lo = DBL_MAX, hi = 0.0;
        for (int k = t; k < P.n; k += PG_SEP_THREADS) { const double d = P.ldiag[k], d2 = d * d; lo = fmin(lo, d2); hi = fmax(hi, d2); }
        for (int k = t; k < P.S - 1; k += PG_SEP_THREADS) { lo = fmin(lo, cv.piv[2 * k]); hi = fmax(hi, cv.piv[2 * k + 1]); }
        for (int h = 32; h > 0; h >>= 1) { lo = fmin(lo, __shfl_xor(lo, h)); hi = fmax(hi, __shfl_xor(hi, h)); }
        if ((t & 63) == 0) { smin[t >> 6] = lo; smax[t >> 6] = hi; }
        __syncthreads();
        for (int w = 0; w < PG_SEP_THREADS / 64; ++w) { lo = fmin(lo, smin[w]); hi = fmax(hi, smax[w]); }
        if (t == 0) { ctl->min_pivot = lo; ctl->max_pivot = hi; ctl->bad_node = -1; }
        if (hi <= DBL_MAX) {                    // uniform: every thread holds the same two numbers
            const double* Ls = P.band;
            double* Zs = Zp.band;
            const int n = P.n;
            for (int b = P.S - 1; b >= 0; --b) {
                const int m = pg_rowset(P, b, rows, wtot);
                for (int q = t; q < m; q += PG_SEP_THREADS) {
                    const int r = rows[q], rb = r / 6, w = P.sep_w[rb];
                    code[q] = w >= 0 ? 6 * w + (r - 6 * rb) : -1 - (r * 12 - 6 * (rb - 1));
                }
                if (t < 6) sd[t] = P.ldiag[6 * b + t];
                __syncthreads();
                // a block whose longest column fits keeps the column of L and the new column of Z in LDS (lk is double-buffered: the next column's L is
                // fetched beside the diagonal entry's sum); a longer one reads both from memory.  The same sums in the same order either way.
                const bool fits = m - 1 <= PG_COV_LDS;
                int cur = 0;
                if (fits) for (int q = t; q < m - 6; q += PG_SEP_THREADS) lk[0][q] = Ls[pg_cov_at(code[6 + q], 6 * b + 5, n)];
                __syncthreads();
                for (int k = 6 * b + 5; k >= 6 * b; --k) {
                    const int start = k - 6 * b + 1, mm = m - start, kc = code[start - 1];
                    const double d = sd[k - 6 * b];
                    for (int q = t; q < mm; q += PG_SEP_THREADS) {
                        const int r = rows[start + q], rc = code[start + q];
                        double s = 0;
#pragma unroll 8
                        for (int p = 0; p < mm; ++p) {          // (unrolled: the loads of eight terms are in flight together; the sum keeps its order)
                            const int c = rows[start + p], cc = code[start + p];
                            s += Zs[r > c ? pg_cov_at(rc, c, n) : pg_cov_at(cc, r, n)] * (fits ? lk[cur][p] : Ls[pg_cov_at(cc, k, n)]);
                        }
                        const double v = -s / d;
                        Zs[pg_cov_at(rc, k, n)] = v;
                        if (fits) zk[q] = v;
                    }
                    __syncthreads();
                    if (t == 0) {
                        double s = 0;
                        if (fits) {
                            for (int p = 0; p < mm; ++p) s += lk[cur][p] * zk[p];
                        } else {
#pragma unroll 8
                            for (int p = 0; p < mm; ++p) { const size_t at = pg_cov_at(code[start + p], k, n); s += Ls[at] * Zs[at]; }
                        }
                        Zs[pg_cov_at(kc, k, n)] = 1.0 / (d * d) - s / d;
                    } else if (fits && t >= 64 && k > 6 * b) {
                        for (int q = t - 64; q < mm + 1; q += PG_SEP_THREADS - 64) lk[cur ^ 1][q] = Ls[pg_cov_at(code[start - 1 + q], k - 1, n)];
                    }
                    __syncthreads();
                    cur ^= 1;
                }
            }
            return;
        }
    }
    // a pivot failed (the segments' kernel named its node; the separator factor left at its column: ldiag, zeroed by the host, ends there) or is not finite
    if (t != 0) return;
    int bad = -1;
    for (int k = 0; k < P.S - 1 && bad < 0; ++k) bad = cv.bad[k];
    for (int k = 0; k < P.n && bad < 0; ++k) { const double d2 = P.ldiag[k] * P.ldiag[k]; if (!(d2 > 0.0) || !(d2 <= DBL_MAX)) bad = P.sep_node[k / 6]; }
    ctl->pivot_fail = 1; ctl->bad_node = bad;
}

// One wavefront per separator k, lanes = the entries of a 6x6 block.  The separator's own block of Z is its covariance.  Then the segment to its right, from
// node sR - 1 down to sL + 1, with n the node behind i (sR at the start), L the left separator and Y_C = D~^-1 C, Y_E = D~^-1 E as k_pg_segments left them:
//   Sigma_in = -Y_C Sigma_nn - Y_E Sigma_nL^T      Sigma_iL = -Y_C Sigma_nL - Y_E Sigma_LL      Sigma_ii = D~_i^-1 - Sigma_in Y_C^T - Sigma_iL Y_E^T
// Sigma_nn, Sigma_nL, Sigma_LL are carried in LDS; they start as blocks (k+1, k+1), (k+1, k), (k, k) of Z -- adjacent separators, inside the band.  next[i] is
// Sigma_in; next[sL] is the spike Sigma_aL^T at the segment's first node a, or Z's sub-diagonal block when the segment has no interior.  Every diagonal block:
// the lower triangle, mirrored.
__global__ void __launch_bounds__(64) k_pg_cov_sweep(PgPlan P, PgPlan Zp, PgCovSeg cv, double* diag, double* next, const PgCtl* ctl) {
    if (ctl->pivot_fail) return;
    __shared__ double sNN[36], sNL[36], sLL[36], sY[72], sDi[36], sIN[36], sIL[36];
    const int k = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < 36;
    const int r = on ? lane / 6 : 0, c = on ? lane % 6 : 0, hi = r > c ? r : c, lo = r > c ? c : r;
    const int sL = P.sep_node[k];
    if (on) {
        const double v = *pg_A(Zp, 6 * k + hi, 6 * k + lo);
        diag[(size_t)36 * sL + lane] = v; sLL[lane] = v;
    }
    if (k + 1 >= P.S) return;
    const int sR = P.sep_node[k + 1];
    if (on) { sNN[lane] = *pg_A(Zp, 6 * (k + 1) + hi, 6 * (k + 1) + lo); sNL[lane] = *pg_A(Zp, 6 * (k + 1) + r, 6 * k + c); }
    double y0 = 0, y1 = 0, d0 = 0;              // the next node's Y_C, Y_E, D~^-1 entries, loaded one node ahead
    if (on && sR - 1 > sL) { const double* Y = P.Y + (size_t)PG_YS * (sR - 1); y0 = Y[lane]; y1 = Y[36 + lane]; d0 = cv.dinv[(size_t)36 * (sR - 1) + lane]; }
    for (int i = sR - 1; i > sL; --i) {
        if (on) { sY[lane] = y0; sY[36 + lane] = y1; sDi[lane] = d0; }
        if (on && i - 1 > sL) { const double* Y = P.Y + (size_t)PG_YS * (i - 1); y0 = Y[lane]; y1 = Y[36 + lane]; d0 = cv.dinv[(size_t)36 * (i - 1) + lane]; }
        __syncthreads();
        if (on) {
            double a = 0, b = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) { a += sY[6 * r + q] * sNN[6 * q + c]; b += sY[6 * r + q] * sNL[6 * q + c]; }
#pragma unroll
            for (int q = 0; q < 6; ++q) { a += sY[36 + 6 * r + q] * sNL[6 * c + q]; b += sY[36 + 6 * r + q] * sLL[6 * q + c]; }
            sIN[lane] = -a; sIL[lane] = -b;
            next[(size_t)36 * i + lane] = -a;
        }
        __syncthreads();
        double s = 0;
        if (on) {
            s = sDi[6 * hi + lo];
#pragma unroll
            for (int q = 0; q < 6; ++q) s -= sIN[6 * hi + q] * sY[6 * lo + q];
#pragma unroll
            for (int q = 0; q < 6; ++q) s -= sIL[6 * hi + q] * sY[36 + 6 * lo + q];
            diag[(size_t)36 * i + lane] = s;
        }
        __syncthreads();
        if (on) { sNN[lane] = s; sNL[lane] = sIL[lane]; }
    }
    __syncthreads();
    if (on) next[(size_t)36 * sL + lane] = sNL[6 * c + r];
}

// xo = x [+] delta per node (xo may be x).  A damped trial (dr not null) retracts into the candidate table and leaves the node's share of the model decrease,
// sum_a delta_a (dr_a delta_a - g_a) with dr = d / rho the very numbers the factorisation added and g the node's COMPLETE gradient (both from k_pg_damping), in
// nm[i]: no H delta product.
__global__ void __launch_bounds__(256) k_pg_update(int N, const double* x, double* xo, const double* delta, const PgCtl* ctl, const double* dr, const double* g, double* nm) {
    if (ctl->done || ctl->pivot_fail) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double* p = x + (size_t)7 * i;
    double* o = xo + (size_t)7 * i;
    const double* d = delta + (size_t)6 * i;
    double R[9], dq[4], q[4], dt[3];
    pg_qmat(p + 3, R);
    pg_mv(R, d + 3, dt);
    pg_exp(d, dq);
    pg_qmul(p + 3, dq, q);
    double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (q[0] < 0) nrm = -nrm;
    for (int k = 0; k < 3; ++k) o[k] = p[k] + dt[k];
    for (int k = 0; k < 4; ++k) o[3 + k] = q[k] / nrm;
    if (dr) {
        double s = 0;
        for (int k = 0; k < 6; ++k) s += d[k] * (dr[(size_t)6 * i + k] * d[k] - g[(size_t)6 * i + k]);
        nm[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------ the damped trial
// d_i / rho for every scalar unknown, d_i = clamp(H_ii, min_diagonal, max_diagonal) from the node's COMPLETE diagonal: lin.D (chain factors, prior, GPS) and, at a
// loop endpoint, the loops' diagonal blocks in insertion order -- they reach the matrix only in the separator assembly, and every loop endpoint is a separator.
// The ONE definition of the damping: k_pg_segments and k_pg_sep_assemble add these numbers, k_pg_update forms the model decrease with them.
// The node's complete gradient goes the same way into gf (lin.g holds the chain and unary share alone): what the model decrease is formed with.
__global__ void __launch_bounds__(256) k_pg_damping(int N, PgPlan P, PgLin lin, const PgCtl* ctl, double* dr, double* gf, double min_diag, double max_diag) {
    if (ctl->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int lo = 0, hi = P.S;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.sep_node[mid] < i) lo = mid + 1; else hi = mid; }
    const bool sep = lo < P.S && P.sep_node[lo] == i;
    const double rho = ctl->radius;
    for (int a = 0; a < 6; ++a) {
        double v = lin.D[(size_t)36 * i + 7 * a], gv = lin.g[(size_t)6 * i + a];
        if (sep)
            for (int q = P.sl_off[lo]; q < P.sl_off[lo + 1]; ++q) {
                const int l = P.sl_idx[q] >> 1, end = P.sl_idx[q] & 1;
                v += lin.lp_out[(size_t)PG_LOOP_OUT * l + (end ? 72 : 0) + 7 * a];
                gv += lin.lp_out[(size_t)PG_LOOP_OUT * l + (end ? 114 : 108) + a];
            }
        v = tr_clip_diagonal(v, min_diag, max_diag);
        dr[(size_t)6 * i + a] = v / rho;
        gf[(size_t)6 * i + a] = gv;
    }
}

__global__ void k_pg_lm_begin(PgCtl* ctl, double initial_radius) {
    ctl->radius = initial_radius; ctl->decrease_factor = TR_LM_DECREASE_FACTOR; ctl->lin_fresh = 1;
}

// ONE workgroup, the end of a trial: the error at the candidate and the model decrease in the fixed order of k_pg_error, then Ceres 1.14's
// LevenbergMarquardtStrategy / monotonic TrustRegionMinimizer rule (include/glio_pgraph_lm.h).  hist row: E tried, the radius used, m, 1 / 0 / -1.
__global__ void __launch_bounds__(1024) k_pg_lm_decide(int N, int L, const double* nerr, const double* lp_out, const double* nm, PgCtl* ctl, double* hist, PgLm o,
                                                       double rel_tol, double abs_tol) {
    if (ctl->done) return;
    __shared__ double sh[1024];
    const int t = threadIdx.x;
    const bool pivot = ctl->pivot_fail != 0;                    // uniform; after it the kernels of this trial returned: nerr and nm are stale
    __syncthreads();                                            // everyone has read it before thread 0 clears it
    double e = 0, m = 0;
    if (!pivot) {
        e = pg_block_sum(N, nerr, sh);
        m = 0.5 * pg_block_sum(N, nm, sh);
    }
    if (t != 0) return;
    for (int l = 0; l < L && !pivot; ++l) e += lp_out[(size_t)PG_LOOP_OUT * l + 120];
    const double cur = ctl->err_cur, rho = ctl->radius;
    const int trial = ctl->iterations + 1;
    ctl->iterations = trial;
    ctl->pivot_fail = 0;
    const bool valid = !pivot && m > 0.0 && m <= DBL_MAX;
    int verdict = valid ? 0 : -1;
    if (valid) {
        const double gain = tr_step_quality(cur, e, m);
        if (tr_step_accepted(gain, o.min_relative_decrease)) verdict = 1;        // (a candidate error that is not finite makes the gain NaN or -inf: rejected)
        if (verdict == 1) {
            ctl->radius = tr_lm_accepted_radius(rho, tr_cube_mul(2.0 * gain - 1.0), o.max_radius);          // (the pose graph cubes with products, the window with pow)
            ctl->decrease_factor = TR_LM_DECREASE_FACTOR;
            ctl->err_cur = e; ctl->accepted += 1; ctl->commit_trial = trial;
            if (pg_error_converged(cur, e, rel_tol, abs_tol)) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_CONVERGED; }
        }
    }
    ctl->lin_fresh = verdict == 1;
    if (verdict != 1) {
        ctl->rejected += 1;
        if (verdict < 0) ctl->invalid += 1;
        double r = rho, df = ctl->decrease_factor;
        tr_lm_rejected(r, df);
        ctl->radius = r; ctl->decrease_factor = df;
        if (r <= o.min_radius) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_MIN_RADIUS; }
    }
    if (!ctl->done && trial >= o.max_trials) { ctl->done = 1; ctl->reason = GLIO_PGRAPH_ITERATION_LIMIT; }
    double* h = hist + (size_t)4 * (trial - 1);
    h[0] = valid ? e : cur; h[1] = rho; h[2] = pivot ? 0.0 : m; h[3] = (double)verdict;
}

// the accepted candidate becomes the estimate; trial is the launch's own number, so the launches enqueued behind the end of a solve copy nothing
__global__ void __launch_bounds__(256) k_pg_lm_commit(int N, double* x, const double* xc, const PgCtl* ctl, int trial) {
    if (ctl->commit_trial != trial) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 7 * N) x[i] = xc[i];
}

// ------------------------------------------------------------------------------------------------------------------------------------ the object
struct glio_pgraph {
    int device;
    glio_pgraph_opts o;
    hipStream_t stream;
    hipEvent_t ev_done, ev_t[6];
    // the graph as the host holds it
    int N, n_dev;                               // nodes; nodes whose rows are already on the device
    std::vector<double> h_x, h_cm, h_cw;        // rows [n_dev, N) wait for their upload (rows below n_dev of h_x are stale: the device holds the estimate)
    int have_prior; double prior_m[7], prior_w[6];
    std::vector<int> gps_node; std::vector<double> gps_m, gps_w;
    std::vector<int> lp_i, lp_j; std::vector<double> lp_m, lp_w;
    int factors_dirty;
    // device
    double* d_x; double* d_x0; double* d_cm; double* d_cw;
    int* d_un_node; int* d_un_type; double* d_un_m; double* d_un_w; int U;
    int* d_lp_i; int* d_lp_j; double* d_lp_m; double* d_lp_w;
    double* d_D; double* d_C; double* d_g; double* d_nerr; double* d_lp_out;
    double* d_Y; double* d_seg; double* d_delta;
    int* d_plan; size_t plan_cap;               // one int block: sep_node, sep_w, w_blk, w_lo, lp_si, lp_sj, sl_off, sl_idx
    double* d_sys; size_t sys_cap;              // band, wide, ldiag
    PgCtl* d_ctl; PgCtl* h_ctl;
    // the damped solve's own tables (allocated by the first glio_pgraph_solve_damped): candidate poses, d / rho, the complete gradient, the nodes' shares of the
    // model decrease, history
    double* d_xc; double* d_dr; double* d_gf; double* d_nm; double* d_hist; size_t hist_cap;
    std::vector<double> lm_hist;                // [trials][4] of the last damped solve that returned GLIO_OK
    std::vector<double> lm_hist_in;             // where a running solve's rows arrive
    // the covariance of every node (allocated by the first glio_pgraph_covariance_all*, for cov_cap nodes): Z on the factor's pattern (band, wide), the
    // segments' record, the result on the device (diag [N][36], then next [N - 1][36]) and in pinned memory, the last call's times (five stages, the whole)
    double* d_zsys; size_t zsys_cap;
    double* d_dinv; double* d_segpiv; int* d_segbad; double* d_cov; double* h_cov; size_t cov_cap;
    float cov_ms[6]; int cov_timed;
};

#define PG_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

static bool pg_finite(const double* v, int n) {
    for (int k = 0; k < n; ++k) if (!(fabs(v[k]) <= DBL_MAX)) return false;
    return true;
}
static bool pg_var_ok(const double* v, int n) {
    for (int k = 0; k < n; ++k) if (!(v[k] > 0.0) || !(v[k] <= DBL_MAX)) return false;
    return true;
}
// t, q with q normalised and w >= 0; false for a pose that is not finite or has no rotation
static bool pg_pose_in(const double* in, double* out) {
    if (!pg_finite(in, 7)) return false;
    const double n = sqrt(in[3] * in[3] + in[4] * in[4] + in[5] * in[5] + in[6] * in[6]);
    if (!(n > 0.0) || !(n <= DBL_MAX)) return false;
    const double s = in[3] < 0 ? -n : n;
    for (int k = 0; k < 3; ++k) out[k] = in[k];
    for (int k = 0; k < 4; ++k) out[3 + k] = in[3 + k] / s;
    return true;
}
// between(a, b): t = Ra^T (tb - ta), q = qa^-1 qb
static void pg_between_meas(const double* a, const double* b, double* m) {
    double R[9], qc[4];
    pg_qmat(a + 3, R);
    const double dt[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    pg_mtv(R, dt, m);
    pg_qconj(a + 3, qc);
    pg_qmul(qc, b + 3, m + 3);
}

static int pg_flush_nodes(glio_pgraph* pg) {
    if (pg->n_dev < pg->N) {
        const size_t a = pg->n_dev, n = pg->N - pg->n_dev;
        PG_CHECK(hipMemcpyAsync(pg->d_x + 7 * a, pg->h_x.data() + 7 * a, n * 7 * 8, hipMemcpyHostToDevice, pg->stream));
        PG_CHECK(hipMemcpyAsync(pg->d_cm + 7 * a, pg->h_cm.data() + 7 * a, n * 7 * 8, hipMemcpyHostToDevice, pg->stream));
        PG_CHECK(hipMemcpyAsync(pg->d_cw + 6 * a, pg->h_cw.data() + 6 * a, n * 6 * 8, hipMemcpyHostToDevice, pg->stream));
        PG_CHECK(hipStreamSynchronize(pg->stream));     // pageable sources: nothing may change under the copy
        pg->n_dev = pg->N;
    }
    return GLIO_OK;
}
static int pg_flush_factors(glio_pgraph* pg) {
    if (!pg->factors_dirty) return GLIO_OK;
    // the unary table sorted by node, insertion order within a node, the prior of node 0 first
    const int ng = (int)pg->gps_node.size();
    std::vector<int> order(ng);
    for (int k = 0; k < ng; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pg->gps_node[a] < pg->gps_node[b]; });
    const int U = ng + (pg->have_prior ? 1 : 0);
    std::vector<int> node(U), type(U); std::vector<double> m((size_t)7 * U, 0.0), w((size_t)6 * U, 0.0);
    int at = 0;
    if (pg->have_prior) { node[0] = 0; type[0] = PG_UNARY_PRIOR; memcpy(&m[0], pg->prior_m, 56); memcpy(&w[0], pg->prior_w, 48); at = 1; }
    for (int k = 0; k < ng; ++k, ++at) {
        const int s = order[k];
        node[at] = pg->gps_node[s]; type[at] = PG_UNARY_GPS;
        memcpy(&m[(size_t)7 * at], &pg->gps_m[(size_t)3 * s], 24); memcpy(&w[(size_t)6 * at], &pg->gps_w[(size_t)3 * s], 24);
    }
    if (U) {
        PG_CHECK(hipMemcpy(pg->d_un_node, node.data(), (size_t)U * 4, hipMemcpyHostToDevice)); PG_CHECK(hipMemcpy(pg->d_un_type, type.data(), (size_t)U * 4, hipMemcpyHostToDevice));
        PG_CHECK(hipMemcpy(pg->d_un_m, m.data(), (size_t)U * 56, hipMemcpyHostToDevice)); PG_CHECK(hipMemcpy(pg->d_un_w, w.data(), (size_t)U * 48, hipMemcpyHostToDevice));
    }
    pg->U = U;
    const size_t L = pg->lp_i.size();
    if (L) {
        PG_CHECK(hipMemcpy(pg->d_lp_i, pg->lp_i.data(), L * 4, hipMemcpyHostToDevice)); PG_CHECK(hipMemcpy(pg->d_lp_j, pg->lp_j.data(), L * 4, hipMemcpyHostToDevice));
        PG_CHECK(hipMemcpy(pg->d_lp_m, pg->lp_m.data(), L * 56, hipMemcpyHostToDevice)); PG_CHECK(hipMemcpy(pg->d_lp_w, pg->lp_w.data(), L * 48, hipMemcpyHostToDevice));
    }
    pg->factors_dirty = 0;
    return GLIO_OK;
}
static PgGraph pg_graph(const glio_pgraph* pg) {
    PgGraph G;
    G.N = pg->N; G.U = pg->U; G.L = (int)pg->lp_i.size();
    G.x = pg->d_x; G.cm = pg->d_cm; G.cw = pg->d_cw;
    G.un_node = pg->d_un_node; G.un_type = pg->d_un_type; G.un_m = pg->d_un_m; G.un_w = pg->d_un_w;
    G.lp_i = pg->d_lp_i; G.lp_j = pg->d_lp_j; G.lp_m = pg->d_lp_m; G.lp_w = pg->d_lp_w;
    return G;
}
static PgLin pg_lin(const glio_pgraph* pg) { PgLin l; l.D = pg->d_D; l.C = pg->d_C; l.g = pg->d_g; l.nerr = pg->d_nerr; l.lp_out = pg->d_lp_out; return l; }

static int pg_segment_nodes(const glio_pgraph* pg) {
    if (pg->o.segment_nodes > 0) return pg->o.segment_nodes;
    const int m = (int)lround(sqrt((double)pg->N));
    return std::min(255, std::max(4, m));
}
// the separators (node 0, the last node, every loop endpoint, the node whose covariance is asked, and a node after every segment_nodes interior nodes), the
// full-row separators, the loops per separator: computed on the host, one upload.  rhs false: no right-hand side (the covariance of every node)
static int pg_make_plan(glio_pgraph* pg, int cov_node, PgPlan* P, bool rhs = true) {
    const int N = pg->N, L = (int)pg->lp_i.size(), seg = pg_segment_nodes(pg);
    std::vector<int> forced;
    forced.push_back(0); forced.push_back(N - 1);
    for (int l = 0; l < L; ++l) { forced.push_back(pg->lp_i[l]); forced.push_back(pg->lp_j[l]); }
    if (cov_node >= 0) forced.push_back(cov_node);
    std::sort(forced.begin(), forced.end());
    forced.erase(std::unique(forced.begin(), forced.end()), forced.end());
    std::vector<int> sep;
    for (size_t f = 0; f < forced.size(); ++f) {
        if (f > 0) for (long long s = (long long)forced[f - 1] + seg + 1; s < forced[f]; s += seg + 1) sep.push_back((int)s);
        sep.push_back(forced[f]);
    }
    const int S = (int)sep.size();
    auto sep_of = [&](int node) { return (int)(std::lower_bound(sep.begin(), sep.end(), node) - sep.begin()); };
    std::vector<int> lp_si(L), lp_sj(L), lo(S);
    for (int k = 0; k < S; ++k) lo[k] = k;
    std::vector<std::vector<int>> at(S);
    for (int l = 0; l < L; ++l) {
        const int a = sep_of(pg->lp_i[l]), b = sep_of(pg->lp_j[l]);
        lp_si[l] = a; lp_sj[l] = b;
        at[a].push_back(2 * l); at[b].push_back(2 * l + 1);
        const int hi = std::max(a, b), lw = std::min(a, b);
        lo[hi] = std::min(lo[hi], lw);
    }
    std::vector<int> sep_w(S, -1), w_blk, w_lo;
    for (int k = 0; k < S; ++k) if (lo[k] < k) { sep_w[k] = (int)w_blk.size(); w_blk.push_back(k); w_lo.push_back(lo[k]); }
    const int nW = (int)w_blk.size();
    std::vector<int> sl_off(S + 1, 0), sl_idx;
    for (int k = 0; k < S; ++k) { for (int v : at[k]) sl_idx.push_back(v); sl_off[k + 1] = (int)sl_idx.size(); }
    // one block of ints
    std::vector<int> blk;
    auto put = [&](const std::vector<int>& v) { const size_t o = blk.size(); blk.insert(blk.end(), v.begin(), v.end()); return o; };
    const size_t o_sep = put(sep), o_sw = put(sep_w), o_wb = put(w_blk), o_wl = put(w_lo), o_si = put(lp_si), o_sj = put(lp_sj), o_off = put(sl_off), o_idx = put(sl_idx);
    if (blk.size() > pg->plan_cap) {
        if (pg->d_plan) { hipFree(pg->d_plan); pg->d_plan = nullptr; pg->plan_cap = 0; }
        const size_t cap = blk.size() * 2;
        PG_CHECK(hipMalloc((void**)&pg->d_plan, cap * 4));
        pg->plan_cap = cap;
    }
    PG_CHECK(hipMemcpy(pg->d_plan, blk.data(), blk.size() * 4, hipMemcpyHostToDevice));
    const int nrhs = cov_node >= 0 ? 6 : (rhs ? 1 : 0), n = 6 * S;
    const size_t need = (size_t)n * 12 + (size_t)(6 * nW + nrhs) * n + n;
    if (need > pg->sys_cap) {
        if (pg->d_sys) { hipFree(pg->d_sys); pg->d_sys = nullptr; pg->sys_cap = 0; }
        const size_t cap = need + need / 2;
        PG_CHECK(hipMalloc((void**)&pg->d_sys, cap * 8));
        pg->sys_cap = cap;
    }
    P->S = S; P->nW = nW; P->nrhs = nrhs; P->n = n;
    P->cov_sep = cov_node >= 0 ? sep_of(cov_node) : -1;
    P->sep_node = pg->d_plan + o_sep; P->sep_w = pg->d_plan + o_sw; P->w_blk = pg->d_plan + o_wb; P->w_lo = pg->d_plan + o_wl;
    P->lp_si = pg->d_plan + o_si; P->lp_sj = pg->d_plan + o_sj; P->sl_off = pg->d_plan + o_off; P->sl_idx = pg->d_plan + o_idx;
    P->Y = pg->d_Y; P->seg = pg->d_seg; P->delta = pg->d_delta; P->dr = nullptr;
    P->band = pg->d_sys; P->wide = pg->d_sys + (size_t)n * 12; P->ldiag = P->wide + (size_t)(6 * nW + nrhs) * n;
    return GLIO_OK;
}

// the two linearisation kernels at the pose table x; skip_fresh: see k_pg_lin_nodes
static void pg_enqueue_lin_at(glio_pgraph* pg, const double* x, int skip_fresh) {
    PgGraph G = pg_graph(pg);
    G.x = x;
    const PgLin lin = pg_lin(pg);
    hipLaunchKernelGGL(k_pg_lin_nodes, dim3((G.N + 63) / 64), dim3(64), 0, pg->stream, G, lin, pg->d_ctl, skip_fresh);
    if (G.L) hipLaunchKernelGGL(k_pg_lin_loops, dim3((G.L + 63) / 64), dim3(64), 0, pg->stream, G, lin, pg->d_ctl, skip_fresh);
}
static void pg_enqueue_linearise(glio_pgraph* pg, int phase, int max_iter) {
    pg_enqueue_lin_at(pg, pg->d_x, 0);
    hipLaunchKernelGGL(k_pg_error, dim3(1), dim3(1024), 0, pg->stream, pg->N, (int)pg->lp_i.size(), pg->d_nerr, pg->d_lp_out, pg->d_ctl, phase, max_iter,
                       pg->o.relative_error_tol, pg->o.absolute_error_tol);
}
// segments, separator system, back-substitution of one linear solve; ev (may be null): events after the segments and after the separator system;
// cv (may be null): the segments' record for the covariance of every node
static void pg_enqueue_linear_solve(glio_pgraph* pg, const PgPlan& P, hipEvent_t* ev, const PgCovSeg* cv = nullptr) {
    const PgLin lin = pg_lin(pg);
    if (P.S > 1) {
        if (cv) hipLaunchKernelGGL(k_pg_segments<true>, dim3(P.S - 1), dim3(64), 0, pg->stream, P, lin, pg->d_ctl, *cv);
        else hipLaunchKernelGGL(k_pg_segments<false>, dim3(P.S - 1), dim3(64), 0, pg->stream, P, lin, pg->d_ctl, PgCovSeg{nullptr, nullptr, nullptr});
    }
    if (ev) hipEventRecord(ev[0], pg->stream);
    const size_t cells = (size_t)P.n * 12 + (size_t)(6 * P.nW + P.nrhs) * P.n;
    hipLaunchKernelGGL(k_pg_sep_zero, dim3((unsigned)std::min<size_t>(1024, (cells + 255) / 256)), dim3(256), 0, pg->stream, P, pg->d_ctl);
    hipLaunchKernelGGL(k_pg_sep_assemble, dim3(P.S), dim3(64), 0, pg->stream, P, lin, pg->d_ctl);
    hipLaunchKernelGGL(k_pg_sep_factor, dim3(1), dim3(PG_SEP_THREADS), 0, pg->stream, P, pg->d_ctl);
    if (ev) hipEventRecord(ev[1], pg->stream);
}

extern "C" {

void glio_pgraph_opts_default(glio_pgraph_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->relative_error_tol = 1e-5; o->absolute_error_tol = 1e-5; o->max_iterations = 100;     // gtsam::GaussNewtonParams (unpinned)
    const double p[6] = {1e-2, 1e-2, M_PI * M_PI, 1e8, 1e8, 1e8}, od[6] = {1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4};        // Estimator.cpp:864-865
    for (int k = 0; k < 6; ++k) { o->prior_var[k] = p[k]; o->odom_var[k] = od[k]; }
    o->gps_var_floor = 1.0;                 // max(noise, 1.0f), Estimator.cpp:1986
    o->max_nodes = 65536; o->max_loops = 64; o->max_unary = 4096; o->segment_nodes = 0;
}
int glio_pgraph_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_pgraph_opts), (int32_t)sizeof(glio_pgraph_info)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

void glio_pgraph_destroy(glio_pgraph* pg) {
    if (!pg) return;
    (void)hipSetDevice(pg->device);
    if (pg->stream) (void)hipStreamSynchronize(pg->stream);
    void* p[] = {pg->d_x, pg->d_x0, pg->d_cm, pg->d_cw, pg->d_un_node, pg->d_un_type, pg->d_un_m, pg->d_un_w, pg->d_lp_i, pg->d_lp_j, pg->d_lp_m, pg->d_lp_w,
                 pg->d_D, pg->d_C, pg->d_g, pg->d_nerr, pg->d_lp_out, pg->d_Y, pg->d_seg, pg->d_delta, pg->d_plan, pg->d_sys, pg->d_ctl, pg->d_xc, pg->d_dr, pg->d_gf, pg->d_nm, pg->d_hist,
                 pg->d_zsys, pg->d_dinv, pg->d_segpiv, pg->d_segbad, pg->d_cov};
    for (void* q : p) if (q) (void)hipFree(q);
    if (pg->h_ctl) (void)hipHostFree(pg->h_ctl);
    if (pg->h_cov) (void)hipHostFree(pg->h_cov);
    if (pg->ev_done) (void)hipEventDestroy(pg->ev_done);
    for (hipEvent_t e : pg->ev_t) if (e) (void)hipEventDestroy(e);
    if (pg->stream) (void)hipStreamDestroy(pg->stream);
    delete pg;
}

static int pg_create_body(glio_pgraph* pg) {
    PG_CHECK(hipStreamCreateWithFlags(&pg->stream, hipStreamNonBlocking));
    PG_CHECK(hipEventCreateWithFlags(&pg->ev_done, hipEventDisableTiming | hipEventBlockingSync));
    for (int k = 0; k < 6; ++k) PG_CHECK(hipEventCreate(&pg->ev_t[k]));
    const size_t N = (size_t)pg->o.max_nodes, U = (size_t)pg->o.max_unary + 1, L = (size_t)std::max(1, pg->o.max_loops);
    PG_CHECK(hipMalloc((void**)&pg->d_x, N * 56)); PG_CHECK(hipMalloc((void**)&pg->d_x0, N * 56));
    PG_CHECK(hipMalloc((void**)&pg->d_cm, N * 56)); PG_CHECK(hipMalloc((void**)&pg->d_cw, N * 48));
    PG_CHECK(hipMalloc((void**)&pg->d_un_node, U * 4)); PG_CHECK(hipMalloc((void**)&pg->d_un_type, U * 4));
    PG_CHECK(hipMalloc((void**)&pg->d_un_m, U * 56)); PG_CHECK(hipMalloc((void**)&pg->d_un_w, U * 48));
    PG_CHECK(hipMalloc((void**)&pg->d_lp_i, L * 4)); PG_CHECK(hipMalloc((void**)&pg->d_lp_j, L * 4));
    PG_CHECK(hipMalloc((void**)&pg->d_lp_m, L * 56)); PG_CHECK(hipMalloc((void**)&pg->d_lp_w, L * 48));
    PG_CHECK(hipMalloc((void**)&pg->d_D, N * 288)); PG_CHECK(hipMalloc((void**)&pg->d_C, N * 288)); PG_CHECK(hipMalloc((void**)&pg->d_g, N * 48));
    PG_CHECK(hipMalloc((void**)&pg->d_nerr, N * 8)); PG_CHECK(hipMalloc((void**)&pg->d_lp_out, L * PG_LOOP_OUT * 8));
    PG_CHECK(hipMalloc((void**)&pg->d_Y, N * PG_YS * 8)); PG_CHECK(hipMalloc((void**)&pg->d_seg, N * PG_SEGS * 8)); PG_CHECK(hipMalloc((void**)&pg->d_delta, N * 48));
    PG_CHECK(hipMalloc((void**)&pg->d_ctl, sizeof(PgCtl))); PG_CHECK(hipHostMalloc((void**)&pg->h_ctl, sizeof(PgCtl)));
    return GLIO_OK;
}
static void pg_reset(glio_pgraph* pg) {
    pg->N = 0; pg->n_dev = 0; pg->have_prior = 0; pg->U = 0; pg->factors_dirty = 1;
    pg->h_x.clear(); pg->h_cm.clear(); pg->h_cw.clear();
    pg->gps_node.clear(); pg->gps_m.clear(); pg->gps_w.clear();
    pg->lp_i.clear(); pg->lp_j.clear(); pg->lp_m.clear(); pg->lp_w.clear();
}

int glio_pgraph_create(int device, const glio_pgraph_opts* opts, glio_pgraph** out) {
    if (!opts || !out) { glio_set_error("glio_pgraph_create: null argument"); return GLIO_E_ARG; }
    const glio_pgraph_opts& o = *opts;
    if (o.max_nodes < 1 || o.max_nodes > (1 << 24) || o.max_loops < 0 || o.max_loops > PG_MAX_LOOPS || o.max_unary < 0 || o.max_unary > (1 << 24) || o.segment_nodes < 0 ||
        !pg_finite(&o.relative_error_tol, 1) || !pg_finite(&o.absolute_error_tol, 1) || !pg_var_ok(o.prior_var, 6) || !pg_var_ok(o.odom_var, 6) ||
        !(o.gps_var_floor >= 0.0) || !pg_finite(&o.gps_var_floor, 1)) {
        glio_set_error("bad glio_pgraph_opts (max_nodes %d, max_loops %d of at most %d, max_unary %d, segment_nodes %d, or a tolerance / variance that is not finite and positive)",
                       o.max_nodes, o.max_loops, PG_MAX_LOOPS, o.max_unary, o.segment_nodes);
        return GLIO_E_ARG;
    }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { glio_set_error("no HIP device visible: the pose graph has no CPU fallback"); return GLIO_E_HIP; }
    if (device < 0 || device >= nd) { glio_set_error("glio_pgraph_create: device %d of %d", device, nd); return GLIO_E_ARG; }
    PG_CHECK(hipSetDevice(device));
    glio_pgraph* pg = new glio_pgraph();
    pg->device = device; pg->o = o;
    pg_reset(pg);
    const int rc = pg_create_body(pg);
    if (rc != GLIO_OK) { glio_pgraph_destroy(pg); return rc; }
    *out = pg;
    return GLIO_OK;
}

int glio_pgraph_clear(glio_pgraph* pg) {
    if (!pg) return GLIO_E_ARG;
    pg_reset(pg);
    return GLIO_OK;
}

int glio_pgraph_set_prior(glio_pgraph* pg, const double pose[7], const double var[6]) {
    if (!pg || !pose) { glio_set_error("glio_pgraph_set_prior: null argument"); return GLIO_E_ARG; }
    const double* v = var ? var : pg->o.prior_var;
    double m[7];
    if (!pg_pose_in(pose, m)) { glio_set_error("glio_pgraph_set_prior: the pose is not finite (or its quaternion is zero)"); return GLIO_E_ARG; }
    if (!pg_var_ok(v, 6)) { glio_set_error("glio_pgraph_set_prior: a variance is not positive and finite"); return GLIO_E_ARG; }
    memcpy(pg->prior_m, m, 56);
    for (int k = 0; k < 6; ++k) pg->prior_w[k] = 1.0 / sqrt(v[k]);
    pg->have_prior = 1; pg->factors_dirty = 1;
    return GLIO_OK;
}

int glio_pgraph_append(glio_pgraph* pg, int n, const double* poses, const double* prev_pose, const double* var) {
    GLIO_TRACE("glio_pgraph_append");
    if (!pg || n < 1 || !poses) { glio_set_error("glio_pgraph_append: null argument or n < 1"); return GLIO_E_ARG; }
    if ((long long)pg->N + n > (long long)pg->o.max_nodes) { glio_set_error("glio_pgraph_append: %d + %d nodes, max_nodes = %d", pg->N, n, pg->o.max_nodes); return GLIO_E_ARG; }
    const double* v = var ? var : pg->o.odom_var;
    if (!pg_var_ok(v, 6)) { glio_set_error("glio_pgraph_append: a variance is not positive and finite"); return GLIO_E_ARG; }
    std::vector<double> x((size_t)7 * n), cm((size_t)7 * n, 0.0);
    for (int k = 0; k < n; ++k)
        if (!pg_pose_in(poses + (size_t)7 * k, &x[(size_t)7 * k])) { glio_set_error("glio_pgraph_append: pose %d is not finite (or its quaternion is zero)", k); return GLIO_E_ARG; }
    double prev[7];
    if (pg->N > 0) {
        if (prev_pose) {
            if (!pg_pose_in(prev_pose, prev)) { glio_set_error("glio_pgraph_append: prev_pose is not finite (or its quaternion is zero)"); return GLIO_E_ARG; }
        } else {
            PG_CHECK(hipSetDevice(pg->device));
            const int rf = pg_flush_nodes(pg);
            if (rf != GLIO_OK) return rf;
            PG_CHECK(hipMemcpy(prev, pg->d_x + (size_t)7 * (pg->N - 1), 56, hipMemcpyDeviceToHost));
        }
    }
    for (int k = 0; k < n; ++k) {
        const double* a = k > 0 ? &x[(size_t)7 * (k - 1)] : (pg->N > 0 ? prev : nullptr);
        if (a) pg_between_meas(a, &x[(size_t)7 * k], &cm[(size_t)7 * k]);
        else cm[(size_t)7 * k + 3] = 1.0;
    }
    pg->h_x.resize((size_t)7 * pg->N); pg->h_cm.resize((size_t)7 * pg->N); pg->h_cw.resize((size_t)6 * pg->N);
    pg->h_x.insert(pg->h_x.end(), x.begin(), x.end());
    pg->h_cm.insert(pg->h_cm.end(), cm.begin(), cm.end());
    for (int k = 0; k < n; ++k) for (int c = 0; c < 6; ++c) pg->h_cw.push_back(1.0 / sqrt(v[c]));
    pg->N += n;
    return GLIO_OK;
}

int glio_pgraph_add_between(glio_pgraph* pg, int i, int j, const double rel[7], const double var[6]) {
    if (!pg || !rel || !var) { glio_set_error("glio_pgraph_add_between: null argument"); return GLIO_E_ARG; }
    if (i < 0 || j < 0 || i >= pg->N || j >= pg->N || i == j) { glio_set_error("glio_pgraph_add_between: nodes %d, %d of %d (they must differ)", i, j, pg->N); return GLIO_E_ARG; }
    if ((int)pg->lp_i.size() >= pg->o.max_loops) { glio_set_error("glio_pgraph_add_between: max_loops = %d edges are held", pg->o.max_loops); return GLIO_E_ARG; }
    double m[7];
    if (!pg_pose_in(rel, m)) { glio_set_error("glio_pgraph_add_between: the measurement is not finite (or its quaternion is zero)"); return GLIO_E_ARG; }
    if (!pg_var_ok(var, 6)) { glio_set_error("glio_pgraph_add_between: a variance is not positive and finite"); return GLIO_E_ARG; }
    pg->lp_i.push_back(i); pg->lp_j.push_back(j);
    pg->lp_m.insert(pg->lp_m.end(), m, m + 7);
    for (int k = 0; k < 6; ++k) pg->lp_w.push_back(1.0 / sqrt(var[k]));
    pg->factors_dirty = 1;
    return GLIO_OK;
}

int glio_pgraph_add_gps(glio_pgraph* pg, int i, const double xyz[3], const double var[3]) {
    if (!pg || !xyz || !var) { glio_set_error("glio_pgraph_add_gps: null argument"); return GLIO_E_ARG; }
    if (i < 0 || i >= pg->N) { glio_set_error("glio_pgraph_add_gps: node %d of %d", i, pg->N); return GLIO_E_ARG; }
    if ((int)pg->gps_node.size() >= pg->o.max_unary) { glio_set_error("glio_pgraph_add_gps: max_unary = %d factors are held", pg->o.max_unary); return GLIO_E_ARG; }
    if (!pg_finite(xyz, 3)) { glio_set_error("glio_pgraph_add_gps: the position is not finite"); return GLIO_E_ARG; }
    if (!pg_var_ok(var, 3)) { glio_set_error("glio_pgraph_add_gps: a variance is not positive and finite"); return GLIO_E_ARG; }
    pg->gps_node.push_back(i);
    pg->gps_m.insert(pg->gps_m.end(), xyz, xyz + 3);
    for (int k = 0; k < 3; ++k) pg->gps_w.push_back(1.0 / sqrt(std::max(var[k], pg->o.gps_var_floor)));
    pg->factors_dirty = 1;
    return GLIO_OK;
}

static int pg_ready(glio_pgraph* pg, const char* who) {
    if (pg->N < 1) { glio_set_error("%s: the graph has no node", who); return GLIO_E_ARG; }
    if (!pg->have_prior && pg->gps_node.empty()) { glio_set_error("%s: neither a prior nor a GPS factor exists", who); return GLIO_E_ARG; }
    PG_CHECK(hipSetDevice(pg->device));
    int rc = pg_flush_nodes(pg);
    if (rc == GLIO_OK) rc = pg_flush_factors(pg);
    return rc;
}

int glio_pgraph_solve(glio_pgraph* pg, glio_pgraph_info* info) {
    GLIO_TRACE("glio_pgraph_solve");
    if (!pg) return GLIO_E_ARG;
    { const int rc = pg_ready(pg, "glio_pgraph_solve"); if (rc != GLIO_OK) return rc; }
    PgPlan P;
    { const int rc = pg_make_plan(pg, -1, &P); if (rc != GLIO_OK) return rc; }
    const int N = pg->N;
    PG_CHECK(hipMemsetAsync(pg->d_ctl, 0, sizeof(PgCtl), pg->stream));
    PG_CHECK(hipMemcpyAsync(pg->d_x0, pg->d_x, (size_t)N * 56, hipMemcpyDeviceToDevice, pg->stream));
    PG_CHECK(hipEventRecord(pg->ev_t[0], pg->stream));
    pg_enqueue_linearise(pg, 0, pg->o.max_iterations);
    PG_CHECK(hipEventRecord(pg->ev_t[1], pg->stream));
    // The first PG_AHEAD iterations are enqueued ahead and waited for once; Gauss-Newton on these graphs ends within them.  A solve that does not gets the
    // rest of its max_iterations enqueued ahead the same way, behind one more wait.
    for (int it = 0; it < pg->o.max_iterations; ++it) {
        pg_enqueue_linear_solve(pg, P, it == 0 ? &pg->ev_t[2] : nullptr);
        if (P.S > 1) hipLaunchKernelGGL(k_pg_backsub, dim3(P.S - 1), dim3(64), 0, pg->stream, P, pg->d_ctl);
        hipLaunchKernelGGL(k_pg_update, dim3((N + 255) / 256), dim3(256), 0, pg->stream, N, pg->d_x, pg->d_x, pg->d_delta, pg->d_ctl, nullptr, nullptr, nullptr);
        if (it == 0) PG_CHECK(hipEventRecord(pg->ev_t[4], pg->stream));
        pg_enqueue_linearise(pg, 1, pg->o.max_iterations);
        if (it + 1 == PG_AHEAD || it + 1 == pg->o.max_iterations) {
            PG_CHECK(hipEventRecord(pg->ev_t[5], pg->stream));
            PG_CHECK(hipMemcpyAsync(pg->h_ctl, pg->d_ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, pg->stream));
            PG_CHECK(hipEventRecord(pg->ev_done, pg->stream));
            PG_CHECK(hipEventSynchronize(pg->ev_done));
            if (pg->h_ctl->done || pg->h_ctl->pivot_fail) break;
        }
    }
    if (pg->o.max_iterations <= 0) {
        PG_CHECK(hipEventRecord(pg->ev_t[5], pg->stream));
        PG_CHECK(hipMemcpyAsync(pg->h_ctl, pg->d_ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, pg->stream));
        PG_CHECK(hipEventRecord(pg->ev_done, pg->stream));
        PG_CHECK(hipEventSynchronize(pg->ev_done));
    }
    PG_CHECK(hipGetLastError());
    const PgCtl& c = *pg->h_ctl;
    int reason = c.reason;
    if (c.pivot_fail) reason = GLIO_PGRAPH_NONPOSITIVE_PIVOT;
    if (reason == GLIO_PGRAPH_NONPOSITIVE_PIVOT) {
        PG_CHECK(hipMemcpyAsync(pg->d_x, pg->d_x0, (size_t)N * 56, hipMemcpyDeviceToDevice, pg->stream));
        PG_CHECK(hipStreamSynchronize(pg->stream));
    }
    if (info) {
        memset(info, 0, sizeof *info);
        info->initial_error = c.err0;
        info->final_error = reason == GLIO_PGRAPH_NONPOSITIVE_PIVOT ? c.err0 : c.err_cur;
        info->iterations = c.iterations; info->termination = reason;
        info->separators = P.S; info->segments = P.S - 1;
        (void)hipEventElapsedTime(&info->device_ms, pg->ev_t[0], pg->ev_t[5]);
        if (pg->o.max_iterations > 0) {
            (void)hipEventElapsedTime(&info->stage_ms[0], pg->ev_t[0], pg->ev_t[1]);
            (void)hipEventElapsedTime(&info->stage_ms[1], pg->ev_t[1], pg->ev_t[2]);
            (void)hipEventElapsedTime(&info->stage_ms[2], pg->ev_t[2], pg->ev_t[3]);
            (void)hipEventElapsedTime(&info->stage_ms[3], pg->ev_t[3], pg->ev_t[4]);
        }
    }
    return GLIO_OK;
}

void glio_pgraph_lm_opts_default(glio_pgraph_lm_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->initial_radius = TR_INITIAL_RADIUS; o->max_radius = TR_MAX_RADIUS; o->min_radius = TR_MIN_RADIUS; o->min_relative_decrease = TR_MIN_RELATIVE_DECREASE;
    o->min_diagonal = TR_MIN_DIAGONAL; o->max_diagonal = TR_MAX_DIAGONAL; o->max_trials = 0;      // ceres::Solver::Options (1.14), tr_math.h
}
int glio_pgraph_lm_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_pgraph_lm_opts), (int32_t)sizeof(glio_pgraph_lm_info)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

// the copy of the control block (and, for a damped solve, of the history) behind everything enqueued so far, and the wait for it
static int pg_wait_ctl(glio_pgraph* pg, int hist_rows) {
    PG_CHECK(hipEventRecord(pg->ev_t[5], pg->stream));
    PG_CHECK(hipMemcpyAsync(pg->h_ctl, pg->d_ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, pg->stream));
    if (hist_rows > 0) PG_CHECK(hipMemcpyAsync(pg->lm_hist_in.data(), pg->d_hist, (size_t)hist_rows * 32, hipMemcpyDeviceToHost, pg->stream));
    PG_CHECK(hipEventRecord(pg->ev_done, pg->stream));
    PG_CHECK(hipEventSynchronize(pg->ev_done));
    return GLIO_OK;
}

int glio_pgraph_solve_damped(glio_pgraph* pg, const glio_pgraph_lm_opts* lm_opts, glio_pgraph_info* info, glio_pgraph_lm_info* lm_info) {
    GLIO_TRACE("glio_pgraph_solve_damped");
    if (!pg) return GLIO_E_ARG;
    glio_pgraph_lm_opts lo;
    if (lm_opts) lo = *lm_opts; else glio_pgraph_lm_opts_default(&lo);
    const double pos[5] = {lo.initial_radius, lo.max_radius, lo.min_radius, lo.min_diagonal, lo.max_diagonal};
    if (!pg_var_ok(pos, 5) || lo.min_radius > lo.initial_radius || lo.initial_radius > lo.max_radius || lo.min_diagonal > lo.max_diagonal ||
        !(lo.min_relative_decrease >= 0.0) || !(lo.min_relative_decrease < 1.0) || lo.max_trials < 0) {
        glio_set_error("bad glio_pgraph_lm_opts (a radius or a diagonal bound that is not finite and positive, min_radius <= initial_radius <= max_radius or "
                       "min_diagonal <= max_diagonal violated, min_relative_decrease outside [0, 1), or max_trials %d < 0)", lo.max_trials);
        return GLIO_E_ARG;
    }
    { const int rc = pg_ready(pg, "glio_pgraph_solve_damped"); if (rc != GLIO_OK) return rc; }
    PgPlan P;
    { const int rc = pg_make_plan(pg, -1, &P); if (rc != GLIO_OK) return rc; }
    const int N = pg->N, L = (int)pg->lp_i.size(), max_trials = lo.max_trials > 0 ? lo.max_trials : pg->o.max_iterations;
    {                                           // each table by its own pointer: a call that failed half way is finished by the next one
        const size_t cap = (size_t)pg->o.max_nodes;
        if (!pg->d_xc) PG_CHECK(hipMalloc((void**)&pg->d_xc, cap * 56));
        if (!pg->d_dr) PG_CHECK(hipMalloc((void**)&pg->d_dr, cap * 48));
        if (!pg->d_gf) PG_CHECK(hipMalloc((void**)&pg->d_gf, cap * 48));
        if (!pg->d_nm) PG_CHECK(hipMalloc((void**)&pg->d_nm, cap * 8));
    }
    if ((size_t)max_trials > pg->hist_cap) {
        if (pg->d_hist) { hipFree(pg->d_hist); pg->d_hist = nullptr; pg->hist_cap = 0; }
        PG_CHECK(hipMalloc((void**)&pg->d_hist, (size_t)max_trials * 32));
        pg->hist_cap = (size_t)max_trials;
    }
    pg->lm_hist_in.assign((size_t)4 * std::max(max_trials, 0), 0.0);
    P.dr = pg->d_dr;
    PgLm o;
    o.max_radius = lo.max_radius; o.min_radius = lo.min_radius; o.min_relative_decrease = lo.min_relative_decrease;
    o.min_diagonal = lo.min_diagonal; o.max_diagonal = lo.max_diagonal; o.max_trials = max_trials;
    const PgLin lin = pg_lin(pg);
    PG_CHECK(hipMemsetAsync(pg->d_ctl, 0, sizeof(PgCtl), pg->stream));
    hipLaunchKernelGGL(k_pg_lm_begin, dim3(1), dim3(1), 0, pg->stream, pg->d_ctl, lo.initial_radius);
    PG_CHECK(hipEventRecord(pg->ev_t[0], pg->stream));
    pg_enqueue_linearise(pg, 0, max_trials);
    PG_CHECK(hipEventRecord(pg->ev_t[1], pg->stream));
    // The trials are enqueued ahead as glio_pgraph_solve's iterations are.  A trial: the linearisation at x (skipped while the tables still hold it), the
    // damping, the damped linear solve, the candidate with the model decrease, the linearisation at the candidate (its error; and the next trial's tables when
    // the candidate is accepted), the decision, the copy of an accepted candidate.  x itself is written by that copy alone.
    bool waited = false;
    for (int it = 0; it < max_trials; ++it) {
        pg_enqueue_lin_at(pg, pg->d_x, 1);
        hipLaunchKernelGGL(k_pg_damping, dim3((N + 255) / 256), dim3(256), 0, pg->stream, N, P, lin, pg->d_ctl, pg->d_dr, pg->d_gf, lo.min_diagonal, lo.max_diagonal);
        pg_enqueue_linear_solve(pg, P, it == 0 ? &pg->ev_t[2] : nullptr);
        if (P.S > 1) hipLaunchKernelGGL(k_pg_backsub, dim3(P.S - 1), dim3(64), 0, pg->stream, P, pg->d_ctl);
        hipLaunchKernelGGL(k_pg_update, dim3((N + 255) / 256), dim3(256), 0, pg->stream, N, pg->d_x, pg->d_xc, pg->d_delta, pg->d_ctl, pg->d_dr, pg->d_gf, pg->d_nm);
        if (it == 0) PG_CHECK(hipEventRecord(pg->ev_t[4], pg->stream));
        pg_enqueue_lin_at(pg, pg->d_xc, 0);
        hipLaunchKernelGGL(k_pg_lm_decide, dim3(1), dim3(1024), 0, pg->stream, N, L, pg->d_nerr, pg->d_lp_out, pg->d_nm, pg->d_ctl, pg->d_hist, o,
                           pg->o.relative_error_tol, pg->o.absolute_error_tol);
        hipLaunchKernelGGL(k_pg_lm_commit, dim3((7 * N + 255) / 256), dim3(256), 0, pg->stream, N, pg->d_x, pg->d_xc, pg->d_ctl, it + 1);
        if (it + 1 == PG_AHEAD || it + 1 == max_trials) {
            { const int rc = pg_wait_ctl(pg, it + 1); if (rc != GLIO_OK) return rc; }
            waited = true;
            if (pg->h_ctl->done) break;
        }
    }
    if (!waited) { const int rc = pg_wait_ctl(pg, 0); if (rc != GLIO_OK) return rc; }
    PG_CHECK(hipGetLastError());
    const PgCtl& c = *pg->h_ctl;
    pg->lm_hist_in.resize((size_t)4 * c.iterations);
    pg->lm_hist.swap(pg->lm_hist_in);            // only now: a solve that returned early leaves the last history in place
    if (info) {
        memset(info, 0, sizeof *info);
        info->initial_error = c.err0; info->final_error = c.err_cur;
        info->iterations = c.iterations; info->termination = c.reason;
        info->separators = P.S; info->segments = P.S - 1;
        (void)hipEventElapsedTime(&info->device_ms, pg->ev_t[0], pg->ev_t[5]);
        if (max_trials > 0) {
            (void)hipEventElapsedTime(&info->stage_ms[0], pg->ev_t[0], pg->ev_t[1]);
            (void)hipEventElapsedTime(&info->stage_ms[1], pg->ev_t[1], pg->ev_t[2]);
            (void)hipEventElapsedTime(&info->stage_ms[2], pg->ev_t[2], pg->ev_t[3]);
            (void)hipEventElapsedTime(&info->stage_ms[3], pg->ev_t[3], pg->ev_t[4]);
        }
    }
    if (lm_info) {
        lm_info->final_radius = c.radius;
        lm_info->accepted = c.accepted; lm_info->rejected = c.rejected; lm_info->invalid = c.invalid; lm_info->trials = c.iterations;
    }
    return GLIO_OK;
}

int glio_pgraph_lm_history(glio_pgraph* pg, int first, int n, double* out) {
    if (!pg) return GLIO_E_ARG;
    const long long rows = (long long)(pg->lm_hist.size() / 4);
    if (first < 0 || n < 0 || (long long)first + n > rows || (n > 0 && !out)) { glio_set_error("glio_pgraph_lm_history: rows [%d, %d + %d) of %lld", first, first, n, rows); return GLIO_E_ARG; }
    if (n > 0) memcpy(out, pg->lm_hist.data() + (size_t)4 * first, (size_t)n * 32);
    return GLIO_OK;
}

int glio_pgraph_size(glio_pgraph* pg, int* n_nodes) {
    if (!pg || !n_nodes) return GLIO_E_ARG;
    *n_nodes = pg->N;
    return GLIO_OK;
}

int glio_pgraph_read_poses(glio_pgraph* pg, int first, int n, double* out) {
    if (!pg || first < 0 || n < 0 || (long long)first + n > (long long)pg->N || (n > 0 && !out)) { glio_set_error("glio_pgraph_read_poses: bad range"); return GLIO_E_ARG; }
    if (n == 0) return GLIO_OK;
    PG_CHECK(hipSetDevice(pg->device));
    { const int rc = pg_flush_nodes(pg); if (rc != GLIO_OK) return rc; }
    PG_CHECK(hipMemcpyAsync(out, pg->d_x + (size_t)7 * first, (size_t)n * 56, hipMemcpyDeviceToHost, pg->stream));
    PG_CHECK(hipStreamSynchronize(pg->stream));
    return GLIO_OK;
}

int glio_pgraph_error(glio_pgraph* pg, double* error) {
    if (!pg || !error) return GLIO_E_ARG;
    { const int rc = pg_ready(pg, "glio_pgraph_error"); if (rc != GLIO_OK) return rc; }
    PG_CHECK(hipMemsetAsync(pg->d_ctl, 0, sizeof(PgCtl), pg->stream));
    pg_enqueue_linearise(pg, -1, 0);
    PG_CHECK(hipMemcpyAsync(pg->h_ctl, pg->d_ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, pg->stream));
    PG_CHECK(hipStreamSynchronize(pg->stream));
    PG_CHECK(hipGetLastError());
    *error = pg->h_ctl->err;
    return GLIO_OK;
}

int glio_pgraph_marginal_covariance(glio_pgraph* pg, int node, double* out) {
    GLIO_TRACE("glio_pgraph_marginal_covariance");
    if (!pg || !out) return GLIO_E_ARG;
    if (node < 0 || node >= pg->N) { glio_set_error("glio_pgraph_marginal_covariance: node %d of %d", node, pg->N); return GLIO_E_ARG; }
    { const int rc = pg_ready(pg, "glio_pgraph_marginal_covariance"); if (rc != GLIO_OK) return rc; }
    PgPlan P;
    { const int rc = pg_make_plan(pg, node, &P); if (rc != GLIO_OK) return rc; }
    PG_CHECK(hipMemsetAsync(pg->d_ctl, 0, sizeof(PgCtl), pg->stream));
    pg_enqueue_linearise(pg, -1, 0);
    pg_enqueue_linear_solve(pg, P, nullptr);
    PG_CHECK(hipMemcpyAsync(pg->h_ctl, pg->d_ctl, sizeof(PgCtl), hipMemcpyDeviceToHost, pg->stream));
    PG_CHECK(hipStreamSynchronize(pg->stream));
    PG_CHECK(hipGetLastError());
    if (pg->h_ctl->pivot_fail) { glio_set_error("glio_pgraph_marginal_covariance: a non-positive pivot"); return GLIO_E_NUMERIC; }
    memcpy(out, pg->h_ctl->cov, 36 * 8);
    return GLIO_OK;
}

int glio_pgraph_cov_struct_sizes(int32_t* out, int n) {
    if (out && n > 0) out[0] = (int32_t)sizeof(glio_pgraph_cov_info);
    return 1;
}

// One factorisation with the plan of a solve and no right-hand side, the selected inversion, one wait.  to_host: diag (and next, unless null) go through pinned
// memory into the caller's arrays; otherwise the result stays on the device.
static int pg_covariance_all(glio_pgraph* pg, const char* who, bool to_host, double* diag, double* next, glio_pgraph_cov_info* info) {
    { const int rc = pg_ready(pg, who); if (rc != GLIO_OK) return rc; }
    PgPlan P;
    { const int rc = pg_make_plan(pg, -1, &P, false); if (rc != GLIO_OK) return rc; }
    const int N = pg->N;
    if ((size_t)N > pg->cov_cap) {              // everything that scales with the nodes, for twice as many as asked now (at most max_nodes)
        void* old[] = {pg->d_dinv, pg->d_segpiv, pg->d_segbad, pg->d_cov};
        for (void* q : old) if (q) (void)hipFree(q);
        if (pg->h_cov) (void)hipHostFree(pg->h_cov);
        pg->d_dinv = pg->d_segpiv = pg->d_cov = pg->h_cov = nullptr; pg->d_segbad = nullptr; pg->cov_cap = 0;
        const size_t cap = std::min<size_t>((size_t)pg->o.max_nodes, std::max<size_t>(2 * (size_t)N, 64));
        PG_CHECK(hipMalloc((void**)&pg->d_dinv, cap * 288)); PG_CHECK(hipMalloc((void**)&pg->d_segpiv, cap * 16)); PG_CHECK(hipMalloc((void**)&pg->d_segbad, cap * 4));
        PG_CHECK(hipMalloc((void**)&pg->d_cov, cap * 576)); PG_CHECK(hipHostMalloc((void**)&pg->h_cov, cap * 576));
        pg->cov_cap = cap;
    }
    const size_t zneed = (size_t)P.n * 12 + (size_t)6 * P.nW * P.n;
    if (zneed > pg->zsys_cap) {
        if (pg->d_zsys) { hipFree(pg->d_zsys); pg->d_zsys = nullptr; pg->zsys_cap = 0; }
        PG_CHECK(hipMalloc((void**)&pg->d_zsys, (zneed + zneed / 2) * 8));
        pg->zsys_cap = zneed + zneed / 2;
    }
    PgPlan Zp = P;
    Zp.band = pg->d_zsys; Zp.wide = pg->d_zsys + (size_t)P.n * 12;
    const PgCovSeg cv = {pg->d_dinv, pg->d_segpiv, pg->d_segbad};
    double* d_diag = pg->d_cov;
    double* d_next = pg->d_cov + (size_t)36 * N;
    PG_CHECK(hipMemsetAsync(pg->d_ctl, 0, sizeof(PgCtl), pg->stream));
    PG_CHECK(hipMemsetAsync(pg->d_segbad, 0xff, (size_t)std::max(P.S - 1, 1) * 4, pg->stream));
    PG_CHECK(hipMemsetAsync(P.ldiag, 0, (size_t)P.n * 8, pg->stream));
    PG_CHECK(hipEventRecord(pg->ev_t[0], pg->stream));
    pg_enqueue_lin_at(pg, pg->d_x, 0);
    PG_CHECK(hipEventRecord(pg->ev_t[1], pg->stream));
    pg_enqueue_linear_solve(pg, P, nullptr, &cv);
    PG_CHECK(hipEventRecord(pg->ev_t[2], pg->stream));
    hipLaunchKernelGGL(k_pg_sep_inverse, dim3(1), dim3(PG_SEP_THREADS), 0, pg->stream, P, Zp, cv, pg->d_ctl);
    PG_CHECK(hipEventRecord(pg->ev_t[3], pg->stream));
    hipLaunchKernelGGL(k_pg_cov_sweep, dim3(P.S), dim3(64), 0, pg->stream, P, Zp, cv, d_diag, d_next, pg->d_ctl);
    PG_CHECK(hipEventRecord(pg->ev_t[4], pg->stream));
    const size_t words = (size_t)36 * N + (next ? (size_t)36 * (N - 1) : 0);
    if (to_host) PG_CHECK(hipMemcpyAsync(pg->h_cov, pg->d_cov, words * 8, hipMemcpyDeviceToHost, pg->stream));
    { const int rc = pg_wait_ctl(pg, 0); if (rc != GLIO_OK) return rc; }
    PG_CHECK(hipGetLastError());
    const PgCtl& c = *pg->h_ctl;
    for (int k = 0; k < 5; ++k) (void)hipEventElapsedTime(&pg->cov_ms[k], pg->ev_t[k], pg->ev_t[k + 1]);
    (void)hipEventElapsedTime(&pg->cov_ms[5], pg->ev_t[0], pg->ev_t[5]);
    pg->cov_timed = 1;
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_nodes = N; info->separators = P.S; info->full_row_separators = P.nW; info->segment_nodes = pg_segment_nodes(pg);
        info->bad_node = c.pivot_fail ? c.bad_node : -1;
        if (!c.pivot_fail) { info->min_pivot = c.min_pivot; info->max_pivot = c.max_pivot; }
    }
    if (c.pivot_fail) { glio_set_error("%s: the pivot of node %d is not positive and finite", who, c.bad_node); return GLIO_E_NUMERIC; }
    if (to_host) {
        memcpy(diag, pg->h_cov, (size_t)N * 288);
        if (next && N > 1) memcpy(next, pg->h_cov + (size_t)36 * N, (size_t)(N - 1) * 288);
    }
    return GLIO_OK;
}

int glio_pgraph_covariance_all(glio_pgraph* pg, double* diag, double* next, glio_pgraph_cov_info* info) {
    GLIO_TRACE("glio_pgraph_covariance_all");
    if (!pg || !diag) { glio_set_error("glio_pgraph_covariance_all: null argument"); return GLIO_E_ARG; }
    return pg_covariance_all(pg, "glio_pgraph_covariance_all", true, diag, next, info);
}

int glio_pgraph_covariance_all_dev(glio_pgraph* pg, const double** diag_dev, const double** next_dev, int* n_nodes) {
    GLIO_TRACE("glio_pgraph_covariance_all_dev");
    if (!pg || !diag_dev) { glio_set_error("glio_pgraph_covariance_all_dev: null argument"); return GLIO_E_ARG; }
    const int rc = pg_covariance_all(pg, "glio_pgraph_covariance_all_dev", false, nullptr, nullptr, nullptr);
    if (rc != GLIO_OK) return rc;
    *diag_dev = pg->d_cov;
    if (next_dev) *next_dev = pg->d_cov + (size_t)36 * pg->N;
    if (n_nodes) *n_nodes = pg->N;
    return GLIO_OK;
}

int glio_pgraph_covariance_all_last_device_ms(glio_pgraph* pg, float* ms) {
    if (!pg || !ms) return GLIO_E_ARG;
    if (!pg->cov_timed) { glio_set_error("glio_pgraph_covariance_all_last_device_ms: no call yet"); return GLIO_E_STATE; }
    *ms = pg->cov_ms[5];
    return GLIO_OK;
}

int glio_pgraph_covariance_all_last_stage_ms(glio_pgraph* pg, float* ms5) {
    if (!pg || !ms5) return GLIO_E_ARG;
    if (!pg->cov_timed) { glio_set_error("glio_pgraph_covariance_all_last_stage_ms: no call yet"); return GLIO_E_STATE; }
    memcpy(ms5, pg->cov_ms, 5 * sizeof(float));
    return GLIO_OK;
}

int glio_pgraph_poses_dev(glio_pgraph* pg, const double** poses_dev, int* n_nodes) {
    if (!pg || !poses_dev) return GLIO_E_ARG;
    PG_CHECK(hipSetDevice(pg->device));
    { const int rc = pg_flush_nodes(pg); if (rc != GLIO_OK) return rc; }
    *poses_dev = pg->d_x;
    if (n_nodes) *n_nodes = pg->N;
    return GLIO_OK;
}

}  // extern "C"

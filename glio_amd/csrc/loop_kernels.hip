// loop_kernels.hip -- loop closure on the device: detectLoopClosure's two submaps from the resident keyframe clouds of a glio_bassoc and
// performLoopClosure's pcl::IterativeClosestPoint (reference GLIO/src/Estimator.cpp:5101-5273).  The rules are stated in include/glio_hip.h
// (glio_loop_*); they restate PCL 1.8.1 and are UNPINNED (PCL is not part of the reference tree).
//
// Submaps: the local map's VoxelGrid (localmap_kernels.hip, glio_vg_*: float sums in concatenation order, PCL's output order) over the listed
// keyframes -- no second VoxelGrid.
//
// Registration.  The target is fixed for a whole alignment: its points are binned ONCE into a uniform grid over their bounding box (cell 2.5 leaves,
// grown until the box has at most 2^21 cells; counting sort: count, scan, scatter).  A query walks the shells of cells around its own cell; after shell r
// every point of the cube of (2r+1)^3 cells has been seen, so the best distance is EXACT as soon as it is no larger than the distance from the query to
// the nearest face of that cube behind which unsearched cells lie (less a margin for the float rounding of the binning).  The answer is the minimum of
// (d2, index) in that order, so ties go to the lowest target index whatever the order of a cell's points.  A query that is not certified after
// LP_MAX_SHELL shells (far from the target: the first rounds of a bad initial guess, the isolated points of the tests) is appended to a list and answered
// by a brute-force scan of the whole target through LDS tiles, one wavefront per query.
// A round is six launches (search, fallback, two reductions, the solve, the transform).  The convergence test runs on the device (k_lp_solve, one
// workgroup); every kernel of a later round returns at once when it finds the `done` word set, so all max_iterations rounds are enqueued ahead and no
// round costs a host round trip.  glio_loop_align then blocks on ONE event behind the copy of the result into pinned memory: the loop thread of the
// reference runs at 1 Hz, a spinning core would be taken from the keyframe cycle for nothing.
// Reductions (count, means, Sigma, mse, fitness): fp64, wavefront butterfly, then the four wavefronts of the workgroup in order, then the per-workgroup
// partials in a fixed order by one workgroup -- bit-identical from run to run.  No float atomics anywhere; the integer atomics (cell counts, the fallback
// list) do not influence any result.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "glio_device.h"
#include "cloud_device.h"

// d2 = dx*dx + dy*dy + dz*dz and T*p must round like scalar float code (and the numpy restatement): no FMA contraction in this file
#pragma clang fp contract(off)

#define LP_MAX_CELLS (1 << 21)
#define LP_MAX_SHELL 3
#define LP_TILE 2048            /* target points per LDS tile of the brute-force scan (32 KB) */
#define LP_MAX_ITER 1000

struct LoopGrid { float ox, oy, oz, cell, inv_cell; int nx, ny, nz, ncell; };
struct LoopState {
    LoopGrid g;
    double prev_mse, mse, sum_d2;
    double mu_s[3], mu_t[3];
    float T[16], Tfinal[16];
    int done, converged, state, iterations, n_corr, rank_def;
    unsigned apply_tag;             // launch sequence number + 1 of the round whose transform k_lp_apply has to apply
    int n_fb, last_fb, fit_fb;      // fallback queries: running counter of the search in flight, of the last round, of the fitness search
    int min_corr, max_iter;
    double max_d2, tr_eps, fit_eps, abs_eps;
};

struct glio_loop {
    GlioBassocView v;
    glio_loop_opts o;
    hipStream_t stream;
    hipEvent_t ev_dep, ev_done, ev_t0, ev_t1;
    LocalMap* vg;
    float4* d_pts[2];               // the submaps: source, target
    float4* d_cur;                  // the source moved by the rounds so far
    float4* d_tsorted;              // the target in cell order, w = index in the target
    int* d_cell_start; int* d_cell_cnt; int* d_tcell;
    int* d_bbox;
    int* d_idx; float* d_d2; int* d_fb_list; int* d_fb_hist;
    double* d_partA; double* d_partB;
    LoopState* d_st;
    glio_loop_result* d_res; glio_loop_result* h_res;
    glio_loop_step_result* d_step; glio_loop_step_result* h_step;
    const float4** h_src; int* h_nsrc;
    int n[2];
    int tgt_dirty, cur_valid, have_ms, hist_n;
    unsigned seq;
};

// ---- the target's grid
__global__ void k_lp_bbox_init(int* bbox) { const int i = threadIdx.x; if (i < 3) bbox[i] = 0x7fffffff; else if (i < 6) bbox[i] = (int)0x80000000; }
__global__ __launch_bounds__(256) void k_lp_bbox(const float4* __restrict__ pts, const int n, int* bbox) {
    __shared__ int s_box[256 / 64 * 6];
    CloudBox b;
    b.init();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        const float c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) if (c[a] == c[a] && fabsf(c[a]) <= FLT_MAX) b.add(a, f2ord(c[a]));      // (finite coordinates only, per axis)
    }
    b.commit<256 / 64>(s_box, bbox);
}
__global__ void k_lp_grid_params(const int* __restrict__ bbox, const float cell0, LoopState* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = bbox[a] == 0x7fffffff ? 0.f : ord2f(bbox[a]);          // (no finite coordinate on this axis: one cell)
        hi[a] = bbox[3 + a] == (int)0x80000000 ? 0.f : ord2f(bbox[3 + a]);
    }
    LoopGrid g;
    g.ox = lo[0]; g.oy = lo[1]; g.oz = lo[2];
    float cell = cell0;
    for (int it = 0; it < 400; ++it) {
        const double inv = 1.0 / (double)cell;
        const double cells = (floor(((double)hi[0] - lo[0]) * inv) + 2.0) * (floor(((double)hi[1] - lo[1]) * inv) + 2.0) * (floor(((double)hi[2] - lo[2]) * inv) + 2.0);
        if (cells <= (double)LP_MAX_CELLS) break;
        cell *= 1.26f;
    }
    g.cell = cell; g.inv_cell = 1.0f / cell;
    // the dimensions by the very expression that bins a point (lp_cell_of), so that the largest coordinate falls into the last cell
    int d[3];
    for (int a = 0; a < 3; ++a) {
        const float f = floorf((hi[a] - lo[a]) * g.inv_cell);
        d[a] = f >= 0.f && f < 2097152.f ? (int)f + 1 : 1;
    }
    if ((double)d[0] * d[1] * d[2] > (double)LP_MAX_CELLS) { d[0] = d[1] = d[2] = 1; }      // (cannot happen after the loop above; one cell is always right)
    g.nx = d[0]; g.ny = d[1]; g.nz = d[2]; g.ncell = d[0] * d[1] * d[2];
    st->g = g;
}
// cell coordinates of a point, clamped into the grid (a query outside the box gets the nearest cell; NaN goes to cell 0)
__device__ __forceinline__ void lp_cell_of(const LoopGrid& g, const float4 p, int& cx, int& cy, int& cz) {
    cx = (int)fminf(fmaxf(floorf((p.x - g.ox) * g.inv_cell), 0.f), (float)(g.nx - 1));
    cy = (int)fminf(fmaxf(floorf((p.y - g.oy) * g.inv_cell), 0.f), (float)(g.ny - 1));
    cz = (int)fminf(fmaxf(floorf((p.z - g.oz) * g.inv_cell), 0.f), (float)(g.nz - 1));
}
__global__ void k_lp_cell_count(const float4* __restrict__ tgt, const int n, const LoopState* __restrict__ st, int* __restrict__ tcell, int* cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LoopGrid g = st->g;
    int cx, cy, cz;
    lp_cell_of(g, tgt[i], cx, cy, cz);
    const int c = cx + g.nx * (cy + g.ny * cz);
    tcell[i] = c;
    atomicAdd(cnt + c, 1);
}
// exclusive scan of the cell counts by one workgroup (a contiguous chunk per thread; once per target); the counts are zeroed for the scatter's fill
__global__ __launch_bounds__(1024) void k_lp_cell_scan(const LoopState* __restrict__ st, int* __restrict__ cnt, int* __restrict__ start) {
    __shared__ int part[1024];
    const int ncell = st->g.ncell, tid = threadIdx.x, chunk = (ncell + 1023) / 1024, c0 = min(ncell, tid * chunk), c1 = min(ncell, c0 + chunk);
    int s = 0;
    for (int c = c0; c < c1; ++c) s += cnt[c];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int k = 0; k < 1024; ++k) { const int x = part[k]; part[k] = t; t += x; } start[ncell] = t; }
    __syncthreads();
    int run = part[tid];
    for (int c = c0; c < c1; ++c) { const int x = cnt[c]; start[c] = run; cnt[c] = 0; run += x; }
}
__global__ void k_lp_cell_scatter(const float4* __restrict__ tgt, const int n, const int* __restrict__ tcell, const int* __restrict__ start, int* fill,
                                  float4* __restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = tcell[i];
    const int pos = start[c] + atomicAdd(fill + c, 1);          // (pos < n: the counts of k_lp_cell_count)
    const float4 p = tgt[i];
    sorted[pos] = make_float4(p.x, p.y, p.z, __int_as_float(i));
}

// ---- 1-NN search
__device__ __forceinline__ void lp_scan_range(const float4* __restrict__ sorted, const int a, const int b, const float4 q, float& bd, int& bi) {
    for (int k = a; k < b; ++k) {
        const float4 t = sorted[k];
        const float dx = q.x - t.x, dy = q.y - t.y, dz = q.z - t.z;
        const float d2 = dx * dx + dy * dy + dz * dz;
        const int ti = __float_as_int(t.w);
        if (d2 < bd || (d2 == bd && ti < bi)) { bd = d2; bi = ti; }
    }
}
__global__ __launch_bounds__(128) void k_lp_search(const float4* __restrict__ cur, const int n, const float4* __restrict__ sorted, const int* __restrict__ start,
                                                   LoopState* st, const int gated, int* __restrict__ idx, float* __restrict__ d2o, int* __restrict__ fb_list) {
    if (gated && st->done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LoopGrid g = st->g;
    const float4 q = cur[i];
    int cx, cy, cz;
    lp_cell_of(g, q, cx, cy, cz);
    float bd = INFINITY; int bi = 0x7fffffff;
    // (the faces are origin + k * cell, the binning is floor((p - origin) * (1 / cell)): the margin covers the rounding of both, of the coordinates and of d2)
    const float margin = (0.01f + 1e-6f * (float)(g.nx + g.ny + g.nz)) * g.cell + 1e-5f * (fabsf(q.x) + fabsf(q.y) + fabsf(q.z) + fabsf(g.ox) + fabsf(g.oy) + fabsf(g.oz));
    bool certified = false;
    for (int r = 0; r <= LP_MAX_SHELL && !certified; ++r) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1);
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.nz) continue;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.ny) continue;
                const int row = g.nx * (y + g.ny * z);
                if (dz == -r || dz == r || dy == -r || dy == r) {          // a face row of the shell: cells x0..x1 are consecutive in memory
                    lp_scan_range(sorted, start[row + x0], start[row + x1 + 1], q, bd, bi);
                } else {                                                  // an inner row: only its two end cells are new
                    if (cx - r >= 0) lp_scan_range(sorted, start[row + cx - r], start[row + cx - r + 1], q, bd, bi);
                    if (cx + r < g.nx) lp_scan_range(sorted, start[row + cx + r], start[row + cx + r + 1], q, bd, bi);
                }
            }
        }
        // distance to the nearest face of the cube [c - r, c + r] that has unsearched cells behind it
        float dout = INFINITY;
        if (cx - r > 0) dout = fminf(dout, q.x - (g.ox + (float)(cx - r) * g.cell));
        if (cx + r < g.nx - 1) dout = fminf(dout, (g.ox + (float)(cx + r + 1) * g.cell) - q.x);
        if (cy - r > 0) dout = fminf(dout, q.y - (g.oy + (float)(cy - r) * g.cell));
        if (cy + r < g.ny - 1) dout = fminf(dout, (g.oy + (float)(cy + r + 1) * g.cell) - q.y);
        if (cz - r > 0) dout = fminf(dout, q.z - (g.oz + (float)(cz - r) * g.cell));
        if (cz + r < g.nz - 1) dout = fminf(dout, (g.oz + (float)(cz + r + 1) * g.cell) - q.z);
        if (dout == INFINITY) certified = bi != 0x7fffffff;                // the cube covers the whole grid
        else { const float ds = dout - margin; certified = ds > 0.f && bd <= ds * ds; }
    }
    if (!certified) { fb_list[atomicAdd(&st->n_fb, 1)] = i; return; }      // (every query is appended at most once: < n entries)
    d2o[i] = bd;
    idx[i] = (double)bd <= st->max_d2 ? bi : -1;
}
// the uncertified queries against the WHOLE target: one wavefront per query, the target through LDS tiles shared by the workgroup's four queries
__global__ __launch_bounds__(256) void k_lp_fallback(const float4* __restrict__ cur, const float4* __restrict__ tgt, const int nt, const LoopState* __restrict__ st,
                                                     const int gated, const int* __restrict__ fb_list, int* __restrict__ idx, float* __restrict__ d2o) {
    __shared__ float4 tile[LP_TILE];
    if (gated && st->done) return;
    const int nq = st->n_fb;
    if ((int)blockIdx.x * 4 >= nq) return;                                 // (uniform over the workgroup)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, qi = blockIdx.x * 4 + w;
    const bool live = qi < nq;
    const int i = live ? fb_list[qi] : 0;
    const float4 q = live ? cur[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float bd = INFINITY; int bi = 0x7fffffff;
    for (int t0 = 0; t0 < nt; t0 += LP_TILE) {
        const int m = min(LP_TILE, nt - t0);
        for (int k = threadIdx.x; k < m; k += 256) tile[k] = tgt[t0 + k];
        __syncthreads();
        if (live) for (int k = lane; k < m; k += 64) {
            const float4 t = tile[k];
            const float dx = q.x - t.x, dy = q.y - t.y, dz = q.z - t.z;
            const float d2 = dx * dx + dy * dy + dz * dz;
            if (d2 < bd) { bd = d2; bi = t0 + k; }                         // (ascending index per lane: the first minimum is the lowest index)
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float od = __shfl_xor(bd, off, 64); const int oi = __shfl_xor(bi, off, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (live && lane == 0) {
        if (bi == 0x7fffffff) { bd = INFINITY; bi = -1; }                   // (a NaN query: no distance compares)
        d2o[i] = bd;
        idx[i] = bi >= 0 && (double)bd <= st->max_d2 ? bi : -1;
    }
}

// ---- fixed-order fp64 reductions
template <int NV>
__device__ __forceinline__ void lp_block_reduce(double* v, double* lds /* [4][NV] */) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) for (int k = 0; k < NV; ++k) lds[w * NV + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ((lds[k] + lds[NV + k]) + lds[2 * NV + k]) + lds[3 * NV + k];
}
// the per-workgroup partials [nblk][NV] summed by the calling workgroup (256 threads), the same value in every thread
template <int NV>
__device__ __forceinline__ void lp_sum_partials(const double* __restrict__ part, const int nblk, double* v, double* lds) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] += part[(size_t)b * NV + k];
    }
    lp_block_reduce<NV>(v, lds);
}
// pass A: count, sum s, sum t, sum d2 of the kept pairs (all = 1: count and d2 of every point, for the fitness)
__global__ __launch_bounds__(256) void k_lp_reduce_a(const float4* __restrict__ cur, const int n, const float4* __restrict__ tgt, const int* __restrict__ idx,
                                                     const float* __restrict__ d2, LoopState* st, const int gated, const int all, double* __restrict__ part) {
    __shared__ double lds[4 * 8];
    if (gated && st->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        const int j = idx[i];
        if (all) { v[0] = 1.0; v[7] = (double)d2[i]; }
        else if (j >= 0) {
            const float4 s = cur[i], t = tgt[j];
            v[0] = 1.0; v[1] = s.x; v[2] = s.y; v[3] = s.z; v[4] = t.x; v[5] = t.y; v[6] = t.z; v[7] = (double)d2[i];
        }
    }
    lp_block_reduce<8>(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 8; ++k) part[(size_t)blockIdx.x * 8 + k] = v[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) { if (all) st->fit_fb = st->n_fb; else st->last_fb = st->n_fb; st->n_fb = 0; }      // (the search and its fallback are over)
}
// pass B: the means from pass A's partials (by every workgroup, the same bits), then Sigma's nine sums of (t - mu_t)(s - mu_s)^T
__global__ __launch_bounds__(256) void k_lp_reduce_b(const float4* __restrict__ cur, const int n, const float4* __restrict__ tgt, const int* __restrict__ idx,
                                                     LoopState* st, const double* __restrict__ partA, const int nblk, double* __restrict__ partB) {
    __shared__ double lds[4 * 9];
    if (st->done) return;
    double a[8];
    lp_sum_partials<8>(partA, nblk, a, lds);
    const double cnt = a[0] > 0.0 ? a[0] : 1.0;
    const double ms[3] = {a[1] / cnt, a[2] / cnt, a[3] / cnt}, mt[3] = {a[4] / cnt, a[5] / cnt, a[6] / cnt};
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
        const int j = idx[i];
        if (j >= 0) {
            const float4 s = cur[i], t = tgt[j];
            const double ds[3] = {(double)s.x - ms[0], (double)s.y - ms[1], (double)s.z - ms[2]}, dt[3] = {(double)t.x - mt[0], (double)t.y - mt[1], (double)t.z - mt[2]};
#pragma unroll
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) v[3 * r + c] = dt[r] * ds[c];
        }
    }
    lp_block_reduce<9>(v, lds);
    if (threadIdx.x == 0) for (int k = 0; k < 9; ++k) partB[(size_t)blockIdx.x * 9 + k] = v[k];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->n_corr = (int)a[0]; st->sum_d2 = a[7];
        for (int k = 0; k < 3; ++k) { st->mu_s[k] = ms[k]; st->mu_t[k] = mt[k]; }
    }
}

// ---- the rigid transform: eigenvectors of Sigma^T Sigma by cyclic Jacobi (fp64, one lane), U from Sigma V, R = U diag(1, 1, det U det V) V^T.
// Returns false when Sigma has rank < 2 (the pairs are collinear or one point: no rotation is determined).  The third column of U is u1 x u2, which is the
// column the sign rule leaves in either case (the rotation that completes u1 v1^T + u2 v2^T is unique), so a coplanar cloud (sigma3 = 0) needs no division.
__device__ bool lp_umeyama_R(const double S[9], double R[9]) {
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] = S[r] * S[c] + S[3 + r] * S[3 + c] + S[6 + r] * S[6 + c];      // S^T S
    for (int sweep = 0; sweep < 24; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]), dg = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (!(off > 1e-40 * dg)) break;
        for (int p = 0; p < 2; ++p) for (int q = p + 1; q < 3; ++q) {
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            for (int k = 0; k < 3; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq; }
            for (int k = 0; k < 3; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk; }
            for (int k = 0; k < 3; ++k) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq; }
        }
    }
    int o[3] = {0, 1, 2};
    const double lam[3] = {A[0][0], A[1][1], A[2][2]};
    if (lam[o[0]] < lam[o[1]]) { const int x = o[0]; o[0] = o[1]; o[1] = x; }
    if (lam[o[1]] < lam[o[2]]) { const int x = o[1]; o[1] = o[2]; o[2] = x; }
    if (lam[o[0]] < lam[o[1]]) { const int x = o[0]; o[0] = o[1]; o[1] = x; }
    const double s1 = sqrt(fmax(lam[o[0]], 0.0)), s2 = sqrt(fmax(lam[o[1]], 0.0));
    if (!(s1 > 0.0) || !(s2 > 1e-6 * s1) || !(s1 <= DBL_MAX)) return false;
    double v[3][3], u[3][3];                                   // v[i], u[i]: the i-th right / left singular vector
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) v[i][k] = V[k][o[i]];
    for (int i = 0; i < 2; ++i) for (int r = 0; r < 3; ++r) u[i][r] = S[3 * r] * v[i][0] + S[3 * r + 1] * v[i][1] + S[3 * r + 2] * v[i][2];
    double nn = sqrt(u[0][0] * u[0][0] + u[0][1] * u[0][1] + u[0][2] * u[0][2]);
    if (!(nn > 0.0)) return false;
    for (int r = 0; r < 3; ++r) u[0][r] /= nn;
    const double d01 = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2];
    for (int r = 0; r < 3; ++r) u[1][r] -= d01 * u[0][r];
    nn = sqrt(u[1][0] * u[1][0] + u[1][1] * u[1][1] + u[1][2] * u[1][2]);
    if (!(nn > 0.0)) return false;
    for (int r = 0; r < 3; ++r) u[1][r] /= nn;
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1]; u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2]; u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const double detV = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) - v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) + v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
    const double d = detV >= 0.0 ? 1.0 : -1.0;               // det U = +1 by construction
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = u[0][r] * v[0][c] + u[1][r] * v[1][c] + d * u[2][r] * v[2][c];
    for (int k = 0; k < 9; ++k) if (!(fabs(R[k]) <= 2.0)) return false;       // (non-finite input)
    return true;
}
__device__ __forceinline__ void lp_identity(float* T) { for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f; }
// steps 2, 3, 5 of the round and the bookkeeping of step 4 (the cloud itself is moved by k_lp_apply); one workgroup
__global__ __launch_bounds__(256) void k_lp_solve(LoopState* st, const double* __restrict__ partB, const int nblk, const unsigned seq, int* __restrict__ fb_hist, const int round) {
    __shared__ double lds[4 * 9];
    if (st->done) return;
    double S[9];
    lp_sum_partials<9>(partB, nblk, S, lds);
    if (threadIdx.x != 0) return;
    const int n = st->n_corr;
    if (fb_hist) fb_hist[round] = st->last_fb;          // (for glio_loop_read_fallbacks: written by the rounds that ran)
    st->rank_def = 0;
    lp_identity(st->T);
    st->mse = n > 0 ? st->sum_d2 / (double)n : 0.0;
    if (n < st->min_corr) { st->state = GLIO_LOOP_NO_CORRESPONDENCES; st->converged = 0; st->done = 1; return; }
    for (int k = 0; k < 9; ++k) S[k] /= (double)n;
    double R[9];
    if (!lp_umeyama_R(S, R)) { st->rank_def = 1; st->state = GLIO_LOOP_NOT_CONVERGED; st->converged = 0; st->done = 1; return; }
    float T[16];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[3 * r + c];
        T[4 * r + 3] = (float)(st->mu_t[r] - (R[3 * r] * st->mu_s[0] + R[3 * r + 1] * st->mu_s[1] + R[3 * r + 2] * st->mu_s[2]));
    }
    T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
    float F[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)
        F[4 * r + c] = ((T[4 * r] * st->Tfinal[c] + T[4 * r + 1] * st->Tfinal[4 + c]) + T[4 * r + 2] * st->Tfinal[8 + c]) + T[4 * r + 3] * st->Tfinal[12 + c];
    for (int k = 0; k < 16; ++k) { st->T[k] = T[k]; st->Tfinal[k] = F[k]; }
    st->iterations += 1;
    st->apply_tag = seq + 1u;
    // DefaultConvergenceCriteria, in its order
    const double cosa = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
    const double tsq = ((double)T[3] * (double)T[3] + (double)T[7] * (double)T[7]) + (double)T[11] * (double)T[11];
    const double mse = st->mse;
    int state = GLIO_LOOP_NOT_CONVERGED;
    if (st->iterations >= st->max_iter) state = GLIO_LOOP_ITERATIONS;
    else if (cosa >= 1.0 - st->tr_eps && tsq <= st->tr_eps) state = GLIO_LOOP_TRANSFORM;
    else if (fabs(mse - st->prev_mse) < st->abs_eps) state = GLIO_LOOP_ABS_MSE;
    else if (fabs(mse - st->prev_mse) / st->prev_mse < st->fit_eps) state = GLIO_LOOP_REL_MSE;
    st->state = state;
    if (state != GLIO_LOOP_NOT_CONVERGED) { st->converged = 1; st->done = 1; }
    else st->prev_mse = mse;
}
__global__ void k_lp_apply(float4* __restrict__ cur, const int n, const LoopState* __restrict__ st, const unsigned seq) {
    if (st->apply_tag != seq + 1u) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* T = st->T;
    const float4 p = cur[i];
    cur[i] = make_float4(((T[0] * p.x + T[1] * p.y) + T[2] * p.z) + T[3], ((T[4] * p.x + T[5] * p.y) + T[6] * p.z) + T[7],
                         ((T[8] * p.x + T[9] * p.y) + T[10] * p.z) + T[11], p.w);
}
__global__ void k_lp_begin(LoopState* st, const int keep_state, const glio_loop_opts o) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st->done = 0; st->n_fb = 0;
    st->min_corr = o.min_correspondences; st->max_iter = o.max_iterations;
    st->max_d2 = o.max_corr_dist * o.max_corr_dist; st->tr_eps = o.transformation_eps; st->fit_eps = o.fitness_eps; st->abs_eps = o.abs_mse_eps;
    if (keep_state) return;
    st->prev_mse = DBL_MAX; st->mse = 0.0; st->sum_d2 = 0.0;
    st->converged = 0; st->state = GLIO_LOOP_NOT_CONVERGED; st->iterations = 0; st->n_corr = 0; st->rank_def = 0; st->apply_tag = 0u; st->last_fb = 0; st->fit_fb = 0;
    lp_identity(st->T); lp_identity(st->Tfinal);
}
__global__ __launch_bounds__(256) void k_lp_finish(LoopState* st, const double* __restrict__ partA, const int nblk, const int n, glio_loop_result* res) {
    __shared__ double lds[4 * 8];
    double a[8];
    lp_sum_partials<8>(partA, nblk, a, lds);
    if (threadIdx.x != 0) return;
    glio_loop_result r;
    r.fitness = n > 0 ? a[7] / (double)n : 0.0;
    r.last_mse = st->mse;
    for (int k = 0; k < 16; ++k) r.transform[k] = st->Tfinal[k];
    r.converged = st->converged; r.state = st->state; r.iterations = st->iterations; r.last_n_corr = st->n_corr; r.rank_deficient = st->rank_def; r.reserved_ = 0;
    *res = r;
}
__global__ void k_lp_pack_step(const LoopState* __restrict__ st, glio_loop_step_result* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    glio_loop_step_result r;
    r.mse = st->mse;
    for (int k = 0; k < 16; ++k) r.transform[k] = st->T[k];
    r.n_corr = st->n_corr; r.state = st->state; r.n_fallback = st->last_fb; r.rank_deficient = st->rank_def;
    *out = r;
}

#define LP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

// the association's pending frame copies come first -- for the loop's stream, not for the host
static int lp_order_behind_assoc(glio_loop* lp) {
    LP_CHECK(hipEventRecord(lp->ev_dep, lp->v.stream));
    LP_CHECK(hipStreamWaitEvent(lp->stream, lp->ev_dep, 0));
    return GLIO_OK;
}
static int lp_build_grid(glio_loop* lp) {
    const int nt = lp->n[GLIO_LOOP_TARGET];
    const float4* tgt = lp->d_pts[GLIO_LOOP_TARGET];
    hipLaunchKernelGGL(k_lp_bbox_init, dim3(1), dim3(64), 0, lp->stream, lp->d_bbox);
    hipLaunchKernelGGL(k_lp_bbox, dim3(std::min(256, (nt + 255) / 256)), dim3(256), 0, lp->stream, tgt, nt, lp->d_bbox);
    hipLaunchKernelGGL(k_lp_grid_params, dim3(1), dim3(64), 0, lp->stream, lp->d_bbox, 2.5f * lp->o.leaf, lp->d_st);
    LP_CHECK(hipMemsetAsync(lp->d_cell_cnt, 0, (size_t)LP_MAX_CELLS * 4, lp->stream));
    hipLaunchKernelGGL(k_lp_cell_count, dim3((nt + 255) / 256), dim3(256), 0, lp->stream, tgt, nt, lp->d_st, lp->d_tcell, lp->d_cell_cnt);
    hipLaunchKernelGGL(k_lp_cell_scan, dim3(1), dim3(1024), 0, lp->stream, lp->d_st, lp->d_cell_cnt, lp->d_cell_start);
    hipLaunchKernelGGL(k_lp_cell_scatter, dim3((nt + 255) / 256), dim3(256), 0, lp->stream, tgt, nt, lp->d_tcell, lp->d_cell_start, lp->d_cell_cnt, lp->d_tsorted);
    LP_CHECK(hipGetLastError());
    lp->tgt_dirty = 0;
    return GLIO_OK;
}
static void lp_enqueue_search(glio_loop* lp, int gated) {
    const int ns = lp->n[GLIO_LOOP_SOURCE], nt = lp->n[GLIO_LOOP_TARGET];
    hipLaunchKernelGGL(k_lp_search, dim3((ns + 127) / 128), dim3(128), 0, lp->stream, lp->d_cur, ns, lp->d_tsorted, lp->d_cell_start, lp->d_st, gated, lp->d_idx, lp->d_d2, lp->d_fb_list);
    hipLaunchKernelGGL(k_lp_fallback, dim3((ns + 3) / 4), dim3(256), 0, lp->stream, lp->d_cur, lp->d_pts[GLIO_LOOP_TARGET], nt, lp->d_st, gated, lp->d_fb_list, lp->d_idx, lp->d_d2);
}
static void lp_enqueue_round(glio_loop* lp, int round) {
    const int ns = lp->n[GLIO_LOOP_SOURCE], nblk = (ns + 255) / 256;
    const float4* tgt = lp->d_pts[GLIO_LOOP_TARGET];
    const unsigned seq = lp->seq++;
    lp_enqueue_search(lp, 1);
    hipLaunchKernelGGL(k_lp_reduce_a, dim3(nblk), dim3(256), 0, lp->stream, lp->d_cur, ns, tgt, lp->d_idx, lp->d_d2, lp->d_st, 1, 0, lp->d_partA);
    hipLaunchKernelGGL(k_lp_reduce_b, dim3(nblk), dim3(256), 0, lp->stream, lp->d_cur, ns, tgt, lp->d_idx, lp->d_st, lp->d_partA, nblk, lp->d_partB);
    hipLaunchKernelGGL(k_lp_solve, dim3(1), dim3(256), 0, lp->stream, lp->d_st, lp->d_partB, nblk, seq, round >= 0 ? lp->d_fb_hist : nullptr, round);
    hipLaunchKernelGGL(k_lp_apply, dim3((ns + 255) / 256), dim3(256), 0, lp->stream, lp->d_cur, ns, lp->d_st, seq);
}
static int lp_reset_current(glio_loop* lp) {
    LP_CHECK(hipMemcpyAsync(lp->d_cur, lp->d_pts[GLIO_LOOP_SOURCE], (size_t)lp->n[GLIO_LOOP_SOURCE] * 16, hipMemcpyDeviceToDevice, lp->stream));
    hipLaunchKernelGGL(k_lp_begin, dim3(1), dim3(64), 0, lp->stream, lp->d_st, 0, lp->o);
    LP_CHECK(hipGetLastError());
    lp->cur_valid = 1;
    return GLIO_OK;
}
static int lp_ready(glio_loop* lp) {
    if (!lp) return GLIO_E_ARG;
    if (lp->n[0] < 1 || lp->n[1] < 1) { glio_set_error("glio_loop: %s submap not set", lp->n[0] < 1 ? "source" : "target"); return GLIO_E_STATE; }
    return GLIO_OK;
}
static void lp_submap_changed(glio_loop* lp, int which, int n) {
    lp->n[which] = n;
    if (which == GLIO_LOOP_TARGET) lp->tgt_dirty = 1; else lp->cur_valid = 0;
    lp->hist_n = 0;
}

extern "C" {

void glio_loop_opts_default(glio_loop_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_corr_dist = 30.0;            // setMaxCorrespondenceDistance(30), Estimator.cpp:5197
    o->transformation_eps = 1e-6;       // :5199
    o->fitness_eps = 1e-6;              // setEuclideanFitnessEpsilon, :5200
    o->abs_mse_eps = 1e-12;             // DefaultConvergenceCriteria::mse_threshold_absolute_
    o->leaf = 0.4f;                     // ds_filter_his_frames.setLeafSize(0.4 ...), :855
    o->max_iterations = 100;            // :5198
    o->min_correspondences = 3;         // Registration::min_number_correspondences_
    o->max_source_points = 65536;
    o->max_target_points = 262144;
    o->max_frames_per_submap = 64;      // (the reference: 6 and 2 lc_map_width + 1 = 51)
}
int glio_loop_struct_sizes(int32_t* out, int n) {
    const int32_t v[3] = {(int32_t)sizeof(glio_loop_opts), (int32_t)sizeof(glio_loop_result), (int32_t)sizeof(glio_loop_step_result)};
    for (int i = 0; i < n && i < 3; ++i) out[i] = v[i];
    return 3;
}

void glio_loop_destroy(glio_loop* lp) {
    if (!lp) return;
    hipSetDevice(lp->v.device);
    if (lp->stream) hipStreamSynchronize(lp->stream);
    if (lp->vg) glio_vg_destroy(lp->vg);
    void* p[] = {lp->d_pts[0], lp->d_pts[1], lp->d_cur, lp->d_tsorted, lp->d_cell_start, lp->d_cell_cnt, lp->d_tcell, lp->d_bbox, lp->d_idx, lp->d_d2, lp->d_fb_list,
                 lp->d_fb_hist, lp->d_partA, lp->d_partB, lp->d_st, lp->d_res, lp->d_step};
    for (void* q : p) if (q) hipFree(q);
    if (lp->h_res) hipHostFree(lp->h_res);
    if (lp->h_step) hipHostFree(lp->h_step);
    hipEvent_t ev[] = {lp->ev_dep, lp->ev_done, lp->ev_t0, lp->ev_t1};
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (lp->stream) hipStreamDestroy(lp->stream);
    delete[] lp->h_src; delete[] lp->h_nsrc;
    delete lp;
}

static int lp_create_body(glio_loop* lp) {
    const glio_loop_opts& o = lp->o;
    LP_CHECK(hipSetDevice(lp->v.device));
    LP_CHECK(hipStreamCreateWithFlags(&lp->stream, hipStreamNonBlocking));
    LP_CHECK(hipEventCreateWithFlags(&lp->ev_dep, hipEventDisableTiming));
    LP_CHECK(hipEventCreateWithFlags(&lp->ev_done, hipEventDisableTiming | hipEventBlockingSync));
    LP_CHECK(hipEventCreate(&lp->ev_t0)); LP_CHECK(hipEventCreate(&lp->ev_t1));
    const size_t ns = (size_t)o.max_source_points, nt = (size_t)o.max_target_points, nblk = (ns + 255) / 256;
    LP_CHECK(hipMalloc((void**)&lp->d_pts[0], ns * 16)); LP_CHECK(hipMalloc((void**)&lp->d_pts[1], nt * 16));
    LP_CHECK(hipMalloc((void**)&lp->d_cur, ns * 16)); LP_CHECK(hipMalloc((void**)&lp->d_tsorted, nt * 16));
    LP_CHECK(hipMalloc((void**)&lp->d_cell_start, ((size_t)LP_MAX_CELLS + 1) * 4)); LP_CHECK(hipMalloc((void**)&lp->d_cell_cnt, (size_t)LP_MAX_CELLS * 4));
    LP_CHECK(hipMalloc((void**)&lp->d_tcell, nt * 4)); LP_CHECK(hipMalloc((void**)&lp->d_bbox, 32));
    LP_CHECK(hipMalloc((void**)&lp->d_idx, ns * 4)); LP_CHECK(hipMalloc((void**)&lp->d_d2, ns * 4)); LP_CHECK(hipMalloc((void**)&lp->d_fb_list, ns * 4));
    LP_CHECK(hipMalloc((void**)&lp->d_fb_hist, ((size_t)o.max_iterations + 1) * 4));
    LP_CHECK(hipMalloc((void**)&lp->d_partA, nblk * 8 * 8)); LP_CHECK(hipMalloc((void**)&lp->d_partB, nblk * 9 * 8));
    LP_CHECK(hipMalloc((void**)&lp->d_st, sizeof(LoopState))); LP_CHECK(hipMemsetAsync(lp->d_st, 0, sizeof(LoopState), lp->stream));
    LP_CHECK(hipMalloc((void**)&lp->d_res, sizeof(glio_loop_result))); LP_CHECK(hipMalloc((void**)&lp->d_step, sizeof(glio_loop_step_result)));
    LP_CHECK(hipHostMalloc((void**)&lp->h_res, sizeof(glio_loop_result))); LP_CHECK(hipHostMalloc((void**)&lp->h_step, sizeof(glio_loop_step_result)));
    lp->h_src = new const float4*[o.max_frames_per_submap]; lp->h_nsrc = new int[o.max_frames_per_submap];
    const int max_vox = o.max_source_points > o.max_target_points ? o.max_source_points : o.max_target_points;
    { const int rv = glio_vg_create(o.max_frames_per_submap, lp->v.cap, o.leaf, max_vox, lp->stream, &lp->vg); if (rv != GLIO_OK) return rv; }
    LP_CHECK(hipStreamSynchronize(lp->stream));
    return GLIO_OK;
}
int glio_loop_create(glio_bassoc* b, const glio_loop_opts* opts, glio_loop** out) {
    if (!b || !opts || !out) return GLIO_E_ARG;
    const glio_loop_opts& o = *opts;
    if (!(o.leaf > 0.f) || !(o.max_corr_dist > 0.0) || !(o.max_corr_dist < 1e18) || o.max_iterations < 1 || o.max_iterations > LP_MAX_ITER || o.min_correspondences < 1 ||
        o.max_source_points < 1 || o.max_source_points > (1 << 24) || o.max_target_points < 1 || o.max_target_points > (1 << 24) || o.max_frames_per_submap < 1 ||
        o.max_frames_per_submap > 4096 || !(o.transformation_eps >= 0.0) || !(o.fitness_eps >= 0.0) || !(o.abs_mse_eps >= 0.0)) {
        glio_set_error("bad glio_loop_opts (leaf %g, max_corr_dist %g, max_iterations %d, capacities %d / %d, frames %d)", (double)o.leaf, o.max_corr_dist, o.max_iterations,
                       o.max_source_points, o.max_target_points, o.max_frames_per_submap);
        return GLIO_E_ARG;
    }
    glio_loop* lp = new glio_loop();
    memset(lp, 0, sizeof *lp);
    lp->o = o;
    { const int rv = glio_bassoc_view(b, &lp->v); if (rv != GLIO_OK) { delete lp; return rv; } }
    const int rc = lp_create_body(lp);
    if (rc != GLIO_OK) { glio_loop_destroy(lp); return rc; }
    *out = lp;
    return GLIO_OK;
}

int glio_loop_build_submap(glio_loop* lp, int which, int n_frames, const int32_t* frame_idx, const double* poses, int* n_points) {
    GLIO_TRACE("glio_loop_build_submap");
    if (!lp || (which != GLIO_LOOP_SOURCE && which != GLIO_LOOP_TARGET) || !frame_idx || !poses) return GLIO_E_ARG;
    if (n_frames < 1 || n_frames > lp->o.max_frames_per_submap) { glio_set_error("glio_loop_build_submap: %d frames, max_frames_per_submap is %d", n_frames, lp->o.max_frames_per_submap); return GLIO_E_ARG; }
    for (int f = 0; f < n_frames; ++f) {
        const int k = frame_idx[f];
        if (k < 0 || k >= lp->v.K) { glio_set_error("glio_loop_build_submap: frame %d outside [0, %d)", k, lp->v.K); return GLIO_E_ARG; }
        if (lp->v.h_n[k] < 1) { glio_set_error("glio_loop_build_submap: frame %d was never set (or holds no point)", k); return GLIO_E_ARG; }
        for (int c = 0; c < 7; ++c) if (!(fabs(poses[7 * f + c]) <= DBL_MAX)) { glio_set_error("glio_loop_build_submap: pose %d is not finite", f); return GLIO_E_ARG; }
        lp->h_src[f] = lp->v.d_local + (size_t)k * lp->v.cap; lp->h_nsrc[f] = lp->v.h_n[k];
    }
    LP_CHECK(hipSetDevice(lp->v.device));
    { const int ro = lp_order_behind_assoc(lp); if (ro != GLIO_OK) return ro; }
    const int cap = which == GLIO_LOOP_SOURCE ? lp->o.max_source_points : lp->o.max_target_points;
    lp_submap_changed(lp, which, 0);               // (whatever happens below, the old submap is gone: its buffer is the destination)
    int nv = 0;
    { const int rv = glio_vg_build(lp->vg, lp->stream, n_frames, lp->h_src, lp->h_nsrc, poses, lp->d_pts[which], cap, &nv); if (rv != GLIO_OK) return rv; }
    if (nv > cap) { glio_set_error("glio_loop_build_submap: %d voxels, the %s submap takes %d", nv, which == GLIO_LOOP_SOURCE ? "source" : "target", cap); return GLIO_E_ARG; }
    if (nv < 1) { glio_set_error("glio_loop_build_submap: empty submap"); return GLIO_E_ARG; }
    lp_submap_changed(lp, which, nv);
    if (n_points) *n_points = nv;
    return GLIO_OK;
}

int glio_loop_set_submap(glio_loop* lp, int which, const float* xyzi, int n) {
    if (!lp || (which != GLIO_LOOP_SOURCE && which != GLIO_LOOP_TARGET)) return GLIO_E_ARG;
    const int cap = which == GLIO_LOOP_SOURCE ? lp->o.max_source_points : lp->o.max_target_points;
    if (n < 1 || !xyzi) { glio_set_error("glio_loop_set_submap: empty submap"); return GLIO_E_ARG; }
    if (n > cap) { glio_set_error("glio_loop_set_submap: %d points, the %s submap takes %d", n, which == GLIO_LOOP_SOURCE ? "source" : "target", cap); return GLIO_E_ARG; }
    LP_CHECK(hipSetDevice(lp->v.device));
    LP_CHECK(hipStreamSynchronize(lp->stream));      // (an alignment that still reads the old submap)
    LP_CHECK(hipMemcpyAsync(lp->d_pts[which], xyzi, (size_t)n * 16, hipMemcpyHostToDevice, lp->stream));
    LP_CHECK(hipStreamSynchronize(lp->stream));      // the caller's buffer may be reused after return
    lp_submap_changed(lp, which, n);
    return GLIO_OK;
}

int glio_loop_read_submap(glio_loop* lp, int which, float* out_xyzi, int capacity, int* n) {
    if (!lp || (which != GLIO_LOOP_SOURCE && which != GLIO_LOOP_TARGET) || !n) return GLIO_E_ARG;
    *n = lp->n[which];
    if (out_xyzi && lp->n[which] > 0) {
        if (capacity < lp->n[which]) return GLIO_E_ARG;
        LP_CHECK(hipSetDevice(lp->v.device));
        LP_CHECK(hipStreamSynchronize(lp->stream));
        LP_CHECK(hipMemcpy(out_xyzi, lp->d_pts[which], (size_t)lp->n[which] * 16, hipMemcpyDeviceToHost));
    }
    return GLIO_OK;
}

int glio_loop_reset_current(glio_loop* lp) {
    { const int rr = lp_ready(lp); if (rr != GLIO_OK) return rr; }
    LP_CHECK(hipSetDevice(lp->v.device));
    return lp_reset_current(lp);
}

int glio_loop_align(glio_loop* lp, glio_loop_result* result) {
    GLIO_TRACE("glio_loop_align");
    if (!result) return GLIO_E_ARG;
    { const int rr = lp_ready(lp); if (rr != GLIO_OK) return rr; }
    LP_CHECK(hipSetDevice(lp->v.device));
    if (lp->tgt_dirty) { const int rg = lp_build_grid(lp); if (rg != GLIO_OK) return rg; }
    LP_CHECK(hipEventRecord(lp->ev_t0, lp->stream));
    { const int rc = lp_reset_current(lp); if (rc != GLIO_OK) return rc; }
    for (int r = 0; r < lp->o.max_iterations; ++r) {
        lp_enqueue_round(lp, r);
    }
    // getFitnessScore: every point of the final cloud, no distance cap
    const int ns = lp->n[GLIO_LOOP_SOURCE], nblk = (ns + 255) / 256;
    lp_enqueue_search(lp, 0);
    hipLaunchKernelGGL(k_lp_reduce_a, dim3(nblk), dim3(256), 0, lp->stream, lp->d_cur, ns, lp->d_pts[GLIO_LOOP_TARGET], lp->d_idx, lp->d_d2, lp->d_st, 0, 1, lp->d_partA);
    hipLaunchKernelGGL(k_lp_finish, dim3(1), dim3(256), 0, lp->stream, lp->d_st, lp->d_partA, nblk, ns, lp->d_res);
    LP_CHECK(hipGetLastError());
    LP_CHECK(hipEventRecord(lp->ev_t1, lp->stream));
    LP_CHECK(hipMemcpyAsync(lp->h_res, lp->d_res, sizeof(glio_loop_result), hipMemcpyDeviceToHost, lp->stream));
    LP_CHECK(hipEventRecord(lp->ev_done, lp->stream));
    LP_CHECK(hipEventSynchronize(lp->ev_done));
    *result = *lp->h_res;
    lp->have_ms = 1;
    lp->hist_n = lp->o.max_iterations;
    return GLIO_OK;
}

int glio_loop_step(glio_loop* lp, glio_loop_step_result* step) {
    if (!step) return GLIO_E_ARG;
    { const int rr = lp_ready(lp); if (rr != GLIO_OK) return rr; }
    LP_CHECK(hipSetDevice(lp->v.device));
    if (lp->tgt_dirty) { const int rg = lp_build_grid(lp); if (rg != GLIO_OK) return rg; }
    if (!lp->cur_valid) { const int rc = lp_reset_current(lp); if (rc != GLIO_OK) return rc; }
    hipLaunchKernelGGL(k_lp_begin, dim3(1), dim3(64), 0, lp->stream, lp->d_st, 1, lp->o);
    lp_enqueue_round(lp, -1);
    hipLaunchKernelGGL(k_lp_pack_step, dim3(1), dim3(64), 0, lp->stream, lp->d_st, lp->d_step);
    LP_CHECK(hipGetLastError());
    LP_CHECK(hipMemcpyAsync(lp->h_step, lp->d_step, sizeof(glio_loop_step_result), hipMemcpyDeviceToHost, lp->stream));
    LP_CHECK(hipEventRecord(lp->ev_done, lp->stream));
    LP_CHECK(hipEventSynchronize(lp->ev_done));
    *step = *lp->h_step;
    return GLIO_OK;
}

int glio_loop_read_correspondences(glio_loop* lp, int32_t* idx_out, float* d2_out) {
    { const int rr = lp_ready(lp); if (rr != GLIO_OK) return rr; }
    LP_CHECK(hipSetDevice(lp->v.device));
    LP_CHECK(hipStreamSynchronize(lp->stream));
    const size_t ns = (size_t)lp->n[GLIO_LOOP_SOURCE];
    if (idx_out) LP_CHECK(hipMemcpy(idx_out, lp->d_idx, ns * 4, hipMemcpyDeviceToHost));
    if (d2_out) LP_CHECK(hipMemcpy(d2_out, lp->d_d2, ns * 4, hipMemcpyDeviceToHost));
    return GLIO_OK;
}

int glio_loop_read_current(glio_loop* lp, float* out_xyzi, int capacity, int* n) {
    if (!lp || !n) return GLIO_E_ARG;
    const int ns = lp->cur_valid ? lp->n[GLIO_LOOP_SOURCE] : 0;
    *n = ns;
    if (out_xyzi && ns > 0) {
        if (capacity < ns) return GLIO_E_ARG;
        LP_CHECK(hipSetDevice(lp->v.device));
        LP_CHECK(hipStreamSynchronize(lp->stream));
        LP_CHECK(hipMemcpy(out_xyzi, lp->d_cur, (size_t)ns * 16, hipMemcpyDeviceToHost));
    }
    return GLIO_OK;
}

int glio_loop_read_fallbacks(glio_loop* lp, int32_t* out, int capacity, int* n) {
    if (!lp || !n || !lp->h_res) return GLIO_E_ARG;
    if (lp->hist_n < 1) { *n = 0; return GLIO_OK; }
    LP_CHECK(hipSetDevice(lp->v.device));
    LP_CHECK(hipStreamSynchronize(lp->stream));
    int rounds = lp->h_res->iterations;
    if (lp->h_res->state == GLIO_LOOP_NO_CORRESPONDENCES || lp->h_res->rank_deficient) rounds += 1;      // (the round that stopped moved nothing but searched)
    if (rounds > lp->hist_n) rounds = lp->hist_n;
    *n = rounds + 1;
    if (!out) return GLIO_OK;
    if (capacity < rounds + 1) return GLIO_E_ARG;
    if (rounds > 0) LP_CHECK(hipMemcpy(out, lp->d_fb_hist, (size_t)rounds * 4, hipMemcpyDeviceToHost));
    LoopState st;
    LP_CHECK(hipMemcpy(&st, lp->d_st, sizeof st, hipMemcpyDeviceToHost));
    out[rounds] = st.fit_fb;
    return GLIO_OK;
}

int glio_loop_last_device_ms(glio_loop* lp, float* ms) {
    if (!lp || !ms) return GLIO_E_ARG;
    if (!lp->have_ms) { glio_set_error("glio_loop_align first"); return GLIO_E_STATE; }
    LP_CHECK(hipSetDevice(lp->v.device));
    LP_CHECK(hipEventSynchronize(lp->ev_t1));
    LP_CHECK(hipEventElapsedTime(ms, lp->ev_t0, lp->ev_t1));
    return GLIO_OK;
}

}  // extern "C"

// covariance_kernels.hip -- selected rows and columns of H^-1 for the window's dense H = J^T J (include/glio_cov.h), fp64 throughout.
//
//   Sigma_SS = Y^T Y,  Y = L^-1 E_S,  H_ff = L L^T  over the columns f that some factor touches (H_kk != 0).
//
//   k_cov_scan      (n > 88)  free-column scan: map[k] = compact index or -1, idx[] its inverse, the info record
//   k_cov_compact   (n > 88)  A = H[idx][idx], lower triangle
//   k_cov_small     (n <= 88) scan + compaction + the whole factorisation in ONE workgroup's LDS (the released window has n = 75)
//   k_cov_panel     (n > 88)  one 32-column panel: every workgroup factors the 32 x 32 diagonal block for itself in LDS (11k flops, the same bits everywhere)
//                             and solves 64 rows below it, one row per lane in registers; workgroup 0 also writes the diagonal block and the pivot record
//   k_cov_trail     (n > 88)  the rank-32 update of the rest, one 64 x 64 tile of the lower triangle per workgroup, v_mfma_f64_16x16x4_f64 over LDS-staged
//                             panel rows.  One launch pair per panel: the launch boundary is the only barrier between workgroups.
//   k_cov_forward             L y = e_s, one wavefront per asked column, starting at the column's own row: 64 rows per round, their part against the
//                             rows already solved as one fixed-order sum per lane, the 64 x 64 diagonal block in registers with the pivots by shuffle
//   k_cov_gram                entry (a, b) = sum over k of Y[a][k] Y[b][k] in ascending k, one thread per entry of a 16 x 16 tile, tiles on and below the
//                             diagonal, each value stored to (a, b) and (b, a)
// L is kept TRANSPOSED (Lt[k][i] = L[i][k], i >= k): every kernel above then reads and writes it with consecutive lanes on consecutive addresses.
// Every sum has a fixed order that depends on the entry's own column(s) only, and no atomic takes part: see "BITS" in the header.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/glio_cov.h"
#include "glio_device.h"

#define COV_SMALL_MAX 88           // 88 rows of stride 89 doubles: 62 656 of the 65 536 bytes a workgroup may declare statically
#define COV_NB 32                  // panel width
#define COV_TILE 64                // rows of a panel workgroup; edge of a trailing-update tile; rows of a forward-substitution round
typedef double v4f64 __attribute__((ext_vector_type(4)));

struct GlioCovWs {
    int n_max = 0;
    double *d_A = nullptr, *d_Lt = nullptr, *d_Y = nullptr, *d_out = nullptr;
    int *d_map = nullptr, *d_idx = nullptr, *d_cols = nullptr;
    glio_cov_info* d_info = nullptr;
    char* h_pin = nullptr;          // pinned: glio_cov_info | cols [n_max] | out [n_max][n_max]
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    glio_cov_info* h_info() { return reinterpret_cast<glio_cov_info*>(h_pin); }
    int32_t* h_cols() { return reinterpret_cast<int32_t*>(h_pin + 64); }
    double* h_out() { return reinterpret_cast<double*>(h_pin + 64 + (((size_t)n_max * 4 + 63) & ~(size_t)63)); }
};

// ------------------------------------------------------------------------------------------------ free columns
// One workgroup of NT >= n threads.  Returns the number of columns kept (the same value in every thread).
template <int NT>
__device__ int cov_scan(const double* __restrict__ H, const int ldh, const int n, const int m, const int* __restrict__ cols, int* __restrict__ map,
                        int* __restrict__ idx, glio_cov_info* __restrict__ info, int* sh) {
    const int t = threadIdx.x;
    const bool in = t < n;
    const bool fr = in && H[(size_t)t * ldh + t] == 0.0;
    sh[t] = (in && !fr) ? 1 : 0;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int x = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const int incl = sh[t], nf = sh[NT - 1];
    if (in) {
        map[t] = fr ? -1 : incl - 1;
        if (!fr) idx[incl - 1] = t;
    }
    __syncthreads();
    int cnt = 0;
    for (int c = t; c < m; c += NT) { const int k = cols[c]; cnt += H[(size_t)k * ldh + k] == 0.0 ? 1 : 0; }
    sh[t] = cnt;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (t < off) sh[t] += sh[t + off];
        __syncthreads();
    }
    if (t == 0) { info->n = n; info->n_free = n - nf; info->n_free_asked = sh[0]; info->bad_pivot = -1; info->min_pivot = 0.0; info->max_pivot = 0.0; }
    __syncthreads();
    return nf;
}
__global__ __launch_bounds__(1024) void k_cov_scan(const double* __restrict__ H, const int n, const int m, const int* __restrict__ cols, int* __restrict__ map,
                                                   int* __restrict__ idx, glio_cov_info* __restrict__ info) {
    __shared__ int sh[1024];
    cov_scan<1024>(H, n, n, m, cols, map, idx, info, sh);
}
// grid (ceil(n / 256), n): entry (i, j), j <= i < nf, of the kept system
__global__ __launch_bounds__(256) void k_cov_compact(const double* __restrict__ H, const int n, const int* __restrict__ idx, const glio_cov_info* __restrict__ info,
                                                     double* __restrict__ A, const int ld) {
    const int nf = n - info->n_free, i = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (i >= nf || j > i) return;
    A[(size_t)i * ld + j] = H[(size_t)idx[i] * n + idx[j]];
}

__device__ __forceinline__ bool cov_pivot_ok(const double p) { return p > 0.0 && p < INFINITY; }

// ------------------------------------------------------------------------------------------------ n <= 88: one workgroup, everything in LDS
// Left looking, one row per thread: column k of L is a_ik - sum_{j < k} l_ij l_kj (ascending j) over sqrt(pivot); two barriers per column.
__global__ __launch_bounds__(128) void k_cov_small(const double* __restrict__ H, const int n, const int m, const int* __restrict__ cols, int* __restrict__ map,
                                                   int* __restrict__ idx, glio_cov_info* __restrict__ info, double* __restrict__ Lt, const int ld) {
    constexpr int LS = COV_SMALL_MAX + 1;
    __shared__ double S[COV_SMALL_MAX * LS];
    __shared__ int sh[128];
    __shared__ double piv;
    const int nf = cov_scan<128>(H, n, n, m, cols, map, idx, info, sh);
    const int i = threadIdx.x;
    if (i < nf) {
        const int hi = idx[i];
        for (int j = 0; j <= i; ++j) S[i * LS + j] = H[(size_t)hi * n + idx[j]];
    }
    __syncthreads();
    double pmin = INFINITY, pmax = 0.0;
    for (int k = 0; k < nf; ++k) {
        double s = 0.0;
        if (i >= k && i < nf) {
            s = S[i * LS + k];
            for (int j = 0; j < k; ++j) s = fma(-S[i * LS + j], S[k * LS + j], s);
            if (i == k) piv = s;
        }
        __syncthreads();
        const double p = piv;
        if (!cov_pivot_ok(p)) {                       // (the same p in every thread: all leave together)
            if (i == 0) info->bad_pivot = idx[k];
            return;
        }
        pmin = fmin(pmin, p); pmax = fmax(pmax, p);
        const double r = sqrt(p);
        if (i >= k && i < nf) S[i * LS + k] = i == k ? r : s / r;
        __syncthreads();
    }
    if (i == 0 && nf > 0) { info->min_pivot = pmin; info->max_pivot = pmax; }
    for (int e = i; e < nf * nf; e += 128) {
        const int k = e / nf, r = e - k * nf;
        if (r >= k) Lt[(size_t)k * ld + r] = S[r * LS + k];
    }
}

// ------------------------------------------------------------------------------------------------ n > 88: panel + trailing update
// grid: max(1, ceil((n - k0 - 32) / 64)) workgroups of one wavefront.  Reads A (the diagonal block and the rows below it, as the updates of the earlier
// panels left them), writes Lt only: no workgroup reads what another one writes.
__global__ __launch_bounds__(64) void k_cov_panel(const double* __restrict__ A, double* __restrict__ Lt, const int ld, const int n, const int k0,
                                                  const int* __restrict__ idx, glio_cov_info* __restrict__ info) {
    constexpr int DS = COV_NB + 1;
    __shared__ double D[COV_NB * DS];
    __shared__ double piv;
    const int nf = n - info->n_free;
    if (info->bad_pivot >= 0 || k0 >= nf) return;
    const int nb = min(COV_NB, nf - k0), t = threadIdx.x;
    if (t < nb)
        for (int j = 0; j <= t; ++j) D[t * DS + j] = A[(size_t)(k0 + t) * ld + k0 + j];
    __syncthreads();
    double pmin = INFINITY, pmax = 0.0;
    for (int k = 0; k < nb; ++k) {
        double s = 0.0;
        if (t >= k && t < nb) {
            s = D[t * DS + k];
            for (int j = 0; j < k; ++j) s = fma(-D[t * DS + j], D[k * DS + j], s);
            if (t == k) piv = s;
        }
        __syncthreads();
        const double p = piv;
        if (!cov_pivot_ok(p)) {
            if (blockIdx.x == 0 && t == 0) info->bad_pivot = idx[k0 + k];
            return;
        }
        pmin = fmin(pmin, p); pmax = fmax(pmax, p);
        const double r = sqrt(p);
        if (t >= k && t < nb) D[t * DS + k] = t == k ? r : s / r;
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        if (t == 0) {
            info->min_pivot = k0 == 0 ? pmin : fmin(info->min_pivot, pmin);
            info->max_pivot = k0 == 0 ? pmax : fmax(info->max_pivot, pmax);
        }
        for (int e = t; e < nb * nb; e += 64) {
            const int k = e / nb, r = e - k * nb;
            if (r >= k) Lt[(size_t)(k0 + k) * ld + k0 + r] = D[r * DS + k];
        }
    }
    // the rows below the block (there are some only when the panel is full: nb == 32): x L11^T = a, one row per lane
    const int row = k0 + COV_NB + COV_TILE * blockIdx.x + t;
    if (nb < COV_NB || row >= nf) return;
    double x[COV_NB];
#pragma unroll
    for (int j = 0; j < COV_NB; ++j) x[j] = A[(size_t)row * ld + k0 + j];
#pragma unroll
    for (int j = 0; j < COV_NB; ++j) {
        double s = x[j];
#pragma unroll
        for (int q = 0; q < j; ++q) s = fma(-x[q], D[j * DS + q], s);
        x[j] = s / D[j * DS + j];
        Lt[(size_t)(k0 + j) * ld + row] = x[j];
    }
}
// grid (T, T), T = ceil((n - k0 - 32) / 64); workgroup (bx, by) with bx <= by takes the tile at rows by, columns bx of the part below the panel.
// MFMA lane map (f64 16x16x4): a = A[row li][k lk], b = B[k lk][col li], c[q] = C[row lk + 4 q][col li], li = lane & 15, lk = lane >> 4.
__global__ __launch_bounds__(256) void k_cov_trail(double* __restrict__ A, const double* __restrict__ Lt, const int ld, const int n, const int k0,
                                                   const glio_cov_info* __restrict__ info) {
    __shared__ double Pr[COV_NB * COV_TILE], Pc[COV_NB * COV_TILE];
    const int nf = n - info->n_free;
    if (info->bad_pivot >= 0 || blockIdx.x > blockIdx.y) return;
    const int base = k0 + COV_NB, R0 = base + COV_TILE * blockIdx.y, C0 = base + COV_TILE * blockIdx.x;
    if (R0 >= nf) return;
    for (int e = threadIdx.x; e < COV_NB * COV_TILE; e += 256) {
        const int k = e >> 6, r = e & 63;
        Pr[e] = R0 + r < nf ? Lt[(size_t)(k0 + k) * ld + R0 + r] : 0.0;
        Pc[e] = C0 + r < nf ? Lt[(size_t)(k0 + k) * ld + C0 + r] : 0.0;
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
    for (int J = 0; J < 4; ++J) {
        if (C0 + 16 * J > R0 + 16 * w + 15) break;          // wholly above the diagonal
        const int c = C0 + 16 * J + li;
        v4f64 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int r = R0 + 16 * w + lk + 4 * q; acc[q] = (r < nf && c <= r) ? A[(size_t)r * ld + c] : 0.0; }
#pragma unroll
        for (int kk = 0; kk < COV_NB; kk += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Pr[(kk + lk) * COV_TILE + 16 * w + li], Pc[(kk + lk) * COV_TILE + 16 * J + li], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int r = R0 + 16 * w + lk + 4 * q; if (r < nf && c <= r) A[(size_t)r * ld + c] = acc[q]; }
    }
}

// ------------------------------------------------------------------------------------------------ Y = L^-1 E_S
// grid m, one wavefront each.  Column c starts at its own row s = map[cols[c]]; Y[c][k] is written for k >= s only (k_cov_gram masks the rest).
__global__ __launch_bounds__(64) void k_cov_forward(const double* __restrict__ Lt, const int ld, const int n, const int* __restrict__ cols, const int* __restrict__ map,
                                                    const glio_cov_info* __restrict__ info, double* __restrict__ Y, const int ldy) {
    __shared__ double y[GLIO_MAX_UNKNOWNS];
    const int nf = n - info->n_free;
    if (info->bad_pivot >= 0) return;
    const int cidx = blockIdx.x, s = map[cols[cidx]], t = threadIdx.x;
    if (s < 0) return;
    for (int r0 = s; r0 < nf; r0 += COV_TILE) {
        const int row = r0 + t, rc = row < nf ? row : nf - 1;
        double acc = row == s ? 1.0 : 0.0;
#pragma unroll 8
        for (int k = s; k < r0; ++k) acc = fma(-Lt[(size_t)k * ld + rc], y[k], acc);
        double lrow[COV_TILE];
#pragma unroll
        for (int j = 0; j < COV_TILE; ++j) lrow[j] = Lt[(size_t)min(r0 + j, nf - 1) * ld + rc];     // (lanes t < j read above the diagonal: loaded, never used)
        const double ldiag = Lt[(size_t)rc * ld + rc];
#pragma unroll
        for (int j = 0; j < COV_TILE; ++j) {
            if (t == j) acc = acc / ldiag;
            const double yj = __shfl(acc, j);
            if (t > j) acc = fma(-lrow[j], yj, acc);
        }
        if (row < nf) { y[row] = acc; Y[(size_t)cidx * ldy + row] = acc; }
        __syncthreads();
    }
}
// grid (ceil(m / 16), ceil(m / 16)) of 16 x 16 threads; tiles with bx <= by.  out [m][m].
__global__ __launch_bounds__(256) void k_cov_gram(const double* __restrict__ Y, const int ldy, const int n, const int m, const int* __restrict__ cols,
                                                  const int* __restrict__ map, const glio_cov_info* __restrict__ info, double* __restrict__ out) {
    __shared__ double Ya[16 * 65], Yb[16 * 65];
    __shared__ int sa[16], sb[16];
    if (info->bad_pivot >= 0 || blockIdx.x > blockIdx.y) return;
    const int nf = n - info->n_free, tx = threadIdx.x, ty = threadIdx.y;
    const int a = 16 * blockIdx.y + ty, b = 16 * blockIdx.x + tx;
    if (ty == 0) { const int ca = 16 * blockIdx.y + tx, cb = 16 * blockIdx.x + tx; sa[tx] = ca < m ? map[cols[ca]] : -1; sb[tx] = cb < m ? map[cols[cb]] : -1; }
    __syncthreads();
    int kmin = nf;
    for (int q = 0; q < 16; ++q) { if (sa[q] >= 0) kmin = min(kmin, sa[q]); if (sb[q] >= 0) kmin = min(kmin, sb[q]); }
    const int my_sa = sa[ty], my_sb = sb[ty];          // the row of the staging tiles this thread fills
    double acc = 0.0;
    for (int kc = kmin; kc < nf; kc += 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = kc + tx + 16 * q;
            Ya[ty * 65 + tx + 16 * q] = (my_sa >= 0 && k < nf && k >= my_sa) ? Y[(size_t)(16 * blockIdx.y + ty) * ldy + k] : 0.0;
            Yb[ty * 65 + tx + 16 * q] = (my_sb >= 0 && k < nf && k >= my_sb) ? Y[(size_t)(16 * blockIdx.x + ty) * ldy + k] : 0.0;
        }
        __syncthreads();
#pragma unroll 16
        for (int kk = 0; kk < 64; ++kk) acc = fma(Ya[ty * 65 + kk], Yb[tx * 65 + kk], acc);
        __syncthreads();
    }
    if (a < m && b < m) {
        if (sa[ty] < 0 || sb[tx] < 0) acc = a == b ? INFINITY : 0.0;       // a free column: no information
        out[(size_t)a * m + b] = acc;
        out[(size_t)b * m + a] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ host
void glio_cov_free(GlioCovWs* ws) {
    if (!ws) return;
    hipFree(ws->d_A); hipFree(ws->d_Lt); hipFree(ws->d_Y); hipFree(ws->d_out); hipFree(ws->d_map); hipFree(ws->d_idx); hipFree(ws->d_cols); hipFree(ws->d_info);
    if (ws->h_pin) hipHostFree(ws->h_pin);
    if (ws->ev0) hipEventDestroy(ws->ev0);
    if (ws->ev1) hipEventDestroy(ws->ev1);
    delete ws;
}
static int cov_alloc(glio_ctx* c, GlioCovWs** out) {
    GlioCovWs* ws = new GlioCovWs;
    *out = ws;                                         // (owned by the context from here on: a partial allocation is freed with it)
    ws->n_max = c->n_max;
    const size_t nn = (size_t)c->n_max * c->n_max * 8;
    GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_A, nn)); GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_Lt, nn));
    GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_Y, nn)); GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_out, nn));
    GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_map, (size_t)c->n_max * 4)); GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_idx, (size_t)c->n_max * 4));
    GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_cols, (size_t)c->n_max * 4)); GLIO_HIP_CHECK(hipMalloc((void**)&ws->d_info, sizeof(glio_cov_info)));
    GLIO_HIP_CHECK(hipHostMalloc((void**)&ws->h_pin, 64 + (((size_t)c->n_max * 4 + 63) & ~(size_t)63) + nn, hipHostMallocDefault));
    GLIO_HIP_CHECK(hipEventCreate(&ws->ev0)); GLIO_HIP_CHECK(hipEventCreate(&ws->ev1));
    return GLIO_OK;
}
// Checks the request, allocates the workspace at the first call and marks the start of the device time.  Nothing on the device has changed when it refuses.
int glio_cov_begin(glio_ctx* c, GlioCovWs** pws, int n, int m, const int32_t* cols) {
    if (m < 1 || m > n) { glio_set_error("covariance: %d columns asked of a system of %d", m, n); return GLIO_E_ARG; }
    std::vector<char> seen((size_t)n, 0);
    for (int k = 0; k < m; ++k) {
        if (cols[k] < 0 || cols[k] >= n) { glio_set_error("covariance: column %d is outside [0, %d)", (int)cols[k], n); return GLIO_E_ARG; }
        if (seen[cols[k]]) { glio_set_error("covariance: column %d is listed twice", (int)cols[k]); return GLIO_E_ARG; }
        seen[cols[k]] = 1;
    }
    if (!*pws) { const int rc = cov_alloc(c, pws); if (rc) return rc; }
    GlioCovWs* ws = *pws;
    if (!ws->h_pin || !ws->ev1) { glio_set_error("covariance: the workspace could not be allocated"); return GLIO_E_HIP; }
    memcpy(ws->h_cols(), cols, (size_t)m * 4);
    ws->timed = false;
    GLIO_HIP_CHECK(hipEventRecord(ws->ev0, c->stream));
    return GLIO_OK;
}
// The staging area a caller's matrix goes to (glio_debug_covariance_of): the result buffer, which nothing reads before the last kernel writes it.
double* glio_cov_staging(GlioCovWs* ws) { return ws->d_out; }
// d_H: n x n row major on the device, only the lower triangle is read.  The one host wait of the call is in here.
int glio_cov_finish(glio_ctx* c, GlioCovWs* ws, const double* d_H, int n, int m, double* out, glio_cov_info* info) {
    hipStream_t st = c->stream;
    const int ld = ws->n_max;
    GLIO_HIP_CHECK(hipMemcpyAsync(ws->d_cols, ws->h_cols(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (n <= COV_SMALL_MAX) {
        hipLaunchKernelGGL(k_cov_small, dim3(1), dim3(128), 0, st, d_H, n, m, ws->d_cols, ws->d_map, ws->d_idx, ws->d_info, ws->d_Lt, ld);
    } else {
        hipLaunchKernelGGL(k_cov_scan, dim3(1), dim3(1024), 0, st, d_H, n, m, ws->d_cols, ws->d_map, ws->d_idx, ws->d_info);
        hipLaunchKernelGGL(k_cov_compact, dim3((n + 255) / 256, n), dim3(256), 0, st, d_H, n, ws->d_idx, ws->d_info, ws->d_A, ld);
        for (int k0 = 0; k0 < n; k0 += COV_NB) {
            const int below = n - k0 - COV_NB, T = below > 0 ? (below + COV_TILE - 1) / COV_TILE : 0;
            hipLaunchKernelGGL(k_cov_panel, dim3(T > 0 ? T : 1), dim3(64), 0, st, ws->d_A, ws->d_Lt, ld, n, k0, ws->d_idx, ws->d_info);
            if (T > 0) hipLaunchKernelGGL(k_cov_trail, dim3(T, T), dim3(256), 0, st, ws->d_A, ws->d_Lt, ld, n, k0, ws->d_info);
        }
    }
    hipLaunchKernelGGL(k_cov_forward, dim3(m), dim3(64), 0, st, ws->d_Lt, ld, n, ws->d_cols, ws->d_map, ws->d_info, ws->d_Y, ld);
    const int mt = (m + 15) / 16;
    hipLaunchKernelGGL(k_cov_gram, dim3(mt, mt), dim3(16, 16), 0, st, ws->d_Y, ld, n, m, ws->d_cols, ws->d_map, ws->d_info, ws->d_out);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipMemcpyAsync(ws->h_info(), ws->d_info, sizeof(glio_cov_info), hipMemcpyDeviceToHost, st));
    GLIO_HIP_CHECK(hipMemcpyAsync(ws->h_out(), ws->d_out, (size_t)m * m * 8, hipMemcpyDeviceToHost, st));
    GLIO_HIP_CHECK(hipEventRecord(ws->ev1, st));
    GLIO_HIP_CHECK(hipStreamSynchronize(st));
    ws->timed = true;
    const glio_cov_info got = *ws->h_info();
    if (info) *info = got;
    if (got.bad_pivot >= 0) {
        glio_set_error("covariance: H is not positive definite (pivot of column %d is not positive and finite)", got.bad_pivot);
        return GLIO_E_NUMERIC;
    }
    memcpy(out, ws->h_out(), (size_t)m * m * 8);
    return GLIO_OK;
}
int glio_cov_last_ms(GlioCovWs* ws, float* ms) {
    if (!ws || !ws->timed) { glio_set_error("covariance: no call has completed on this context"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, ws->ev0, ws->ev1));
    return GLIO_OK;
}

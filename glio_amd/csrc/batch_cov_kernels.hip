// batch_cov_kernels.hip -- the marginal covariance of every keyframe of the batch problem (include/glio_batch_cov.h): the diagonal blocks of H^-1
// and the blocks (k, k + 1), by a SELECTED INVERSION down the elimination tree of the block cyclic reduction (batch_solve_kernels.hip).
//
// The reduction leaves, per node p eliminated between the then-active neighbours a < p < b, L (A_pp = L L^T after the Schur updates of the levels
// below), U_a = A_ap L^-T and U_b = A_bp L^-T.  With T_a = U_a L^-1, T_b = U_b L^-1 (= A_ap A_pp^-1, A_bp A_pp^-1) the blocks of the inverse obey
//     Sigma_pa = -T_a^T Sigma_aa - T_b^T Sigma_ba          Sigma_pb = -T_a^T Sigma_ab - T_b^T Sigma_bb
//     Sigma_pp = L^-T L^-1 - Sigma_pa T_a - Sigma_pb T_b   (a root: L^-T L^-1)
// walked from the last level to the first.  Sigma_ab is always at hand: once p is gone a and b are adjacent, so the one of them eliminated first
// had the other as its neighbour and produced that block one or more levels up.  Every adjacent pair of super-blocks has a member eliminated at
// level 0, which is where the (k, k + 1) blocks across a super-block boundary come from.
//
//   k_cov_scale    S = diag(1 / sqrt(H_kk)) from the linearisation's replicated diagonal; the anchor's six pose columns get scale 0 and an additive
//                  diagonal 1 -- through the solver's own operator (BcrOp.sc / .dadd) that is the identity block with zero couplings of a padding
//                  keyframe.  A diagonal entry elsewhere that is not positive and finite is a bad pivot.
//   (factor)       glio_bcr_enqueue_local: k_bcr_pre / k_bcr_init, k_bcr_elim / k_bcr_elim2, k_bcr_update, unchanged
//   k_cov_tri      X L = U for the rows of [I; U_a; U_b] of every node (and [I; U] of every pre-elimination) at once: one row per lane, the whole
//                  back substitution inside the lane -- no barrier, no shuffle; L is read from LDS as a broadcast
//   k_cov_down     one launch per level, one workgroup per node: the seven M x M products above on v_mfma_f64_16x16x4 over LDS-staged operands
//   k_cov_pre      with the IMU chain: the pre-eliminated speed / bias blocks of a super-block's inner keyframes from preL / preU the same way
//   k_cov_gather   the B x B blocks per keyframe and per (k, k + 1) out of Sigma_ss / Sigma_{s,s+1}, unscaled by S; the lower triangle mirrored
// Every sum has a fixed order (the MFMA chains run over k in order, one tile per wavefront): two runs are bit-identical.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/glio_batch_cov.h"
#include "batch_device.h"

typedef double cov_v4f64 __attribute__((ext_vector_type(4)));
#define COV_TH 512
#define COV_LD 93              // row stride of a staged operand: 4 ceil(90 / 4) | 1 (odd: the 16 rows of an MFMA operand lie on distinct banks)
#define COV_ROWS 96            // rows of a staged operand, 16 ceil(90 / 16)
#define COV_MAX 90             // largest block the reduction works on
#define COV_DOWN_LDS(m) ((size_t)2 * ((((m) + 15) / 16) * 16) * COV_LD * 8)
#define COV_TRI_LDS(n, rows) ((size_t)((n) + (rows)) * ((n) | 1) * 8)

struct CovStatus { int sbad; int skf; int fail; int ord; double minp, maxp; };       // sbad: a diagonal entry was bad, skf: the smallest such keyframe
struct CovNode { int node, a, b, from_a; };          // from_a: Sigma_ab lies with a (its right cross block), else with b (its left one, transposed)

// ------------------------------------------------------------------------------------------------ scale
__global__ void k_cov_init(CovStatus* st, int* bcr_fail) {
    if (threadIdx.x == 0) { st->sbad = 0; st->skf = INT_MAX; st->fail = 0; st->ord = INT_MAX; st->minp = 0.0; st->maxp = 0.0; bcr_fail[1] = INT_MAX; }
}
__global__ void k_cov_scale(const double* __restrict__ diag, const int n, const int B, const int anchor, double* __restrict__ sc, double* __restrict__ dadd,
                            CovStatus* st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = i / B, r = i - B * k;
    if (k == anchor && r < 6) { sc[i] = 0.0; dadd[i] = 1.0; return; }
    const double d = diag[i];
    double s = 1.0;
    if (!(d > 0.0) || !isfinite(d)) { st->sbad = 1; atomicMin(&st->skf, k); } else s = 1.0 / sqrt(d);
    sc[i] = s; dadd[i] = 0.0;
}

// ------------------------------------------------------------------------------------------------ X L = U, one row per lane
struct CovTri {
    const double* L; long long sL; int n, nparts;
    const double* src[3]; long long ssrc[3]; int rows[3];      // src null: the identity (rows = n): X = L^-1
    double* dst[3]; long long sdst[3];
};
__global__ __launch_bounds__(128) void k_cov_tri(const CovTri t) {
    extern __shared__ double cov_lds[];
    const int n = t.n, LD = n | 1, part = blockIdx.y, rows = t.rows[part], tid = threadIdx.x;
    double* Ls = cov_lds;                  // [n][LD]
    double* X = Ls + n * LD;               // [rows][LD]
    const double* Lg = t.L + (size_t)blockIdx.x * t.sL;
    const double* src = t.src[part] ? t.src[part] + (size_t)blockIdx.x * t.ssrc[part] : nullptr;
    for (int e = tid; e < n * n; e += 128) { const int r = e / n, c = e - n * r; Ls[r * LD + c] = Lg[e]; }
    for (int e = tid; e < rows * n; e += 128) { const int r = e / n, c = e - n * r; X[r * LD + c] = src ? src[e] : (r == c ? 1.0 : 0.0); }
    __syncthreads();
    if (tid < rows) {
        double* x = X + tid * LD;
        for (int j = n - 1; j >= 0; --j) {          // x_j = (u_j - sum_{k > j} x_k L_kj) / L_jj
            double s0 = 0.0, s1 = 0.0;
            int k = j + 1;
            for (; k + 1 < n; k += 2) { s0 += x[k] * Ls[k * LD + j]; s1 += x[k + 1] * Ls[(k + 1) * LD + j]; }
            if (k < n) s0 += x[k] * Ls[k * LD + j];
            x[j] = (x[j] - (s0 + s1)) / Ls[j * LD + j];
        }
    }
    __syncthreads();
    double* dst = t.dst[part] + (size_t)blockIdx.x * t.sdst[part];
    for (int e = tid; e < rows * n; e += 128) { const int r = e / n, c = e - n * r; dst[e] = X[r * LD + c]; }
}

// ------------------------------------------------------------------------------------------------ products on the matrix core
// dst [R][KP] (stride COV_LD) = src [R][Kd] (row stride lds), or its transpose (tr: entry (r, c) = src[c lds + r]); rows up to the next multiple
// of 16 and columns up to the next multiple of 4 are zero
__device__ __forceinline__ void cov_stage(double* __restrict__ dst, const double* __restrict__ src, const int R, const int Kd, const int lds, const bool tr) {
    const int RP = ((R + 15) >> 4) << 4, KP = ((Kd + 3) >> 2) << 2, N = RP * KP;
    constexpr int U = 4;
    for (int e0 = threadIdx.x; e0 < N; e0 += U * COV_TH) {
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * COV_TH;
            int r, c;
            if (tr) { c = e / RP; r = e - RP * c; } else { r = e / KP; c = e - KP * r; }          // (transposed: consecutive lanes walk a source row)
            v[u] = (e < N && r < R && c < Kd) ? (tr ? src[(size_t)c * lds + r] : src[(size_t)r * lds + c]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * COV_TH;
            if (e >= N) continue;
            int r, c;
            if (tr) { c = e / RP; r = e - RP * c; } else { r = e / KP; c = e - KP * r; }
            dst[r * COV_LD + c] = v[u];
        }
    }
}
// dst [R][C] (global, row stride ldd) = (acc ? dst : 0) +- X Y^T, X [R][Kd] and Y [C][Kd] staged.  v_mfma_f64_16x16x4 takes A[i][k] from lane i + 16 k
// and B[k][j] from lane j + 16 k and returns row (lane >> 4) + 4 q, column lane & 15 in register q (k_bcr_update's layout); one tile per wavefront
// at a time, its k loop in order.
__device__ __forceinline__ void cov_xyT(double* __restrict__ dst, const int ldd, const int R, const int C, const int Kd, const bool acc, const bool neg,
                                        const double* __restrict__ X, const double* __restrict__ Y) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int TI = (R + 15) >> 4, TJ = (C + 15) >> 4, KP = ((Kd + 3) >> 2) << 2;
    for (int tile = wave; tile < TI * TJ; tile += COV_TH / 64) {
        const int I = tile / TJ, J = tile - TJ * I;
        cov_v4f64 c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * I + lk + 4 * q, col = 16 * J + li;
            c[q] = (acc && r < R && col < C) ? dst[(size_t)r * ldd + col] : 0.0;
        }
        const double* px = X + (16 * I + li) * COV_LD + lk;
        const double* py = Y + (16 * J + li) * COV_LD + lk;
        for (int k0 = 0; k0 < KP; k0 += 4) { const double a = px[k0]; c = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -a : a, py[k0], c, 0, 0, 0); }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * I + lk + 4 * q, col = 16 * J + li;
            if (r < R && col < C) dst[(size_t)r * ldd + col] = c[q];
        }
    }
}

struct CovBufs {
    const double* W; const double* Ta; const double* Tb;      // [nnode][M M]: L^-1, U_a L^-1, U_b L^-1
    double* Sd; double* XL; double* XR;                       // [nnode][M M]: Sigma_pp, Sigma_{p, left neighbour}, Sigma_{p, right neighbour} (rows p)
    const double* preW; const double* preT;                   // [S][NI NI], [S][NK NI]
    double* Sik; double* Sii;                                 // [S][NI NK], [S][NI NI]
    const int* bcr_fail; const CovStatus* st;
};
__device__ __forceinline__ bool cov_failed(const CovBufs& w) { return w.bcr_fail[0] != 0 || w.st->sbad != 0; }

// ------------------------------------------------------------------------------------------------ down the tree
__global__ __launch_bounds__(COV_TH) void k_cov_down(const CovBufs w, const CovNode* __restrict__ tab, const int M) {
    if (cov_failed(w)) return;
    extern __shared__ double cov_lds[];
    double* XA = cov_lds;
    double* XB = XA + (((M + 15) >> 4) << 4) * COV_LD;
    const CovNode t = tab[blockIdx.x];
    const size_t MM = (size_t)M * M;
    const double* Wp = w.W + t.node * MM; const double* Tap = w.Ta + t.node * MM; const double* Tbp = w.Tb + t.node * MM;
    double* Spp = w.Sd + t.node * MM; double* Spa = w.XL + t.node * MM; double* Spb = w.XR + t.node * MM;
    const bool ha = t.a >= 0, hb = t.b >= 0;
    // Sigma_ab (rows a, columns b) as it lies: with a as its right cross block, or with b as Sigma_ba
    const double* Sab = (ha && hb) ? (t.from_a ? w.XR + t.a * MM : w.XL + t.b * MM) : nullptr;
    if (ha) {          // Sigma_pa = -T_a^T Sigma_aa - T_b^T Sigma_ba: X[i][k] = T[k][i], Y[j][k] = Sigma_aa[j][k] / Sigma_ab[j][k]
        cov_stage(XA, Tap, M, M, M, true); cov_stage(XB, w.Sd + t.a * MM, M, M, M, false);
        __syncthreads();
        cov_xyT(Spa, M, M, M, M, false, true, XA, XB);
        __syncthreads();
        if (hb) {
            cov_stage(XA, Tbp, M, M, M, true); cov_stage(XB, Sab, M, M, M, !t.from_a);
            __syncthreads();
            cov_xyT(Spa, M, M, M, M, true, true, XA, XB);
            __syncthreads();
        }
    }
    if (hb) {          // Sigma_pb = -T_b^T Sigma_bb - T_a^T Sigma_ab: Y[j][k] = Sigma_bb[j][k] / Sigma_ab[k][j]
        cov_stage(XA, Tbp, M, M, M, true); cov_stage(XB, w.Sd + t.b * MM, M, M, M, false);
        __syncthreads();
        cov_xyT(Spb, M, M, M, M, false, true, XA, XB);
        __syncthreads();
        if (ha) {
            cov_stage(XA, Tap, M, M, M, true); cov_stage(XB, Sab, M, M, M, t.from_a != 0);
            __syncthreads();
            cov_xyT(Spb, M, M, M, M, true, true, XA, XB);
            __syncthreads();
        }
    }
    // Sigma_pp = W^T W - Sigma_pa T_a - Sigma_pb T_b
    cov_stage(XA, Wp, M, M, M, true);
    __syncthreads();
    cov_xyT(Spp, M, M, M, M, false, false, XA, XA);
    __syncthreads();
    if (ha) {
        cov_stage(XA, Spa, M, M, M, false); cov_stage(XB, Tap, M, M, M, true);
        __syncthreads();
        cov_xyT(Spp, M, M, M, M, true, true, XA, XB);
        __syncthreads();
    }
    if (hb) {
        cov_stage(XA, Spb, M, M, M, false); cov_stage(XB, Tbp, M, M, M, true);
        __syncthreads();
        cov_xyT(Spp, M, M, M, M, true, true, XA, XB);
    }
}

// ------------------------------------------------------------------------------------------------ the pre-eliminated inner blocks
// super-block s: inner unknowns i (NI), kept unknowns k (NK = M, the node); T = A_ki A_ii^-1 [NK][NI]:
//     Sigma_ik = -T^T Sigma_kk        Sigma_ii = L^-T L^-1 - Sigma_ik T
__global__ __launch_bounds__(COV_TH) void k_cov_pre(const CovBufs w, const int NI, const int NK) {
    if (cov_failed(w)) return;
    extern __shared__ double cov_lds[];
    double* XA = cov_lds;
    double* XB = XA + COV_ROWS * COV_LD;
    const size_t s = blockIdx.x;
    const double* Wi = w.preW + s * NI * NI; const double* T = w.preT + s * NK * NI;
    double* Sik = w.Sik + s * NI * NK; double* Sii = w.Sii + s * NI * NI;
    cov_stage(XA, T, NI, NK, NI, true); cov_stage(XB, w.Sd + s * NK * NK, NK, NK, NK, false);
    __syncthreads();
    cov_xyT(Sik, NK, NI, NK, NK, false, true, XA, XB);
    __syncthreads();
    cov_stage(XA, Wi, NI, NI, NI, true);
    __syncthreads();
    cov_xyT(Sii, NI, NI, NI, NI, false, false, XA, XA);
    __syncthreads();
    cov_stage(XA, Sik, NI, NK, NK, false); cov_stage(XB, T, NI, NK, NI, true);
    __syncthreads();
    cov_xyT(Sii, NI, NI, NI, NK, true, true, XA, XB);
}

// ------------------------------------------------------------------------------------------------ pivots and status
__global__ __launch_bounds__(256) void k_cov_status(const double* __restrict__ L, const int nnode, const int M, const double* __restrict__ preL, const int S,
                                                    const int NI, const int* __restrict__ bcr_fail, CovStatus* st) {
    __shared__ double lo[256], hi[256];
    double mn = INFINITY, mx = 0.0;
    for (int e = threadIdx.x; e < nnode * M; e += 256) { const double d = L[(size_t)(e / M) * M * M + (size_t)(e % M) * (M + 1)]; const double p = d * d; mn = fmin(mn, p); mx = fmax(mx, p); }
    if (preL) for (int e = threadIdx.x; e < S * NI; e += 256) { const double d = preL[(size_t)(e / NI) * NI * NI + (size_t)(e % NI) * (NI + 1)]; const double p = d * d; mn = fmin(mn, p); mx = fmax(mx, p); }
    lo[threadIdx.x] = mn; hi[threadIdx.x] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) { lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + h]); hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + h]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) { st->minp = lo[0]; st->maxp = hi[0]; st->fail = bcr_fail[0]; st->ord = bcr_fail[1]; }
}

// ------------------------------------------------------------------------------------------------ gather
struct CovGather { int K, B, M, sbk, pre, NI, NK, anchor; const int* level; const double* sc; double* diag; double* next; };
// the scaled inverse's entry between unknown (ka, r) and (kb, c); ka <= kb in the same or in neighbouring super-blocks
__device__ __forceinline__ double cov_entry(const CovBufs& w, const CovGather& g, const int ka, const int r, const int kb, const int c) {
    const int sa = ka / g.sbk, sb = kb / g.sbk, la = ka - sa * g.sbk, lb = kb - sb * g.sbk, M = g.M;
    const bool ia = g.pre && la >= 1 && la <= g.sbk - 2 && r >= 6, ib = g.pre && lb >= 1 && lb <= g.sbk - 2 && c >= 6;
    auto kept = [&](const int l, const int q) { return !g.pre ? l * g.B + q : (l == 0 ? q : (l == g.sbk - 1 ? 15 + 6 * (g.sbk - 2) + q : 15 + (l - 1) * 6 + q)); };
    const int pa = ia ? (la - 1) * 9 + r - 6 : kept(la, r), pb = ib ? (lb - 1) * 9 + c - 6 : kept(lb, c);
    if (sa == sb) {
        if (ia && ib) return w.Sii[((size_t)sa * g.NI + pa) * g.NI + pb];
        if (ia) return w.Sik[((size_t)sa * g.NI + pa) * g.NK + pb];
        if (ib) return w.Sik[((size_t)sa * g.NI + pb) * g.NK + pa];
        return w.Sd[((size_t)sa * M + pa) * M + pb];
    }
    // neighbouring super-blocks: the last keyframe of sa and the first of sb are kept whole; the block lies with the one eliminated first
    if (g.level[sa] < g.level[sb]) return w.XR[((size_t)sa * M + pa) * M + pb];
    return w.XL[((size_t)sb * M + pb) * M + pa];
}
__global__ __launch_bounds__(256) void k_cov_gather(const CovBufs w, const CovGather g) {
    if (cov_failed(w)) return;
    const int k = blockIdx.x, B = g.B, BB = B * B;
    const bool fixed_k = k == g.anchor;
    for (int e = threadIdx.x; e < BB; e += 256) {          // block (k, k): the lower triangle, mirrored
        const int r = e / B, c = e - B * r;
        if (c > r) continue;
        double v = 0.0;
        if (!(fixed_k && (r < 6 || c < 6))) v = cov_entry(w, g, k, c, k, r) * (g.sc[(size_t)k * B + r] * g.sc[(size_t)k * B + c]);
        g.diag[(size_t)k * BB + r * B + c] = v;
        g.diag[(size_t)k * BB + c * B + r] = v;
    }
    if (!g.next || k + 1 >= g.K) return;
    const bool fixed_n = k + 1 == g.anchor;
    for (int e = threadIdx.x; e < BB; e += 256) {          // block (k, k + 1)
        const int r = e / B, c = e - B * r;
        double v = 0.0;
        if (!((fixed_k && r < 6) || (fixed_n && c < 6))) v = cov_entry(w, g, k, r, k + 1, c) * (g.sc[(size_t)k * B + r] * g.sc[(size_t)(k + 1) * B + c]);
        g.next[(size_t)k * BB + e] = v;
    }
}

// ------------------------------------------------------------------------------------------------ host
struct BatchCov {
    void* bcr; int B, K, M, nnode, S, NI, NK, levels;          // what the workspaces were sized for
    double* d_sc; double* d_dadd;
    double* d_W; double* d_Ta; double* d_Tb; double* d_Sd; double* d_XL; double* d_XR;
    double* d_preW; double* d_preT; double* d_Sik; double* d_Sii;
    CovNode* d_tab; int* d_level; CovStatus* d_st;
    double* d_out; double* h_out; size_t out_doubles;          // diag | next | CovStatus (pinned copy)
    std::vector<int> elim_off; std::vector<int> node_of_ord;
    hipEvent_t ev[6]; bool timed;
};
static void cov_free(BatchCov* c) {
    void* p[] = {c->d_sc, c->d_dadd, c->d_W, c->d_Ta, c->d_Tb, c->d_Sd, c->d_XL, c->d_XR, c->d_preW, c->d_preT, c->d_Sik, c->d_Sii, c->d_tab, c->d_level, c->d_st, c->d_out};
    for (void* q : p) if (q) hipFree(q);
    if (c->h_out) hipHostFree(c->h_out);
    c->d_sc = c->d_dadd = c->d_W = c->d_Ta = c->d_Tb = c->d_Sd = c->d_XL = c->d_XR = c->d_preW = c->d_preT = c->d_Sik = c->d_Sii = c->d_out = nullptr;
    c->d_tab = nullptr; c->d_level = nullptr; c->d_st = nullptr; c->h_out = nullptr; c->bcr = nullptr;
}
void glio_batch_cov_destroy(glio_batch* b) {
    BatchCov* c = b->cov;
    if (!c) return;
    cov_free(c);
    for (hipEvent_t e : c->ev) if (e) hipEventDestroy(e);
    delete c;
    b->cov = nullptr;
}
static int cov_ensure(glio_batch* b, void* bcr, const BcrView& v) {
    BatchCov* c = b->cov;
    if (c->bcr == bcr && c->B == v.B && c->K == v.K && c->M == v.M && c->nnode == v.nnode && c->S == v.S) return GLIO_OK;
    cov_free(c);
    const int M = v.M, nn = v.nnode, n = v.B * v.K;
    if (M > COV_MAX || v.NI > COV_MAX || v.nnode != v.S) { glio_set_error("batch covariance: unexpected solver shape (M %d, %d nodes, %d super-blocks)", M, v.nnode, v.S); return GLIO_E_STATE; }
    const size_t MM = (size_t)M * M, BB = (size_t)v.B * v.B;
    auto A = [](auto** p, size_t bytes) { return hipMalloc((void**)p, bytes > 0 ? bytes : 16) == hipSuccess; };
    bool ok = A(&c->d_sc, (size_t)n * 8) && A(&c->d_dadd, (size_t)n * 8) && A(&c->d_W, nn * MM * 8) && A(&c->d_Ta, nn * MM * 8) && A(&c->d_Tb, nn * MM * 8) &&
              A(&c->d_Sd, nn * MM * 8) && A(&c->d_XL, nn * MM * 8) && A(&c->d_XR, nn * MM * 8) && A(&c->d_tab, (size_t)(v.n_elim + 1) * sizeof(CovNode)) &&
              A(&c->d_level, (size_t)(nn + 1) * 4) && A(&c->d_st, sizeof(CovStatus));
    if (ok && v.pre) ok = A(&c->d_preW, (size_t)v.S * v.NI * v.NI * 8) && A(&c->d_preT, (size_t)v.S * v.NK * v.NI * 8) && A(&c->d_Sik, (size_t)v.S * v.NI * v.NK * 8) &&
                          A(&c->d_Sii, (size_t)v.S * v.NI * v.NI * 8);
    c->out_doubles = (size_t)v.K * BB + (size_t)(v.K - 1) * BB;
    const size_t out_bytes = c->out_doubles * 8 + sizeof(CovStatus);
    ok = ok && A(&c->d_out, out_bytes) && hipHostMalloc((void**)&c->h_out, out_bytes) == hipSuccess;
    if (!ok) { cov_free(c); (void)hipGetLastError(); glio_set_error("batch covariance: allocation failed"); return GLIO_E_HIP; }
    // the down-sweep's table, in the schedule's order: where Sigma_ab of a node's neighbours lies follows from which of them went first
    std::vector<int> level(nn, 0);
    c->elim_off.assign(v.h_elim_off, v.h_elim_off + v.levels + 1);
    for (int l = 0; l < v.levels; ++l) for (int e = c->elim_off[l]; e < c->elim_off[l + 1]; ++e) level[v.h_elim[e].node] = l;
    std::vector<CovNode> tab(v.n_elim + 1);
    c->node_of_ord.assign(v.n_elim, 0);
    for (int e = 0; e < v.n_elim; ++e) {
        const BcrElim& t = v.h_elim[e];
        tab[e].node = t.node; tab[e].a = t.a; tab[e].b = t.b;
        tab[e].from_a = (t.a >= 0 && t.b >= 0 && level[t.a] < level[t.b]) ? 1 : 0;
        c->node_of_ord[e] = t.node;
    }
    GLIO_HIP_CHECK(hipMemcpy(c->d_tab, tab.data(), (size_t)v.n_elim * sizeof(CovNode), hipMemcpyHostToDevice));
    GLIO_HIP_CHECK(hipMemcpy(c->d_level, level.data(), (size_t)nn * 4, hipMemcpyHostToDevice));
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_cov_down), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_DOWN_LDS(COV_MAX));
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_cov_pre), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_DOWN_LDS(COV_MAX));
    hipFuncSetAttribute(reinterpret_cast<const void*>(k_cov_tri), hipFuncAttributeMaxDynamicSharedMemorySize, (int)COV_TRI_LDS(COV_MAX, COV_MAX));
    (void)hipGetLastError();
    c->bcr = bcr; c->B = v.B; c->K = v.K; c->M = M; c->nnode = nn; c->S = v.S; c->NI = v.NI; c->NK = v.NK; c->levels = v.levels;
    return GLIO_OK;
}

extern "C" {

int glio_batch_cov_struct_sizes(int32_t* out, int n) {
    if (!out || n < 1) return 1;
    out[0] = (int32_t)sizeof(glio_batch_cov_info);
    return 1;
}

int glio_batch_covariance(glio_batch* b, const double* poses, const double* speed_bias, int anchor_keyframe, double* diag, double* next, glio_batch_cov_info* info) {
    GLIO_TRACE("batch covariance glio_batch_covariance");
    if (!b || !poses || !diag) { glio_set_error("batch covariance: null stage, poses or diag"); return GLIO_E_ARG; }
    if (anchor_keyframe < -1 || anchor_keyframe >= b->K) { glio_set_error("batch covariance: anchor keyframe %d outside [-1, %d)", anchor_keyframe, b->K); return GLIO_E_ARG; }
    if (!b->bcr) { glio_set_error("batch covariance: band %d is not covered by the block cyclic reduction", b->band); return GLIO_E_ARG; }
    int has_imu = 0;
    if (glio_batch_tr_world(b, &has_imu) > 1) { glio_set_error("batch covariance: the stage is sharded (not supported)"); return GLIO_E_STATE; }
    if (has_imu && !speed_bias) { glio_set_error("the IMU chain is set: speed_bias [K][9] is needed"); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    if (!b->cov) {
        b->cov = new BatchCov();
        for (hipEvent_t& e : b->cov->ev) GLIO_HIP_CHECK(hipEventCreate(&e));
    }
    GLIO_HIP_CHECK(hipEventRecord(b->cov->ev[0], st));
    BcrOp op; const double* d_diag = nullptr; void* bcr = nullptr; int B = 0;
    { const int rc = glio_batch_tr_linearize_at(b, poses, speed_bias, &op, &d_diag, &bcr, &B); if (rc) return rc; }
    BcrView v;
    glio_bcr_view(bcr, &v);
    { const int rc = cov_ensure(b, bcr, v); if (rc) return rc; }
    BatchCov* c = b->cov;
    const int K = b->K, n = B * K, M = v.M;
    const size_t MM = (size_t)M * M, BB = (size_t)B * B;
    GLIO_HIP_CHECK(hipEventRecord(c->ev[1], st));
    // ---- scale and factor S H S (+ the anchor's identity block) in the solver's workspaces
    hipLaunchKernelGGL(k_cov_init, dim3(1), dim3(64), 0, st, c->d_st, v.fail);
    hipLaunchKernelGGL(k_cov_scale, dim3((n + 255) / 256), dim3(256), 0, st, d_diag, n, B, anchor_keyframe, c->d_sc, c->d_dadd, c->d_st);
    op.sc = c->d_sc; op.dadd = c->d_dadd; op.lambda = 0.0; op.cur = nullptr; op.skip = nullptr;
    glio_bcr_enqueue_local(bcr, op, st);
    GLIO_HIP_CHECK(hipEventRecord(c->ev[2], st));
    // ---- L^-1, U_a L^-1, U_b L^-1 of every node; the same of every pre-elimination
    {
        CovTri t; memset(&t, 0, sizeof t);
        t.L = v.L; t.sL = (long long)MM; t.n = M; t.nparts = 3;
        t.src[0] = nullptr; t.src[1] = v.Ua; t.src[2] = v.Ub;
        t.dst[0] = c->d_W; t.dst[1] = c->d_Ta; t.dst[2] = c->d_Tb;
        for (int p = 0; p < 3; ++p) { t.ssrc[p] = (long long)MM; t.sdst[p] = (long long)MM; t.rows[p] = M; }
        hipLaunchKernelGGL(k_cov_tri, dim3(v.nnode, 3), dim3(128), COV_TRI_LDS(M, M), st, t);
        if (v.pre) {
            CovTri u; memset(&u, 0, sizeof u);
            u.L = v.preL; u.sL = (long long)v.NI * v.NI; u.n = v.NI; u.nparts = 2;
            u.src[0] = nullptr; u.ssrc[0] = 0; u.rows[0] = v.NI; u.dst[0] = c->d_preW; u.sdst[0] = (long long)v.NI * v.NI;
            u.src[1] = v.preU; u.ssrc[1] = (long long)v.NK * v.NI; u.rows[1] = v.NK; u.dst[1] = c->d_preT; u.sdst[1] = (long long)v.NK * v.NI;
            hipLaunchKernelGGL(k_cov_tri, dim3(v.S, 2), dim3(128), COV_TRI_LDS(v.NI, std::max(v.NI, v.NK)), st, u);
        }
    }
    CovBufs w;
    w.W = c->d_W; w.Ta = c->d_Ta; w.Tb = c->d_Tb; w.Sd = c->d_Sd; w.XL = c->d_XL; w.XR = c->d_XR;
    w.preW = c->d_preW; w.preT = c->d_preT; w.Sik = c->d_Sik; w.Sii = c->d_Sii; w.bcr_fail = v.fail; w.st = c->d_st;
    // ---- down the tree, the last level first
    for (int l = v.levels - 1; l >= 0; --l) {
        const int ne = c->elim_off[l + 1] - c->elim_off[l];
        if (ne > 0) hipLaunchKernelGGL(k_cov_down, dim3(ne), dim3(COV_TH), COV_DOWN_LDS(M), st, w, c->d_tab + c->elim_off[l], M);
    }
    if (v.pre) hipLaunchKernelGGL(k_cov_pre, dim3(v.S), dim3(COV_TH), COV_DOWN_LDS(COV_MAX), st, w, v.NI, v.NK);
    hipLaunchKernelGGL(k_cov_status, dim3(1), dim3(256), 0, st, v.L, v.nnode, M, v.pre ? v.preL : nullptr, v.S, v.NI, v.fail, c->d_st);
    GLIO_HIP_CHECK(hipEventRecord(c->ev[3], st));
    // ---- gather, unscaled
    CovGather g;
    g.K = K; g.B = B; g.M = M; g.sbk = v.sbk; g.pre = v.pre; g.NI = v.NI; g.NK = v.NK; g.anchor = anchor_keyframe; g.level = c->d_level; g.sc = c->d_sc;
    g.diag = c->d_out; g.next = next ? c->d_out + (size_t)K * BB : nullptr;
    hipLaunchKernelGGL(k_cov_gather, dim3(K), dim3(256), 0, st, w, g);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(c->ev[4], st));
    const size_t want = (size_t)K * BB + (next ? (size_t)(K - 1) * BB : 0);
    CovStatus* h_st = reinterpret_cast<CovStatus*>(c->h_out + c->out_doubles);
    GLIO_HIP_CHECK(hipMemcpyAsync(h_st, c->d_st, sizeof(CovStatus), hipMemcpyDeviceToHost, st));
    GLIO_HIP_CHECK(hipMemcpyAsync(c->h_out, c->d_out, want * 8, hipMemcpyDeviceToHost, st));
    GLIO_HIP_CHECK(hipEventRecord(c->ev[5], st));
    GLIO_HIP_CHECK(hipStreamSynchronize(st));          // the one host wait
    c->timed = true;
    const CovStatus s = *h_st;
    int bad = -1;
    if (s.sbad) bad = s.skf;
    else if (s.fail) {
        if (s.ord < BCR_ORD_NODE) bad = s.ord * v.sbk;
        else if (s.ord - BCR_ORD_NODE < (int)c->node_of_ord.size()) bad = c->node_of_ord[s.ord - BCR_ORD_NODE] * v.sbk;
        else bad = 0;
        bad = std::min(bad, K - 1);
    }
    if (info) {
        info->n = n; info->B = B; info->anchor = anchor_keyframe; info->bad_keyframe = bad; info->levels = v.levels; info->pad_ = 0;
        info->min_pivot = s.minp; info->max_pivot = s.maxp;
    }
    if (bad >= 0) { glio_set_error("batch covariance: H is not positive definite (keyframe %d); without GNSS factors an anchor keyframe is needed", bad); return GLIO_E_NUMERIC; }
    memcpy(diag, c->h_out, (size_t)K * BB * 8);
    if (next) memcpy(next, c->h_out + (size_t)K * BB, (size_t)(K - 1) * BB * 8);
    return GLIO_OK;
}

int glio_batch_covariance_last_stage_ms(glio_batch* b, float* ms5) {
    if (!b || !ms5) return GLIO_E_ARG;
    if (!b->cov || !b->cov->timed) return GLIO_E_STATE;
    for (int k = 0; k < 5; ++k) GLIO_HIP_CHECK(hipEventElapsedTime(&ms5[k], b->cov->ev[k], b->cov->ev[k + 1]));
    return GLIO_OK;
}
int glio_batch_covariance_last_device_ms(glio_batch* b, float* ms) {
    if (!b || !ms) return GLIO_E_ARG;
    if (!b->cov || !b->cov->timed) return GLIO_E_STATE;
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, b->cov->ev[0], b->cov->ev[5]));
    return GLIO_OK;
}

}  // extern "C"

// batch_solve_kernels.hip -- the damped block-banded solve of the batch problem by BLOCK CYCLIC REDUCTION, parallel over the
// chip and -- round 3 -- over the RANKS of the sharded stage (Estimator::optimizeBatchWithLandMark's normal equations,
// reference GLIO/src/Estimator.cpp:3004-3076,3275-3284: there Ceres' SPARSE_NORMAL_CHOLESKY on one thread).
//
// Unknowns: B per keyframe (6: pose only; 15: pose + speed/bias with the ImuFactor chain, Estimator.cpp:2809-2819,2990-3001).
// The K keyframes are grouped into S = ceil(K / sbk) SUPER-BLOCKS of sbk >= band keyframes (M = sbk B unknowns: 36 / 72 for the
// pose problem with band <= 6 / 12, 90 with the IMU chain): in that blocking the matrix is block TRIDIAGONAL with dense M x M
// blocks.  Odd-even (nested-dissection) elimination: a level eliminates every other active node -- all at once, one workgroup
// each -- then the kept nodes take their Schur updates; ceil(log2 S) + 1 levels.  Exact Cholesky in that order (SPD, no pivoting).
//
// Sharded (world > 1): rank r owns the super-blocks [S r / world, S (r+1) / world); its LAST super-block is a SEPARATOR (ranks
// 0 .. world-2).  A rank eliminates its interior super-blocks with the separators at either end pinned: what remains are Schur
// updates of the (at most two) adjacent separators and the coupling between them -- written into `sepbuf`, which the caller
// all-reduces (every rank then holds the same (world-1)-node separator system, ~ 3 (world-1) M^2 doubles), every rank solves
// that small chain redundantly (same kernels, "top" schedule) and substitutes back through its own levels.  One collective
// per solve, no other exchange.  world = 1 is the same code with no separators and no collective.
//
//   k_bcr_init    super-blocks D_s, couplings A[s+1][s] and right-hand sides of the OWNED rows from the operator
//                 S (H_pose_band + H_imu_chain) S + shift, S g    (scaling and shift applied on the fly, no scaled copy)
//   k_bcr_elim    node p with active neighbours a < p < b: the (3M+1) x M panel [A_pp; A_ap; A_bp; y_p^T] one row per lane,
//                 factored in M register steps with ONE workgroup barrier each (double-buffered column through LDS)
//   k_bcr_update  kept node q: A_qq -= U U^T of its eliminated neighbours, y_q -= U w, new coupling A[b][a] = -U_b U_a^T
//                 (v_mfma_f64_16x16x4 tiles over LDS-staged factors)
//   k_bcr_back    z_p = L^-T (w - U_a^T z_a - U_b^T z_b): the triangular solve inside one wavefront (no barriers)
// Every sum has a fixed order: two runs are bit-identical.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "batch_device.h"

// (BcrElim: batch_device.h -- blocks in the workspace; a / b: neighbour nodes (-1: none))
struct BcrKept { int node, pl, pr, pad_; long long oD, oy, oCnew; };    // eliminated neighbours left / right (-1), new edge (-1: none)
struct BcrInit { int sblock, pad_; long long oD, oy, oC; };             // global super-block; where D, y, A[sblock+1][sblock] go (-1: not wanted)

struct BcrDev {
    int M, sbk, S, K, band, B, rank, world;
    int Slo, Shi, nint, NS, nnode;           // owned super-blocks, interior nodes, separators, nodes with factors (nint + NS)
    int levels_loc, levels_top;
    double* ws;              // D / C / y blocks of the interior nodes and local edges, then sepbuf
    long long ws_doubles, sep_off, sep_doubles;   // sepbuf = [Dsep NS M^2 | Csep (NS-1) M^2 | ysep NS M | 16 extra scalars]
    double* L; double* Ua; double* Ub;       // [nnode][M*M]
    double* w; double* z;                    // [nnode][M]
    BcrElim* elim; BcrKept* kept; BcrInit* init;
    int n_init;
    std::vector<int> h_elim_off, h_kept_off;       // per level [levels_loc + levels_top + 1]
    std::vector<BcrElim> h_elim;                   // the schedule as uploaded (BcrView)
    std::vector<int> node_of_sblock;               // owned super-block (global index - Slo) -> node id
    int* node_of_sblock_dev;
    int* fail;
    // with the IMU chain (B = 15): the speed-bias blocks of the four INNER keyframes of every super-block touch nothing outside their
    // super-block, so they are eliminated before the reduction (k_bcr_pre) and recovered after it (k_bcr_post): the reduction then
    // runs on 54 x 54 blocks (6 poses + the speed-bias blocks of the first and the last keyframe) instead of 90 x 90
    bool pre;
    double* preL; double* preU; double* prew;      // per owned super-block: L [36][36], U = A_ki L^-T [54][36], w = L^-1 y_i [36]
};

// ------------------------------------------------------------------------------------------------ the operator (HView / h_entry: batch_device.h)
__device__ __forceinline__ HView bcr_view(const BcrOp& op, const int K, const int band, const int B) {
    const int cur = op.cur ? *op.cur : 0;
    HView v;
    v.Hg = op.Hg[cur]; v.imu = op.imu[cur]; v.K = K; v.band = band; v.B = B;
    return v;
}

#define BCR_INIT_SPLIT 8
__global__ __launch_bounds__(256) void k_bcr_init(const BcrOp op, const BcrInit* __restrict__ tab, const int K, const int band, const int B, const int M,
                                                  const int sbk, double* __restrict__ ws) {
    if (op.skip && *op.skip) return;
    const BcrInit t = tab[blockIdx.x];
    const HView v = bcr_view(op, K, band, B);
    const int cur = op.cur ? *op.cur : 0;
    const double* gsrc = op.gfull[cur];
    const int s = t.sblock;
    constexpr int U = 4;
    // BCR_INIT_SPLIT workgroups per super-block (blockIdx.y), each a contiguous slice of the M x M entries: the kernel is a gather of
    // dependent loads, so what it needs is wavefronts in flight, not bandwidth
    const int per = (M * M + BCR_INIT_SPLIT - 1) / BCR_INIT_SPLIT, eb = blockIdx.y * per, ee_end = min(M * M, eb + per);
    for (int e0 = eb + threadIdx.x; e0 < ee_end; e0 += U * 256) {          // four entries of either block in flight per thread
        double xd[U], xc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256;
            const int ee = e < ee_end ? e : 0;
            const int i = ee / M, j = ee - M * i;
            const int ka = s * sbk + i / B, r = i % B, kb = s * sbk + j / B, c = j % B;
            xd[u] = 0.0; xc[u] = 0.0;
            if (t.oD >= 0) {
                double x = h_entry(v, ka, r, kb, c);
                if (ka < K && kb < K && op.sc) x *= op.sc[(size_t)ka * B + r] * op.sc[(size_t)kb * B + c];
                if (i == j && ka < K) x += op.dadd ? op.dadd[(size_t)ka * B + r] : op.lambda * x + 1e-12;
                xd[u] = x;
            }
            if (t.oC >= 0) {          // A[s+1][s]: rows in super-block s+1, columns in s
                const int kr = (s + 1) * sbk + i / B;
                if (kr < K && kb < K) {
                    double x = h_entry(v, kr, r, kb, c);
                    if (op.sc) x *= op.sc[(size_t)kr * B + r] * op.sc[(size_t)kb * B + c];
                    xc[u] = x;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256;
            if (e >= ee_end) continue;
            if (t.oD >= 0) ws[t.oD + e] = xd[u];
            if (t.oC >= 0) ws[t.oC + e] = xc[u];
        }
    }
    if (t.oy >= 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < M; i += 256) {
            const int k = s * sbk + i / B, r = i % B;
            double x = 0.0;
            if (k < K) {
                x = gsrc ? gsrc[(size_t)k * B + r] : v.Hg[(size_t)K * (band + 1) * 36 + (size_t)k * 6 + r];
                if (op.sc) x *= op.sc[(size_t)k * B + r];
            }
            ws[t.oy + i] = x;
        }
}

#ifdef GLIO_DEV_STAMPS
__device__ long long g_bcr_stamps[8];      // elim2, workgroup 0: [0] load, [1] register steps, [2] MFMA updates, [3] store (100 MHz ticks, last launch)
#define BCR_T(var) const long long var = wall_clock64()
#define BCR_ACC(k, t1, t0) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_bcr_stamps[k] += (t1) - (t0); } while (0)
#else
#define BCR_T(var) do { } while (0)
#define BCR_ACC(k, t1, t0) do { } while (0)
#endif
// ------------------------------------------------------------------------------------------------ the register-step panel factorisation
// N register steps over a panel of N columns, one row per lane (a = the lane's row; rows 0..N-1 the diagonal block, the rows below are solved
// against it): the (unscaled) column j of the diagonal block goes through the double-buffered LDS row col[2][N], ONE workgroup barrier per
// pivot.  ROWS: the rows of the panel (lanes past them idle); 0 = every launched lane is a row (k_bcr_elim launches BcrCfg<M>::THREADS lanes
// and guards only row >= j).  Ends with a barrier.  Used by k_bcr_elim<M>, k_bcr_pre and k_bcr_pre12.
template <int N, int ROWS>
__device__ __forceinline__ void bcr_register_steps(double (&a)[N], const int row, double (*col)[N], int* s_bad) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (row >= j && row < N) col[j & 1][row] = a[j];
        __syncthreads();
        const double piv = col[j & 1][j];
        double rd;
        if (!(piv > 0.0) || !isfinite(piv)) { rd = 1.0; if (row == j) *s_bad = 1; } else rd = rsqrt(piv);
        if (row >= j && (ROWS == 0 || row < ROWS)) {
            const double lj = a[j] * rd;
            a[j] = lj;
            if (row > j) {
#pragma unroll
                for (int c = j + 1; c < N; ++c) a[c] -= lj * (col[j & 1][c] * rd);
            }
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ pre-elimination of the inner speed-bias blocks
// A super-block of 6 keyframes x 15 unknowns.  KEPT (54): keyframe 0 whole (15), the poses of keyframes 1..4 (4 x 6), keyframe 5 whole (15)
// -- everything that couples to another super-block (the pose band reaches +-6 keyframes, the IMU edge 5 -> 0' the neighbour's first
// keyframe).  INNER (36): the speed-bias blocks of keyframes 1..4, a 4-block chain coupled to the poses and speed-bias blocks of this
// super-block only.  k_bcr_pre forms, from the operator, [A_ii; A_ki; y_i^T] (91 rows x 36), factors it in 36 register steps (one row
// per lane, one barrier per pivot, as k_bcr_elim) and writes the Schur complement A_kk - U U^T, y_k - U w as the super-block's 54 x 54
// node; k_bcr_post recovers z_i = L^-T (w - U^T z_k) and writes the step of the super-block's keyframes.
//
// The same for bands 7..12 (round 4).  The reference gives the first and the last search_range keyframes of a batch a window of
// +-2 search_range (Estimator.cpp:3009-3017): with the ImuFactor chain that is 15 unknowns per keyframe under a pose band of 12.
// Super-blocks of 12 keyframes then (180 unknowns); KEPT (90): keyframe 0 whole, the poses of keyframes 1..10, keyframe 11 whole -- all that
// reaches another super-block -- INNER (90): the speed-bias blocks of keyframes 1..10.  The reduction runs on the same 90 x 90 nodes as
// the un-reduced band-6 problem would (k_bcr_pre12 / k_bcr_post12).
//
// BcrPre<SBK> is the shape of either; what the two kernel pairs share takes it as its parameter.  What they do NOT share, on purpose:
//   - k_bcr_pre gathers its panel SOURCE-major into LDS (coalesced band rows and edge records, A_kk beside the panel in `dk`); k_bcr_pre12,
//     the rare shape (two windows per batch want it), gathers entry by entry through bcr_scaled_entry and reads A_kk from the operator
//     when the Schur complement is formed: its panel alone takes 134.7 KB of LDS, there is no room for A_kk, and the entry-major form was
//     what k_bcr_pre replaced because it was bound by the L1's address path (comment at its gather).
//   - k_bcr_post substitutes back inside one wavefront (36 unknowns: v_readlane, no barrier); k_bcr_post12 has 90 unknowns on two
//     wavefronts and takes two barriers per column.
//   - h_entry (batch_device.h, k_bcr_init) branches on the data; bcr_scaled_entry is its branch-free restatement for the gathers
//     where every thread takes many entries (1.3 us per entry per thread with the branches, measured: comment at bcr_scaled_entry).
typedef double v4f64 __attribute__((ext_vector_type(4)));
template <int SBK> struct BcrPre {
    static constexpr int B = 15, NI = 9 * (SBK - 2), NP = 6 * (SBK - 2), NK = NP + 2 * B, ROWS = NI + NK + 1;
    // row stride of the panel [A_ii; A_ki; y_i^T]: NI + 1 where NI is a multiple of 4, else up to the next multiple of 4 and one more -- the
    // MFMA loop reads k in fours, the columns past NI are zero
    static constexpr int KP = ((NI + 3) / 4) * 4, LDP = KP + 1;
    // kept unknown i -> keyframe of the super-block, unknown of the keyframe; inner unknown p likewise; and back
    static __device__ __forceinline__ void kept(const int i, int& kl, int& r) {
        if (i < B) { kl = 0; r = i; } else if (i < B + NP) { kl = 1 + (i - B) / 6; r = (i - B) % 6; } else { kl = SBK - 1; r = i - (B + NP); }
    }
    static __device__ __forceinline__ void inner(const int p, int& kl, int& r) { kl = 1 + p / 9; r = 6 + p % 9; }
    static __device__ __forceinline__ int kept_of(const int kl, const int r) { return kl == 0 ? r : (kl == SBK - 1 ? B + NP + r : B + (kl - 1) * 6 + r); }
};
static_assert(BcrPre<6>::NI == 36 && BcrPre<6>::NK == 54 && BcrPre<6>::LDP == 37, "the 6-keyframe super-block");
static_assert(BcrPre<12>::NI == 90 && BcrPre<12>::NK == 90 && BcrPre<12>::LDP == 93, "the 12-keyframe super-block");
// S (H_band + H_imu) S + shift, entry (r, c) of block (ka, kb) -- the value of h_entry (batch_device.h) with scale and shift, written WITHOUT
// data-dependent branches: every load goes to a clamped address and is selected afterwards, so the entries a thread gathers are independent
// loads the hardware overlaps (with the branches of h_entry each entry cost a full memory round trip: 1.3 us per entry per thread, measured)
__device__ __forceinline__ double bcr_scaled_entry(const BcrOp& op, const HView& v, const int K, const int B, const int ka, const int r, const int kb, const int c) {
    const bool in = ka < K && kb < K;
    const int kac = ka < K ? ka : K - 1, kbc = kb < K ? kb : K - 1;
    const int d = kbc - kac, bw = v.band + 1;
    // pose band
    const bool hasb = in && r < 6 && c < 6 && d <= v.band && d >= -v.band;
    const int rb = r < 6 ? r : 0, cb = c < 6 ? c : 0, dd = d > v.band ? v.band : (d < -v.band ? -v.band : d);
    const size_t ib = dd >= 0 ? ((size_t)kac * bw + dd) * 36 + rb * 6 + cb : ((size_t)kbc * bw + (-dd)) * 36 + cb * 6 + rb;
    const double xb = hasb ? v.Hg[ib] : 0.0;           // (lane-predicated: a masked lane issues no request -- most entries have no band part)
    // IMU chain: edge e1 holds (ka, kb) for |d| <= 1; the diagonal block takes a second share from the edge arriving at ka
    double x1 = 0.0, x2 = 0.0;
    bool has1 = false, has2 = false;
    if (v.imu) {
        const int e1 = d == -1 ? kbc : kac, e1c = e1 < K - 1 ? e1 : (K >= 2 ? K - 2 : 0);
        const int o1 = d == 0 ? r * 30 + c : (d == 1 ? r * 30 + 15 + c : (15 + r) * 30 + c);
        has1 = in && d >= -1 && d <= 1 && e1 < K - 1;
        has2 = in && d == 0 && kac > 0;
        const int e2c = kac > 0 ? kac - 1 : 0;
        x1 = has1 ? v.imu[e1c].H[o1] : 0.0;
        x2 = has2 ? v.imu[e2c < K - 1 ? e2c : 0].H[(15 + r) * 30 + 15 + c] : 0.0;
    }
    const double sa = op.sc ? op.sc[(size_t)kac * B + r] : 1.0, sb = op.sc ? op.sc[(size_t)kbc * B + c] : 1.0;
    const double da = (op.dadd && in && ka == kb && r == c) ? op.dadd[(size_t)kac * B + r] : 0.0;
    double x = xb + x1 + x2;
    if (!in) return (ka == kb && r == c) ? 1.0 : 0.0;           // identity padding of the last super-block
    x *= sa * sb;
    if (ka == kb && r == c) x += op.dadd ? da : op.lambda * x + 1e-12;
    return x;
}
// the coupling A[s+1][s] between the KEPT unknowns of neighbouring super-blocks (the inner blocks do not reach the neighbour): a gather,
// two workgroups (blockIdx.y = 1, 2), eight entries in flight per thread
template <int SBK>
__device__ __forceinline__ void bcr_pre_coupling(const BcrOp& op, const HView& v, const int K, const int k0, double* __restrict__ dst) {
    using P = BcrPre<SBK>;
    constexpr int B = P::B, NK = P::NK, U = 8;
    const int tid = threadIdx.x;
    const int half = (NK * NK + 1) / 2, eb = (blockIdx.y - 1) * half, ee = min(NK * NK, eb + half);
    for (int e0 = eb + tid; e0 < ee; e0 += U * 256) {
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256, eo = e < ee ? e : eb;
            int kli, ri, klj, cj;
            P::kept(eo / NK, kli, ri); P::kept(eo % NK, klj, cj);
            x[u] = bcr_scaled_entry(op, v, K, B, k0 + SBK + kli, ri, k0 + klj, cj);          // (zero when either keyframe is padding: different blocks)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { const int e = e0 + u * 256; if (e < ee) dst[e] = x[u]; }
    }
}
// the finished panel in LDS ([A_ii; A_ki; y_i^T], one row per lane) -> NI register steps -> [L (zeros above the diagonal); U; w] back in the
// panel; a non-positive or non-finite pivot raises bit 0 of *fail
template <int SBK>
__device__ __forceinline__ void bcr_pre_factor(double* __restrict__ pan, double (*col)[BcrPre<SBK>::NI], int* s_bad, int* fail) {
    using P = BcrPre<SBK>;
    constexpr int NI = P::NI, ROWS = P::ROWS, LDP = P::LDP;
    const int row = threadIdx.x;
    double a[NI];
#pragma unroll
    for (int c = 0; c < NI; ++c) a[c] = row < ROWS ? pan[row * LDP + c] : 0.0;
    bcr_register_steps<NI, ROWS>(a, row, col, s_bad);
    if (row < ROWS) {
#pragma unroll
        for (int c = 0; c < NI; ++c) pan[row * LDP + c] = (row < NI && c > row) ? 0.0 : a[c];
    }
    if (row == 0 && *s_bad) { atomicOr(fail, 1); atomicMin(fail + 1, (int)blockIdx.x); }
    __syncthreads();
}
// from the factored panel: L, U, w out (coalesced); the super-block's node A_kk - U U^T on the matrix core -- T x T tiles of 16 x 16 over the four
// wavefronts, the old block (akk(r, c), r and c inside the block) as the accumulator's initial value -- and its right-hand side yk - U w
template <int SBK, class Akk>
__device__ __forceinline__ void bcr_pre_schur(const double* __restrict__ pan, const size_t sb, double* __restrict__ preL, double* __restrict__ preU,
                                              double* __restrict__ prew, double* __restrict__ D, double* __restrict__ y, const double yk, const Akk akk) {
    using P = BcrPre<SBK>;
    constexpr int NI = P::NI, NK = P::NK, LDP = P::LDP, T = (NK + 15) / 16;
    const int tid = threadIdx.x;
    for (int e = tid; e < NI * NI; e += 256) preL[sb * NI * NI + e] = pan[(e / NI) * LDP + e % NI];
    for (int e = tid; e < NK * NI; e += 256) preU[sb * NK * NI + e] = pan[(NI + e / NI) * LDP + e % NI];
    if (tid < NI) prew[sb * NI + tid] = pan[(NI + NK) * LDP + tid];
    const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    for (int tile = wave; tile < T * T; tile += 4) {
        const int I = tile / T, J = tile - T * I;
        v4f64 c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * I + lk + 4 * q, cc = 16 * J + li;
            const double x = akk(r < NK ? r : 0, cc < NK ? cc : 0);
            c[q] = (r < NK && cc < NK) ? x : 0.0;
        }
        const int ra = 16 * I + li, rb = 16 * J + li;
        const double* pa = pan + (NI + (ra < NK ? ra : 0)) * LDP + lk;
        const double* pb = pan + (NI + (rb < NK ? rb : 0)) * LDP + lk;
#pragma unroll
        for (int kk = 0; kk < P::KP; kk += 4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(ra < NK ? -pa[kk] : 0.0, rb < NK ? pb[kk] : 0.0, c, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) { const int r = 16 * I + lk + 4 * q, cc = 16 * J + li; if (r < NK && cc < NK) D[r * NK + cc] = c[q]; }
    }
    if (y && tid < NK) {
        const double* ui = pan + (NI + tid) * LDP; const double* wv = pan + (NI + NK) * LDP;
        double s0 = 0;
#pragma unroll 6
        for (int c = 0; c < NI; ++c) s0 += ui[c] * wv[c];
        y[tid] = yk - s0;
    }
}
__global__ __launch_bounds__(256) void k_bcr_pre(const BcrOp op, const BcrInit* __restrict__ tab, const int K, const int band, const int Slo, double* __restrict__ ws,
                                                 double* __restrict__ preL, double* __restrict__ preU, double* __restrict__ prew, int* fail) {
    if (op.skip && *op.skip) return;
    using P = BcrPre<6>;
    constexpr int B = P::B, NI = P::NI, NK = P::NK, LDP = P::LDP, PRE_ROWS = P::ROWS;
    __shared__ double pan[PRE_ROWS * LDP];         // [A_ii; A_ki; y_i] rows of 36 (+1 pad), later U (rows 36..89) and w (row 90)
    __shared__ double dk[NK * NK + NK];            // A_kk, y_k
    __shared__ double col[2][NI];
    __shared__ int s_bad;
    const BcrInit t = tab[blockIdx.x];
    const HView v = bcr_view(op, K, band, B);
    const int cur = op.cur ? *op.cur : 0;
    const double* gsrc = op.gfull[cur];
    const int s = t.sblock, k0 = s * 6, tid = threadIdx.x;
    constexpr int U = 8;
    if (blockIdx.y > 0) {
        if (t.oC >= 0) bcr_pre_coupling<6>(op, v, K, k0, ws + t.oC);
        return;
    }
    if (t.oD < 0) return;
    if (tid == 0) s_bad = 0;
#ifdef GLIO_DEV_STAMPS
    if (blockIdx.x == 0 && tid == 0) { g_bcr_stamps[4] = g_bcr_stamps[5] = g_bcr_stamps[6] = 0; }
#endif
    BCR_T(tq0);
    // ---- gather, SOURCE-major: the band rows of the super-block's six keyframes (1512 doubles) and its IMU edge records (900 each) are
    // read as they lie in memory (coalesced: the entry-major form touched 21 cache lines per load instruction and was bound by the L1's
    // address path) and scattered into the LDS panel.  An entry is band + own edge + previous edge, in that order (h_entry): the three
    // sources are three passes with a barrier between them, each writing a cell at most once.  Mixed cells (kept row, inner column) exist
    // once: they take the source entry of that orientation.  Scale, shift and the identity padding follow in a pass over the panel.
    __shared__ double scl[90], dad[90], gsc[90];
    {
        for (int e = tid; e < PRE_ROWS * LDP; e += 256) pan[e] = 0.0;
        for (int e = tid; e < NK * NK + NK; e += 256) dk[e] = 0.0;
        if (tid < 90) {
            const int k = k0 + tid / B, r = tid % B, kc = k < K ? k : K - 1;
            const double sv = op.sc ? op.sc[(size_t)kc * B + r] : 1.0;
            scl[tid] = k < K ? sv : 1.0;
            dad[tid] = (op.dadd && k < K) ? op.dadd[(size_t)kc * B + r] : 0.0;
            gsc[tid] = k < K ? gsrc[(size_t)kc * B + r] * sv : 0.0;
        }
    }
    __syncthreads();
    auto cell = [&](const int u, const int vv) -> double* {          // the LDS cell of entry (row unknown u, column unknown vv), or null
        const int klu = u / B, ru = u - B * klu, klv = vv / B, rv = vv - B * klv;
        const bool iu = klu >= 1 && klu <= 4 && ru >= 6, iv = klv >= 1 && klv <= 4 && rv >= 6;
        const int pu = (klu - 1) * 9 + ru - 6, pv = (klv - 1) * 9 + rv - 6;
        const int ku = klu == 0 ? ru : (klu == 5 ? 39 + ru : 15 + (klu - 1) * 6 + ru), kv = klv == 0 ? rv : (klv == 5 ? 39 + rv : 15 + (klv - 1) * 6 + rv);
        if (iv) return pan + (iu ? pu : NI + ku) * LDP + pv;          // inner column: panel row = inner or kept row
        if (iu) return nullptr;                                        // (inner row, kept column): the cell of the other orientation
        return dk + ku * NK + kv;
    };
    {   // pass 1: band.  t -> keyframe kl, block d, entry (r, c): H(k0 + kl, r | k0 + kl + d, c); both orientations for d > 0
        const int bw = band + 1, per = bw * 36;
        for (int t0 = tid; t0 < 6 * per; t0 += U * 256) {
            double x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256, kl = t / per, ka = k0 + kl, d = (t - per * kl) / 36;
                x[u] = (t < 6 * per && ka < K && ka + d < K) ? v.Hg[(size_t)ka * per + (t - per * kl)] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256;
                if (t >= 6 * per) continue;
                const int kl = t / per, q = t - per * kl, d = q / 36, r = (q % 36) / 6, c = q % 6;
                if (kl + d > 5) continue;
                *cell(kl * B + r, (kl + d) * B + c) = x[u];
                if (d > 0) *cell((kl + d) * B + c, kl * B + r) = x[u];
            }
        }
    }
    __syncthreads();
    if (v.imu) {
        // pass 2: edge (a, a + 1), a = k0 + kl: rows 0..14 of its record = [own diagonal part of a | block (a, a + 1)]; rows 15..29, columns
        // 0..14 = block (a + 1, a).  (kl = 5: only the diagonal part lies in this super-block.)
        for (int t0 = tid; t0 < 6 * 675; t0 += U * 256) {
            double x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256, kl = t / 675, q = t - 675 * kl, ka = k0 + kl;
                // q < 450: row q / 30, column q % 30 of the record; q >= 450: row 15 + (q - 450) / 15, column (q - 450) % 15
                const int o = q < 450 ? q : 450 + ((q - 450) / 15) * 30 + (q - 450) % 15;
                x[u] = (t < 6 * 675 && ka < K - 1) ? v.imu[ka].H[o] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256;
                if (t >= 6 * 675) continue;
                const int kl = t / 675, q = t - 675 * kl;
                int ur, uc;
                if (q < 450) { const int r = q / 30, c = q - 30 * r; ur = kl * B + r; uc = c < 15 ? kl * B + c : (kl + 1) * B + c - 15; }
                else { const int r = (q - 450) / 15, c = (q - 450) - 15 * r; ur = (kl + 1) * B + r; uc = kl * B + c; }
                if (ur >= 90 || uc >= 90) continue;                     // the part of edge 5 that belongs to the next super-block
                double* cl = cell(ur, uc);
                if (cl) *cl += x[u];
            }
        }
        __syncthreads();
        // pass 3: edge (a - 1, a), a = k0 + kl: rows 15..29, columns 15..29 of its record = the previous edge's share of a's diagonal block
        for (int t0 = tid; t0 < 6 * 225; t0 += U * 256) {
            double x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256, kl = t / 225, q = t - 225 * kl, ka = k0 + kl;
                x[u] = (t < 6 * 225 && ka >= 1 && ka < K) ? v.imu[ka - 1].H[(15 + q / 15) * 30 + 15 + q % 15] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + u * 256;
                if (t >= 6 * 225) continue;
                const int kl = t / 225, q = t - 225 * kl;
                double* cl = cell(kl * B + q / 15, kl * B + q % 15);
                if (cl) *cl += x[u];
            }
        }
    }
    __syncthreads();
    {   // pass 4: scale, shift, identity padding, right-hand sides
        auto u_inner = [&](const int pp) { return (1 + pp / 9) * B + 6 + pp % 9; };
        auto u_kept = [&](const int i) { int kl, r; P::kept(i, kl, r); return kl * B + r; };
        auto finish = [&](double& cellv, const int ur, const int uc) {
            const bool pad = k0 + ur / B >= K || k0 + uc / B >= K;
            double x = cellv * (scl[ur] * scl[uc]);
            if (ur == uc) x += op.dadd ? dad[ur] : op.lambda * x + 1e-12;
            cellv = pad ? (ur == uc ? 1.0 : 0.0) : x;
        };
        for (int e = tid; e < (NI + NK) * NI; e += 256) {
            const int row = e / NI, c = e - NI * row;
            finish(pan[row * LDP + c], row < NI ? u_inner(row) : u_kept(row - NI), u_inner(c));
        }
        for (int e = tid; e < NK * NK; e += 256) { const int i = e / NK, j = e - NK * i; finish(dk[e], u_kept(i), u_kept(j)); }
        if (tid < NI) pan[(NI + NK) * LDP + tid] = gsc[u_inner(tid)];
        if (tid >= 64 && tid < 64 + NK) dk[NK * NK + tid - 64] = gsc[u_kept(tid - 64)];
    }
    __syncthreads();
    BCR_T(tq1);
    BCR_ACC(4, tq1, tq0);
    // ---- 36 register steps, one row per lane (rows 0..35 the inner block, 36..89 the kept rows, 90 the right-hand side)
    bcr_pre_factor<6>(pan, col, &s_bad, fail);
    BCR_T(tq2);
    BCR_ACC(5, tq2, tq1);
    // factors out, Schur complement (A_kk from its LDS copy) and right-hand side of the kept unknowns
    bcr_pre_schur<6>(pan, (size_t)(s - Slo), preL, preU, prew, ws + t.oD, t.oy >= 0 ? ws + t.oy : nullptr, tid < NK ? dk[NK * NK + tid] : 0.0,
                     [&](const int r, const int c) { return dk[r * NK + c]; });
#ifdef GLIO_DEV_STAMPS
    __syncthreads();
    { BCR_T(tq3); BCR_ACC(6, tq3, tq2); }
#endif
}
// entry `i` of t = w - U^T z_k of super-block sb (i < NI): the column of U is eighteen independent global loads at a time, the sum keeps three
// interleaved chains
template <int SBK>
__device__ __forceinline__ double bcr_post_rhs(const double* __restrict__ preU, const double* __restrict__ prew, const double* __restrict__ zk, const int sb, const int i) {
    using P = BcrPre<SBK>;
    constexpr int NI = P::NI, NK = P::NK;
    static_assert(NK % 18 == 0, "chunk of the U^T z sums");
    const double* Uc = preU + (size_t)sb * NK * NI + i;
    double p3[3] = {0, 0, 0};
#pragma unroll
    for (int i0 = 0; i0 < NK; i0 += 18) {
        double uv[18];
#pragma unroll
        for (int u = 0; u < 18; ++u) uv[u] = Uc[(size_t)(i0 + u) * NI];
#pragma unroll
        for (int u = 0; u < 18; ++u) p3[u % 3] += uv[u] * zk[i0 + u];
    }
    return prew[(size_t)sb * NI + i] - ((p3[0] + p3[1]) + p3[2]);
}
// the step of the super-block's keyframes: delta = -z, the inner unknowns from zi, the kept ones from the node's solution zk; a non-finite
// entry raises bit 1 of *fail
template <int SBK>
__device__ __forceinline__ void bcr_post_scatter(const double* __restrict__ zi, const double* __restrict__ zk, const int k0, const int K, const int nthreads,
                                                 double* __restrict__ delta, int* fail) {
    using P = BcrPre<SBK>;
    constexpr int B = P::B;
    for (int e = threadIdx.x; e < SBK * B; e += nthreads) {
        const int kl = e / B, r = e - B * kl, k = k0 + kl;
        if (k >= K) continue;
        double val;
        if (r >= 6 && kl >= 1 && kl <= SBK - 2) val = zi[(kl - 1) * 9 + r - 6];
        else val = zk[P::kept_of(kl, r)];
        val = -val;
        if (!isfinite(val)) atomicOr(fail, 2);
        delta[(size_t)k * B + r] = val;
    }
}
// z_i = L^-T (w - U^T z_k) of one owned super-block, then the step of its keyframes: delta = -z (kept unknowns from the node's solution)
__global__ __launch_bounds__(64) void k_bcr_post(const int* skip, const double* __restrict__ z, const int* __restrict__ node_of, const int Slo, const int K,
                                                 const double* __restrict__ preL, const double* __restrict__ preU, const double* __restrict__ prew,
                                                 double* __restrict__ delta, int* fail) {
    if (skip && *skip) return;
    constexpr int NI = BcrPre<6>::NI, NK = BcrPre<6>::NK, LDL = NI + 1;
    __shared__ double Ls[NI * LDL], zk[NK], rd[NI], zi[NI];
    const int sb = blockIdx.x, lane = threadIdx.x, s = Slo + sb, k0 = s * 6;
    const int node = node_of[sb];
    if (lane < NK) zk[lane] = z[(size_t)node * NK + lane];
    for (int e0 = lane; e0 < NI * NI; e0 += 8 * 64) {
        double v8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * 64; v8[u] = e < NI * NI ? preL[(size_t)sb * NI * NI + e] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * 64; if (e < NI * NI) Ls[(e / NI) * LDL + e % NI] = v8[u]; }
    }
    __syncthreads();
    double t = 0.0;
    if (lane < NI) {
        rd[lane] = 1.0 / Ls[lane * LDL + lane];
        t = bcr_post_rhs<6>(preU, prew, zk, sb, lane);
    }
    __syncthreads();
#pragma unroll
    for (int r = NI - 1; r >= 0; --r) {
        const double zr = readlane_d(t, r) * rd[r];
        if (lane == r) t = zr;
        if (lane < r) t -= Ls[r * LDL + lane] * zr;
    }
    if (lane < NI) zi[lane] = t;
    __syncthreads();
    bcr_post_scatter<6>(zi, zk, k0, K, 64, delta, fail);
}

// ------------------------------------------------------------------------------------------------ the same for bands 7..12 (BcrPre<12>, above)
// The panel is gathered entry by entry through bcr_scaled_entry and lives in LDS ([A_ii; A_ki; y_i^T], 181 rows of 90 + 3 zero columns =
// 134.7 KB, dynamic, then col[2][90] and the flag); A_kk is read from the operator when the Schur complement is formed.
#define PRE12_LDS ((size_t)(BcrPre<12>::ROWS * BcrPre<12>::LDP + 2 * BcrPre<12>::NI) * 8 + 16)
__global__ __launch_bounds__(256) void k_bcr_pre12(const BcrOp op, const BcrInit* __restrict__ tab, const int K, const int band, const int Slo, double* __restrict__ ws,
                                                   double* __restrict__ preL, double* __restrict__ preU, double* __restrict__ prew, int* fail) {
    if (op.skip && *op.skip) return;
    using P = BcrPre<12>;
    constexpr int B = P::B, NI = P::NI, NK = P::NK, LDP = P::LDP, ROWS = P::ROWS, SBK = 12;
    extern __shared__ double pre12_lds[];
    double* pan = pre12_lds;                              // [ROWS][LDP]
    double (*col)[NI] = reinterpret_cast<double (*)[NI]>(pre12_lds + ROWS * LDP);       // [2][NI]
    int* s_bad = reinterpret_cast<int*>(pre12_lds + ROWS * LDP + 2 * NI);
    const BcrInit t = tab[blockIdx.x];
    const HView v = bcr_view(op, K, band, B);
    const int cur = op.cur ? *op.cur : 0;
    const double* gsrc = op.gfull[cur];
    const int s = t.sblock, k0 = s * SBK, tid = threadIdx.x;
    constexpr int U = 8;
    if (blockIdx.y > 0) {
        if (t.oC >= 0) bcr_pre_coupling<12>(op, v, K, k0, ws + t.oC);
        return;
    }
    if (t.oD < 0) return;
    if (tid == 0) *s_bad = 0;
    auto unk_inner = [&](const int pp, int& k, int& r) { int kl; P::inner(pp, kl, r); k = k0 + kl; };
    auto unk_kept = [&](const int i, int& k, int& r) { int kl; P::kept(i, kl, r); k = k0 + kl; };
    auto rhs = [&](const int k, const int r) -> double {
        if (k >= K) return 0.0;
        return gsrc[(size_t)k * B + r] * (op.sc ? op.sc[(size_t)k * B + r] : 1.0);
    };
    // ---- the panel: rows 0..89 = A_ii, 90..179 = A_ki, 180 = y_i; columns 90..92 zero (the MFMA loop reads k in fours)
    for (int e0 = tid; e0 < (NI + NK) * NI; e0 += U * 256) {
        double x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * 256, eo = e < (NI + NK) * NI ? e : 0;
            const int row = eo / NI, c = eo - NI * row;
            int ka, ra, kb, cb;
            if (row < NI) unk_inner(row, ka, ra); else unk_kept(row - NI, ka, ra);
            unk_inner(c, kb, cb);
            x[u] = bcr_scaled_entry(op, v, K, B, ka, ra, kb, cb);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) { const int e = e0 + u * 256; if (e < (NI + NK) * NI) pan[(e / NI) * LDP + e % NI] = x[u]; }
    }
    if (tid < NI) { int k, r; unk_inner(tid, k, r); pan[(NI + NK) * LDP + tid] = rhs(k, r); }
    for (int e = tid; e < ROWS * (LDP - NI); e += 256) pan[(e / (LDP - NI)) * LDP + NI + e % (LDP - NI)] = 0.0;
    __syncthreads();
    // ---- 90 register steps, one row per lane (rows 0..89 the inner block, 90..179 the kept rows, 180 the right-hand side)
    bcr_pre_factor<12>(pan, col, s_bad, fail);
    // factors out, Schur complement (A_kk from the operator) and right-hand side of the kept unknowns
    double yk = 0.0;
    if (t.oy >= 0 && tid < NK) { int k, r; unk_kept(tid, k, r); yk = rhs(k, r); }
    bcr_pre_schur<12>(pan, (size_t)(s - Slo), preL, preU, prew, ws + t.oD, t.oy >= 0 ? ws + t.oy : nullptr, yk, [&](const int r, const int c) {
        int ka, ra, kb, cb;
        unk_kept(r, ka, ra); unk_kept(c, kb, cb);
        return bcr_scaled_entry(op, v, K, B, ka, ra, kb, cb);
    });
}
// z_i = L^-T (w - U^T z_k) of one owned 12-keyframe super-block, then the step of its keyframes
__global__ __launch_bounds__(128) void k_bcr_post12(const int* skip, const double* __restrict__ z, const int* __restrict__ node_of, const int Slo, const int K,
                                                    const double* __restrict__ preL, const double* __restrict__ preU, const double* __restrict__ prew,
                                                    double* __restrict__ delta, int* fail) {
    if (skip && *skip) return;
    constexpr int NI = BcrPre<12>::NI, NK = BcrPre<12>::NK, LDL = NI + 1, SBK = 12;
    extern __shared__ double post12_lds[];
    double* Ls = post12_lds;                 // [NI][LDL]
    double* zk = Ls + NI * LDL;              // [NK]
    double* zi = zk + NK;                    // [NI]
    const int sb = blockIdx.x, tid = threadIdx.x, s = Slo + sb, k0 = s * SBK;
    const int node = node_of[sb];
    if (tid < NK) zk[tid] = z[(size_t)node * NK + tid];
    for (int e = tid; e < NI * NI; e += 128) Ls[(e / NI) * LDL + e % NI] = preL[(size_t)sb * NI * NI + e];
    __syncthreads();
    if (tid < NI) zi[tid] = bcr_post_rhs<12>(preU, prew, zk, sb, tid);
    __syncthreads();
    for (int r = NI - 1; r >= 0; --r) {              // back substitution L^T z = t, one column per step
        if (tid == r) zi[r] = zi[r] / Ls[r * LDL + r];
        __syncthreads();
        if (tid < r) zi[tid] -= Ls[r * LDL + tid] * zi[r];
        __syncthreads();
    }
    bcr_post_scatter<12>(zi, zk, k0, K, 128, delta, fail);
}
#define POST12_LDS ((size_t)(BcrPre<12>::NI * (BcrPre<12>::NI + 1) + BcrPre<12>::NK + BcrPre<12>::NI) * 8)

// ------------------------------------------------------------------------------------------------ elimination
template <int M> struct BcrCfg { static constexpr int ROWS = 3 * M + 1; static constexpr int THREADS = ((ROWS + 63) / 64) * 64; };

template <int M>
__global__ __launch_bounds__(BcrCfg<M>::THREADS) void k_bcr_elim(const int* skip, const BcrElim* __restrict__ tab, const double* __restrict__ ws,
                                                                 double* __restrict__ L, double* __restrict__ Ua, double* __restrict__ Ub,
                                                                 double* __restrict__ w, int* fail) {
    if (skip && *skip) return;
    __shared__ double col[2][M];
    __shared__ int s_bad;
    const BcrElim t = tab[blockIdx.x];
    const int row = threadIdx.x;
    const size_t MM = (size_t)M * M;
    double a[M];
    if (row == 0) s_bad = 0;
#pragma unroll
    for (int c = 0; c < M; ++c) a[c] = 0.0;
    if (row < M) {
        const double* src = ws + t.oD + (size_t)row * M;
#pragma unroll
        for (int c = 0; c < M; ++c) a[c] = src[c];
    } else if (row < 2 * M) {             // row r of A[a][node] = column r of A[node][a]
        if (t.a >= 0) {
            const double* src = ws + t.oCa + (row - M);
#pragma unroll
            for (int c = 0; c < M; ++c) a[c] = src[(size_t)c * M];
        }
    } else if (row < 3 * M) {             // row r of A[b][node]
        if (t.b >= 0) {
            const double* src = ws + t.oCb + (size_t)(row - 2 * M) * M;
#pragma unroll
            for (int c = 0; c < M; ++c) a[c] = src[c];
        }
    } else if (row == 3 * M) {
        const double* src = ws + t.oy;
#pragma unroll
        for (int c = 0; c < M; ++c) a[c] = src[c];
    }
    bcr_register_steps<M, 0>(a, row, col, &s_bad);          // (every launched lane is a row: the lanes past 3 M carry zeros)
    if (row == 0 && s_bad) { atomicOr(fail, 1); atomicMin(fail + 1, BCR_ORD_NODE + t.ord); }
    if (row < M) {
        double* dst = L + (size_t)t.node * MM + (size_t)row * M;
#pragma unroll
        for (int c = 0; c < M; ++c) dst[c] = c <= row ? a[c] : 0.0;
    } else if (row < 2 * M) {
        double* dst = Ua + (size_t)t.node * MM + (size_t)(row - M) * M;
#pragma unroll
        for (int c = 0; c < M; ++c) dst[c] = a[c];
    } else if (row < 3 * M) {
        double* dst = Ub + (size_t)t.node * MM + (size_t)(row - 2 * M) * M;
#pragma unroll
        for (int c = 0; c < M; ++c) dst[c] = a[c];
    } else if (row == 3 * M) {
        double* dst = w + (size_t)t.node * M;
#pragma unroll
        for (int c = 0; c < M; ++c) dst[c] = a[c];
    }
}

// ------------------------------------------------------------------------------------------------ elimination, blocked (round 3)
// The same factorisation of the panel [A_pp; A_ap; y^T] and then [A_bp] against L, without a workgroup barrier per pivot:
// 16-column panels; per panel every participating wavefront carries the 16 x 16 diagonal block in lanes 0-15 (factored
// redundantly, pivots and multipliers by v_readlane) and 48 of the rows below in lanes 16-63, so the 16 register steps factor the
// block AND solve those rows; the trailing part takes its rank-16 update as v_mfma_f64_16x16x4 tiles with operands read from LDS
// (the scheme of the window solver's packed LDS Cholesky, solver_kernels.hip, extended by the coupling rows).  Two barriers per
// PANEL instead of one per pivot.  (Another algorithm than k_bcr_elim, not a second writing of it: both stay, chosen by size -- the
// register steps are the faster ones at M = 36, 15 vs 19 us; see GLIO_BCR_ELIM.)  LDS: the packed lower triangle of A_pp (rows at i (i + 1) / 2) + M + 1 full rows
// (A_ap, y, A_bp: 2 M + 1 rows; at M = 90 that is 159.3 of the 160 KB).
#define BCR_E2_THREADS 512
template <int M> struct BcrE2 {
    // row stride of the full rows: M itself when that keeps the 16 rows of an MFMA operand on distinct banks (M = 90: 180 banks apart
    // mod 64 = 52), else M + 1; with stride 90 the whole panel of M = 90 -- triangle + 181 rows -- fits the 160 KB of LDS in ONE pass
    static constexpr int XS = (M % 16 == 10 || M % 16 == 6) ? M : (M | 1), TRI = M * (M + 1) / 2 + ((M * (M + 1) / 2) & 1);
    static constexpr size_t lds_bytes = (size_t)(TRI + (2 * M + 1) * XS) * 8;
};
__device__ __forceinline__ int bcr_pk(const int i) { return (i * (i + 1)) >> 1; }
// 1 / sqrt(d) for a pivot already checked positive and finite: hardware estimate + two Newton steps, without the library's class
// checks (the pivot's reciprocal root is on the critical path of every register step)
__device__ __forceinline__ double bcr_rsqrt(const double d) {
    const double y0 = __builtin_amdgcn_rsq(d);
    const double e = fma(-d * y0, y0, 1.0);
    const double y1 = fma(0.5 * y0, e, y0);
    const double e1 = fma(-d * y1, y1, 1.0);
    return fma(0.5 * y1, e1, y1);
}

// one pass over the panels.  FACTOR: the diagonal rows are factored as well (rows below = remaining diagonal rows, then the R extra
// rows); otherwise L is final and only the R extra rows are solved against it.
template <int M, bool FACTOR>
__device__ __forceinline__ void bcr_panels(double* __restrict__ Lt, double* __restrict__ X, const int R, int* s_bad) {
    using C = BcrE2<M>;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lk = lane >> 4;
    for (int k0 = 0; k0 < M; k0 += 16) {
        const int nb = M - k0 < 16 ? M - k0 : 16, r0 = k0 + nb;
        const int nd = FACTOR ? M - r0 : 0;            // diagonal rows below the block
        const int mb = nd + R;
        BCR_T(tp0);
        if (wv == 0 || wv * 48 < mb) {
            const bool isdiag = lane < 16;
            const int bi = wv * 48 + lane - 16;
            const bool live = isdiag ? lane < nb : bi < mb;
            double* prow = isdiag ? Lt + bcr_pk(live ? k0 + lane : 0) + k0 : (bi < nd ? Lt + bcr_pk(live ? r0 + bi : 0) + k0 : X + (size_t)(live ? bi - nd : 0) * C::XS + k0);
            double a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = (live && j < nb && (!isdiag || j <= lane)) ? prow[j] : ((isdiag && lane == j) ? 1.0 : 0.0);
            bool bad = false;
            if (FACTOR) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if (j >= nb) break;                  // the ragged last panel (6 columns at M = 54, 10 at M = 90): its padding steps are identities
                    double djj = readlane_d(a[j], j);
                    if (!(djj > 1e-290) || !isfinite(djj)) { bad = true; djj = 1.0; }
                    const double rd = bcr_rsqrt(djj);
                    const double lij = (lane == j) ? djj * rd : a[j] * rd;
                    a[j] = lij;
#pragma unroll
                    for (int c = j + 1; c < 16; ++c) a[c] -= lij * readlane_d(lij, c);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) {      // lanes 0-15 hold the finished block L_kk: x_j = a_j / L_jj, a_c -= x_j L_cj
                    if (j >= nb) break;
                    const double ljj = readlane_d(a[j], j);
                    const double xj = isdiag ? a[j] : a[j] / ljj;
                    a[j] = xj;
#pragma unroll
                    for (int c = j + 1; c < 16; ++c) { const double lcj = readlane_d(xj, c); if (!isdiag) a[c] -= xj * lcj; }
                }
            }
            if (live && ((FACTOR && wv == 0) || !isdiag)) {
#pragma unroll
                for (int j = 0; j < 16; ++j) if (j < nb && (!isdiag || j <= lane)) prow[j] = a[j];
            }
            if (bad && wv == 0 && lane == 0) *s_bad = 1;
        }
        __syncthreads();
        BCR_T(tp1);
        BCR_ACC(1, tp1, tp0);
        if (nb == 16 && r0 < M) {
            // rank-16 update of everything right of the panel.  A wavefront owns ROW tiles (16 rows of the list "diagonal rows below the
            // block, then the full rows"): the A operand and the four output-row pointers of a lane are set up once per row tile, the
            // column tiles follow in a loop without divisions (measured: the index arithmetic of a flat tile loop cost as much as
            // the MFMAs themselves).
            const int Tr = (mb + 15) >> 4, Tc = (M - r0 + 15) >> 4;
            constexpr int NW = BCR_E2_THREADS / 64;
            for (int I = wv; I < Tr; I += NW) {
                const int ba = 16 * I + li;
                const bool oka = ba < mb;
                const double* pa = (ba < nd ? Lt + bcr_pk(r0 + (oka ? ba : 0)) : X + (size_t)(oka ? ba - nd : 0) * C::XS) + k0 + lk;
                double ax[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) ax[q] = oka ? pa[4 * q] : 0.0;
                double* orow[4];            // output rows of this lane: row (lane >> 4) + 4 q of the tile; null = outside
                int olim[4];                // last column a diagonal row may take (its own index); M for the full rows
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int br = 16 * I + lk + 4 * q;
                    orow[q] = br >= mb ? nullptr : (br < nd ? Lt + bcr_pk(r0 + br) : X + (size_t)(br - nd) * C::XS);
                    olim[q] = br < nd ? r0 + br : M;
                }
                const int Jn = (FACTOR && 16 * I + 15 < nd) ? (I + 1 < Tc ? I + 1 : Tc) : Tc;      // inside the triangle: tiles up to the diagonal
                for (int J = 0; J < Jn; ++J) {
                    const int cb = r0 + 16 * J + li;
                    const bool okb = cb < M;
                    const double* pb = Lt + bcr_pk(okb ? cb : r0) + k0 + lk;
                    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ax[q], okb ? pb[4 * q] : 0.0, acc, 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (orow[q] && okb && cb <= olim[q]) orow[q][cb] -= acc[q];
                }
            }
        }
        __syncthreads();
        BCR_T(tp2);
        BCR_ACC(2, tp2, tp1);
    }
}

template <int M>
__global__ __launch_bounds__(BCR_E2_THREADS) void k_bcr_elim2(const int* skip, const BcrElim* __restrict__ tab, const double* __restrict__ ws,
                                                              double* __restrict__ L, double* __restrict__ Ua, double* __restrict__ Ub,
                                                              double* __restrict__ w, int* fail) {
    if (skip && *skip) return;
    using C = BcrE2<M>;
    extern __shared__ double bcr_lds[];
    double* Lt = bcr_lds;                  // packed lower triangle of A_pp -> L
    double* X = Lt + C::TRI;               // [2 M + 1][XS]: A_ap rows | y | A_bp rows
    __shared__ int s_bad;
    const BcrElim t = tab[blockIdx.x];
    const int tid = threadIdx.x;
    const size_t MM = (size_t)M * M;
    if (tid == 0) s_bad = 0;
    BCR_T(ts0);
#ifdef GLIO_DEV_STAMPS
    if (blockIdx.x == 0 && tid == 0) { g_bcr_stamps[0] = g_bcr_stamps[1] = g_bcr_stamps[2] = g_bcr_stamps[3] = 0; }
#endif
    constexpr int U = 8;
    for (int e0 = tid; e0 < M * M; e0 += U * BCR_E2_THREADS) {       // eight entries of either block in flight per thread
        double vd[U], vc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * BCR_E2_THREADS, i = e / M, j = e - M * i;
            vd[u] = (e < M * M && j <= i) ? ws[t.oD + e] : 0.0;
            vc[u] = (e < M * M && t.a >= 0) ? ws[t.oCa + e] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * BCR_E2_THREADS, i = e / M, j = e - M * i;
            if (e >= M * M) continue;
            if (j <= i) Lt[bcr_pk(i) + j] = vd[u];
            X[(size_t)j * C::XS + i] = vc[u];          // row r of A[a][node] = column r of A[node][a] (rows node): X[r][c] = C[c][r]
        }
    }
    for (int c = tid; c < M; c += BCR_E2_THREADS) X[(size_t)M * C::XS + c] = ws[t.oy + c];
    // rows M + 1 .. 2 M: A[b][node]
    for (int e0 = tid; e0 < M * M; e0 += U * BCR_E2_THREADS) {
        double vc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int e = e0 + u * BCR_E2_THREADS; vc[u] = (e < M * M && t.b >= 0) ? ws[t.oCb + e] : 0.0; }
#pragma unroll
        for (int u = 0; u < U; ++u) { const int e = e0 + u * BCR_E2_THREADS, i = e / M, j = e - M * i; if (e < M * M) X[(size_t)(M + 1 + i) * C::XS + j] = vc[u]; }
    }
    __syncthreads();
    BCR_T(ts1);
    BCR_ACC(0, ts1, ts0);
    bcr_panels<M, true>(Lt, X, 2 * M + 1, &s_bad);
    BCR_T(ts2);
    // L (zeros above the diagonal), U_a, w, U_b out
    for (int e = tid; e < M * M; e += BCR_E2_THREADS) {
        const int i = e / M, j = e - M * i;
        L[(size_t)t.node * MM + e] = j <= i ? Lt[bcr_pk(i) + j] : 0.0;
        Ua[(size_t)t.node * MM + e] = X[(size_t)i * C::XS + j];
        Ub[(size_t)t.node * MM + e] = X[(size_t)(M + 1 + i) * C::XS + j];
    }
    for (int c = tid; c < M; c += BCR_E2_THREADS) w[(size_t)t.node * M + c] = X[(size_t)M * C::XS + c];
    if (tid == 0 && s_bad) { atomicOr(fail, 1); atomicMin(fail + 1, BCR_ORD_NODE + t.ord); }
#ifdef GLIO_DEV_STAMPS
    __syncthreads();
    { BCR_T(ts3); BCR_ACC(3, ts3, ts2); }
#endif
}
#ifdef GLIO_DEV_STAMPS
extern "C" int glio_debug_bcr_stamps(long long* out8) { return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_bcr_stamps), 64) == hipSuccess ? 0 : -2; }
#endif

// ------------------------------------------------------------------------------------------------ Schur updates of the kept nodes
#define BCR_UP_THREADS 512
// The three M x M x M products of a kept node (U U^T twice, U_b U_a^T once) on the matrix core.  The factors are staged in LDS,
// rows padded with zeros to MP = 16 ceil(M / 16), columns to KP = 4 ceil(M / 4), row stride LD (odd: the 16 lanes of an operand
// column group hit distinct banks).  v_mfma_f64_16x16x4 takes A[i][k] from lane i + 16 k and B[k][j] from lane j + 16 k, so for
// C = X Y^T lane l feeds X[16 I + l % 16][k0 + l / 16] and Y[16 J + l % 16][k0 + l / 16]: ONE 8-byte LDS read per operand per
// 1024 multiply-adds (the 3 x 3 register tiles of the VALU form needed two reads per three).  C comes back with lane l,
// register q = row (l >> 4) + 4 q, column l & 15.
template <int M> struct BcrUp {
    static constexpr int MP = ((M + 15) / 16) * 16, KP = ((M + 3) / 4) * 4, LD = KP | 1, T = MP / 16;
    static constexpr size_t lds_bytes = (size_t)(2 * MP * LD + 2 * M) * 8;
};
// dst (M x M, global, row-major) = (ACCUM ? dst : 0) - X1 Y1^T - X2 Y2^T (either product may be absent: null).  LOWER: only the tiles on and
// below the diagonal (the consumers of a diagonal block read its lower triangle only).  The tile's old values are the accumulator's
// initial value and X is fed negated, so the result lands as "old - X Y^T" without a read-modify-write behind the chain; the next
// tile's old values are loaded while the current chain runs.  (On gfx950 the f64 MFMA has the VALU's throughput -- 78 TFLOP/s either
// way -- so what it buys is operand traffic: one 8-byte LDS read per operand per 1024 multiply-adds.)
template <int M, bool ACCUM, bool LOWER>
__device__ __forceinline__ void bcr_xyT_mfma(const double* __restrict__ X1, const double* __restrict__ Y1, const double* __restrict__ X2,
                                             const double* __restrict__ Y2, const int tid, double* __restrict__ dst) {
    using C = BcrUp<M>;
    const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    constexpr int NW = BCR_UP_THREADS / 64, NT = LOWER ? C::T * (C::T + 1) / 2 : C::T * C::T;
    auto decode = [&](const int tile, int& I, int& J) {
        if (LOWER) { I = 0; while (((I + 1) * (I + 2)) >> 1 <= tile) ++I; J = tile - ((I * (I + 1)) >> 1); }
        else { I = tile / C::T; J = tile - C::T * I; }
    };
    auto load_init = [&](const int tile, v4f64& c) {
        int I = 0, J = 0;
        if (tile < NT) decode(tile, I, J);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * I + lk + 4 * q, col = 16 * J + li;
            c[q] = (ACCUM && tile < NT && r < M && col < M) ? dst[r * M + col] : 0.0;
        }
    };
    v4f64 cnext = {0.0, 0.0, 0.0, 0.0};
    load_init(wave, cnext);
    for (int tile = wave; tile < NT; tile += NW) {
        int I, J;
        decode(tile, I, J);
        v4f64 c = cnext;
        load_init(tile + NW, cnext);
        if (X1) {
            const double* px = X1 + (16 * I + li) * C::LD + lk;
            const double* py = Y1 + (16 * J + li) * C::LD + lk;
#pragma unroll 4
            for (int k0 = 0; k0 < C::KP; k0 += 4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(-px[k0], py[k0], c, 0, 0, 0);
        }
        if (X2) {
            const double* px = X2 + (16 * I + li) * C::LD + lk;
            const double* py = Y2 + (16 * J + li) * C::LD + lk;
#pragma unroll 4
            for (int k0 = 0; k0 < C::KP; k0 += 4) c = __builtin_amdgcn_mfma_f64_16x16x4f64(-px[k0], py[k0], c, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 16 * I + lk + 4 * q, col = 16 * J + li;
            if (r < M && col < M) dst[r * M + col] = c[q];
        }
    }
}
template <int M>
__device__ __forceinline__ void bcr_stage(double* __restrict__ dst, const double* __restrict__ src, const int tid) {
    using C = BcrUp<M>;
    constexpr int N = C::MP * C::KP, U = 8;
    for (int e0 = tid; e0 < N; e0 += U * BCR_UP_THREADS) {          // eight loads in flight per thread
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * BCR_UP_THREADS, r = e / C::KP, c = e - C::KP * r;
            v[u] = (e < N && r < M && c < M) ? src[(size_t)r * M + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * BCR_UP_THREADS, r = e / C::KP, c = e - C::KP * r;
            if (e < N) dst[r * C::LD + c] = v[u];
        }
    }
}

// Two workgroups per kept node: role 0 takes the diagonal block (A_qq -= U_b U_b^T of the node eliminated to the left, -= U_a U_a^T of
// the one to the right: both factors staged side by side, lower tiles only) and the right-hand side; role 1 the new coupling
// A[b][a] = -U_b U_a^T of the node eliminated to the right (all tiles).  The two roles cost about the same.
template <int M>
__global__ __launch_bounds__(BCR_UP_THREADS) void k_bcr_update(const int* skip, const BcrKept* __restrict__ tab, double* __restrict__ ws,
                                                               const double* __restrict__ Ua, const double* __restrict__ Ub, const double* __restrict__ w) {
    if (skip && *skip) return;
    using C = BcrUp<M>;
    extern __shared__ double bcr_lds[];
    double* XA = bcr_lds;
    double* XB = XA + C::MP * C::LD;
    double* wv = XB + C::MP * C::LD;          // [2][M]
    const BcrKept t = tab[blockIdx.x >> 1];
    const int role = blockIdx.x & 1, tid = threadIdx.x;
    const size_t MM = (size_t)M * M;
    if (role == 1) {
        if (t.pr < 0 || t.oCnew < 0) return;
        bcr_stage<M>(XA, Ua + (size_t)t.pr * MM, tid);
        bcr_stage<M>(XB, Ub + (size_t)t.pr * MM, tid);
        __syncthreads();
        bcr_xyT_mfma<M, false, false>(XB, XA, nullptr, nullptr, tid, ws + t.oCnew);          // rows b, columns a (= this node)
        return;
    }
    double* Dq = ws + t.oD;
    double* yq = ws + t.oy;
    if (t.pl >= 0) bcr_stage<M>(XA, Ub + (size_t)t.pl * MM, tid);
    if (t.pr >= 0) bcr_stage<M>(XB, Ua + (size_t)t.pr * MM, tid);
    for (int k = tid; k < M; k += BCR_UP_THREADS) { wv[k] = t.pl >= 0 ? w[(size_t)t.pl * M + k] : 0.0; wv[M + k] = t.pr >= 0 ? w[(size_t)t.pr * M + k] : 0.0; }
    __syncthreads();
    bcr_xyT_mfma<M, true, true>(t.pl >= 0 ? XA : nullptr, XA, t.pr >= 0 ? XB : nullptr, XB, tid, Dq);
    for (int r = tid; r < M; r += BCR_UP_THREADS) {
        double s1 = 0, s2 = 0;
        if (t.pl >= 0) for (int k = 0; k < M; ++k) s1 += XA[r * C::LD + k] * wv[k];
        if (t.pr >= 0) for (int k = 0; k < M; ++k) s2 += XB[r * C::LD + k] * wv[M + k];
        yq[r] = (yq[r] - s1) - s2;
    }
}

// ------------------------------------------------------------------------------------------------ back substitution
template <int M> struct BcrBack { static constexpr size_t lds_bytes = (size_t)(M * (M + 1) + 3 * M + 4 * 128) * 8; };      // Ls, za, zb, rd, pt
template <int M>
__global__ __launch_bounds__(512) void k_bcr_back(const int* skip, const BcrElim* __restrict__ tab, const double* __restrict__ L, const double* __restrict__ Ua,
                                                  const double* __restrict__ Ub, const double* __restrict__ w, double* __restrict__ z) {
    if (skip && *skip) return;
    static_assert(M <= 128 && M % 6 == 0, "two rows per lane; the U^T z sums run in halves of M / 2 rows, three chains");
    extern __shared__ double bcr_lds[];
    constexpr int LD = M + 1, H = M / 2;
    double* Ls = bcr_lds;            // [M][LD]
    double* za = Ls + M * LD;        // [M]
    double* zb = za + M;
    double* pt = zb + M;             // [4][128] partial sums: U_a rows [0, H), [H, M), U_b rows [0, H), [H, M)
    double* rd = pt + 4 * 128;       // [M] reciprocal diagonal of L
    const BcrElim t = tab[blockIdx.x];
    const int tid = threadIdx.x;
    const size_t MM = (size_t)M * M;
    for (int k = tid; k < M; k += 512) { za[k] = t.a >= 0 ? z[(size_t)t.a * M + k] : 0.0; zb[k] = t.b >= 0 ? z[(size_t)t.b * M + k] : 0.0; }
    for (int e0 = tid; e0 < M * M; e0 += 8 * 512) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * 512; v[u] = e < M * M ? L[(size_t)t.node * MM + e] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * 512, r = e / M, c = e - M * r; if (e < M * M) Ls[r * LD + c] = v[u]; }
    }
    __syncthreads();
    // t = w - U_a^T z_a - U_b^T z_b: thread (part, c) sums half of the rows of one factor for column c (coalesced across c)
    {
        const int c = tid & 127, part = tid >> 7, half = part >> 1, r0 = (part & 1) * H;
        const int nbr = half ? t.b : t.a;
        double acc = 0;
        if (c < M && nbr >= 0) {
            const double* U = (half ? Ub : Ua) + (size_t)t.node * MM + (size_t)r0 * M + c;
            const double* zz = (half ? zb : za) + r0;
            // the factor's entries are independent global loads: fifteen at a time in flight (the sums keep three interleaved chains)
            double p3[3] = {0, 0, 0};
            constexpr int CH = H % 15 == 0 ? 15 : 9;
            static_assert(H % CH == 0, "chunk of the U^T z sums");
#pragma unroll
            for (int r = 0; r < H; r += CH) {
                double uv[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) uv[u] = U[(size_t)(r + u) * M];
#pragma unroll
                for (int u = 0; u < CH; ++u) p3[u % 3] += uv[u] * zz[r + u];
            }
            acc = (p3[0] + p3[1]) + p3[2];
        }
        pt[part * 128 + c] = acc;
    }
    if (tid < M) rd[tid] = 1.0 / Ls[tid * LD + tid];
    __syncthreads();
    if (tid >= 64) return;
    // L^T z = t inside wavefront 0, last unknown first; lane l holds t[l] and t[l + 64]; the solved entry travels by a shuffle
    const int lane = tid;
    auto rhs = [&](const int i) { return (w[(size_t)t.node * M + i] - (pt[i] + pt[128 + i])) - (pt[256 + i] + pt[384 + i]); };
    double t0 = lane < M ? rhs(lane) : 0.0;
    double t1 = lane + 64 < M ? rhs(lane + 64) : 0.0;
    // fully unrolled: the pivot entry comes from its lane by v_readlane (a compile-time lane), the reciprocal diagonal and the row of L
    // from LDS -- loads that depend on nothing solved so far, so the scheduler issues them ahead of the chain
#pragma unroll
    for (int r = M - 1; r >= 0; --r) {
        const double tr = r >= 64 ? readlane_d(t1, r - 64) : readlane_d(t0, r);
        const double zr = tr * rd[r];
        if (lane == (r & 63)) { if (r >= 64) t1 = zr; else t0 = zr; }
        if (lane < r) t0 -= Ls[r * LD + lane] * zr;
        if (r > 64 && lane + 64 < r) t1 -= Ls[r * LD + lane + 64] * zr;
    }
    if (lane < M) z[(size_t)t.node * M + lane] = t0;
    if (lane + 64 < M) z[(size_t)t.node * M + lane + 64] = t1;
}

// delta = -z for the OWNED keyframes (the other entries of `delta` are left alone: the sharded caller zeroes them and all-reduces)
__global__ void k_bcr_delta(const int* skip, const double* __restrict__ z, const int* __restrict__ node_of, const int k0, const int k1, const int Slo, const int B,
                            const int M, const int sbk, double* __restrict__ delta, int* fail) {
    if (skip && *skip) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (k1 - k0) * B) return;
    const int k = k0 + e / B, r = e % B;
    const int s = k / sbk;
    const double v = -z[(size_t)node_of[s - Slo] * M + (k % sbk) * B + r];
    if (!isfinite(v)) atomicOr(fail, 2);
    delta[(size_t)k * B + r] = v;
}

// ------------------------------------------------------------------------------------------------ host: schedules
static void bcr_build_schedule(std::vector<int> act, std::vector<char> pinned, std::vector<long long> edgeC /* between consecutive active nodes */,
                               const std::vector<long long>& oD, const std::vector<long long>& oy, long long& next_edge_off, const long long MM,
                               std::vector<BcrElim>& elim, std::vector<BcrKept>& kept, std::vector<int>& elim_off, std::vector<int>& kept_off,
                               long long* final_edge /* the edge left between two pinned nodes, or -1 */) {
    // oD / oy are indexed by node id; edgeC[p] = workspace offset of A[act[p+1]][act[p]]
    for (;;) {
        const int n = (int)act.size();
        int n_free = 0;
        for (int p = 0; p < n; ++p) n_free += pinned[p] ? 0 : 1;
        if (n_free == 0) break;
        std::vector<char> el(n, 0);
        { int idx = 0; for (int p = 0; p < n; ++p) if (!pinned[p]) { el[p] = (idx % 2 == 0); ++idx; } }
        for (int p = 0; p < n; ++p) {
            if (!el[p]) continue;
            BcrElim t;
            t.node = act[p]; t.ord = (int)elim.size();
            t.a = p > 0 ? act[p - 1] : -1; t.b = p + 1 < n ? act[p + 1] : -1;
            t.oD = oD[act[p]]; t.oy = oy[act[p]];
            t.oCa = p > 0 ? edgeC[p - 1] : -1; t.oCb = p + 1 < n ? edgeC[p] : -1;
            elim.push_back(t);
        }
        std::vector<int> nact; std::vector<char> npin; std::vector<long long> nedge;
        for (int p = 0; p < n; ++p) {
            if (el[p]) continue;
            BcrKept t;
            t.node = act[p]; t.pad_ = 0;
            t.pl = (p > 0 && el[p - 1]) ? act[p - 1] : -1;
            t.pr = (p + 1 < n && el[p + 1]) ? act[p + 1] : -1;
            t.oD = oD[act[p]]; t.oy = oy[act[p]];
            t.oCnew = -1;
            // the edge to the next kept node
            long long e_next = -2;        // -2: no next kept node
            if (p + 1 < n && !el[p + 1]) e_next = edgeC[p];                                  // adjacent kept node: the edge stays
            else if (p + 2 < n) { t.oCnew = next_edge_off; next_edge_off += MM; e_next = t.oCnew; }   // through the eliminated node between them
            if (t.pl >= 0 || t.pr >= 0) kept.push_back(t);
            nact.push_back(act[p]); npin.push_back(pinned[p]);
            if (e_next != -2) nedge.push_back(e_next);
        }
        elim_off.push_back((int)elim.size()); kept_off.push_back((int)kept.size());
        act.swap(nact); pinned.swap(npin); edgeC.swap(nedge);
    }
    if (final_edge) *final_edge = (act.size() == 2 && edgeC.size() == 1) ? edgeC[0] : -1;
}

// dynamic LDS above 64 KB has to be allowed per kernel
template <class Kernel>
static void bcr_allow_lds(Kernel* k, const size_t bytes) { hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); }
template <int M>
static void bcr_allow_lds() {
    bcr_allow_lds(k_bcr_update<M>, BcrUp<M>::lds_bytes);
    bcr_allow_lds(k_bcr_elim2<M>, BcrE2<M>::lds_bytes);
    bcr_allow_lds(k_bcr_back<M>, BcrBack<M>::lds_bytes);
}

void* glio_bcr_create2(int K, int band, int B, int rank, int world) {
    if (band > 12 || (B != 6 && B != 15) || world < 1 || rank < 0 || rank >= world) return nullptr;
    BcrDev* b = new BcrDev();
    b->K = K; b->band = band; b->B = B; b->rank = rank; b->world = world;
    b->sbk = band <= 6 ? 6 : 12;
    b->pre = B == 15;
    b->M = b->pre ? (b->sbk == 12 ? BcrPre<12>::NK : BcrPre<6>::NK) : b->sbk * B;
    b->preL = b->preU = b->prew = nullptr;
    b->S = (K + b->sbk - 1) / b->sbk;
    if (b->S < world) { delete b; glio_set_error("batch solver: %d super-blocks cannot be spread over %d ranks", b->S, world); return nullptr; }
    const int S = b->S, M = b->M;
    const long long MM = (long long)M * M;
    b->Slo = (int)((long long)S * rank / world); b->Shi = (int)((long long)S * (rank + 1) / world);
    b->NS = world - 1;
    const bool has_sep = rank < world - 1, has_left = rank > 0;
    const int nown = b->Shi - b->Slo;
    b->nint = nown - (has_sep ? 1 : 0);
    b->nnode = b->nint + b->NS;
    const int nint = b->nint, NS = b->NS;
    // ---- workspace layout: [D int | y int | local edges ... | sepbuf]
    std::vector<long long> oD(b->nnode), oy(b->nnode);
    long long off = 0;
    for (int i = 0; i < nint; ++i) { oD[i] = off; off += MM; }
    for (int i = 0; i < nint; ++i) { oy[i] = off; off += M; }
    // local edge slots: at most 2 per interior node over all levels, plus the original ones
    const long long edge_base = off;
    const long long edge_cap = (long long)(2 * nint + 4) * MM;
    off += edge_cap;
    b->sep_off = off;
    const long long oDsep = off; off += (long long)NS * MM;
    const long long oCsep = off; off += (long long)(NS > 1 ? NS - 1 : 0) * MM;
    const long long oysep = off; off += (long long)NS * M;
    off += 16;
    b->sep_doubles = off - b->sep_off;
    b->ws_doubles = off;
    for (int s = 0; s < NS; ++s) { oD[nint + s] = oDsep + (long long)s * MM; oy[nint + s] = oysep + (long long)s * M; }
    b->node_of_sblock.assign(nown, -1);
    for (int i = 0; i < nint; ++i) b->node_of_sblock[i] = i;
    if (has_sep) b->node_of_sblock[nown - 1] = nint + rank;
    // ---- init tasks (owned super-blocks + the coupling to the left separator) and the local chain
    std::vector<BcrInit> init;
    std::vector<int> act; std::vector<char> pinned; std::vector<long long> edgeC;
    long long next_edge = edge_base;
    if (has_left) {
        // A[Slo][Slo-1]: rows of my first super-block, columns of the left separator; where it goes depends on what my first block is
        BcrInit t; t.sblock = b->Slo - 1; t.pad_ = 0; t.oD = -1; t.oy = -1;
        if (nint > 0) { t.oC = next_edge; next_edge += MM; }
        else t.oC = has_sep ? oCsep + (long long)(rank - 1) * MM : -1;          // no interior block: the separators couple directly
        if (t.oC >= 0) init.push_back(t);
        act.push_back(nint + rank - 1); pinned.push_back(1);
        if (nint > 0) edgeC.push_back(t.oC);
    }
    for (int i = 0; i < nown; ++i) {
        const int node = b->node_of_sblock[i];
        BcrInit t; t.sblock = b->Slo + i; t.pad_ = 0; t.oD = oD[node]; t.oy = oy[node]; t.oC = -1;
        if (i + 1 < nown) { t.oC = next_edge; next_edge += MM; }
        init.push_back(t);
        if (node < nint || has_sep) {
            act.push_back(node); pinned.push_back(node >= nint ? 1 : 0);
            if (i + 1 < nown) edgeC.push_back(t.oC);
        }
    }
    b->n_init = (int)init.size();
    std::vector<BcrElim> elim; std::vector<BcrKept> kept;
    b->h_elim_off.push_back(0); b->h_kept_off.push_back(0);
    long long final_edge = -1;
    // the edge left between the two pinned separators must live in sepbuf (Csep[rank-1]): reserve by building with a scratch edge and
    // redirecting: simplest is to run the schedule, then patch the kept entry that created it
    bcr_build_schedule(act, pinned, edgeC, oD, oy, next_edge, MM, elim, kept, b->h_elim_off, b->h_kept_off, &final_edge);
    b->levels_loc = (int)b->h_elim_off.size() - 1;
    if (has_left && has_sep && final_edge >= 0 && nint > 0) {
        const long long want = oCsep + (long long)(rank - 1) * MM;
        for (BcrKept& t : kept) if (t.oCnew == final_edge) t.oCnew = want;
        for (BcrElim& t : elim) { if (t.oCa == final_edge) t.oCa = want; if (t.oCb == final_edge) t.oCb = want; }
    }
    if (next_edge - edge_base > edge_cap) { delete b; glio_set_error("batch solver: edge workspace exceeded"); return nullptr; }
    // ---- top schedule: the chain of separators
    if (NS > 0) {
        std::vector<int> tact(NS); std::vector<char> tpin(NS, 0); std::vector<long long> tedge;
        for (int s = 0; s < NS; ++s) tact[s] = nint + s;
        for (int s = 0; s + 1 < NS; ++s) tedge.push_back(oCsep + (long long)s * MM);
        // new couplings of the top levels go to private edge slots behind the local ones
        long long top_edge = next_edge;
        bcr_build_schedule(tact, tpin, tedge, oD, oy, top_edge, MM, elim, kept, b->h_elim_off, b->h_kept_off, nullptr);
        if (top_edge - edge_base > edge_cap) { delete b; glio_set_error("batch solver: edge workspace exceeded (top)"); return nullptr; }
    }
    b->levels_top = (int)b->h_elim_off.size() - 1 - b->levels_loc;
    auto A = [](void** p, size_t bytes) { return hipMalloc(p, bytes > 0 ? bytes : 16) == hipSuccess; };
    const size_t nn = (size_t)std::max(b->nnode, 1);
    bool ok = A((void**)&b->ws, (size_t)b->ws_doubles * 8) && A((void**)&b->L, nn * MM * 8) && A((void**)&b->Ua, nn * MM * 8) && A((void**)&b->Ub, nn * MM * 8) &&
              A((void**)&b->w, nn * M * 8) && A((void**)&b->z, nn * M * 8) && A((void**)&b->fail, 16) &&
              A((void**)&b->elim, (elim.size() + 1) * sizeof(BcrElim)) && A((void**)&b->kept, (kept.size() + 1) * sizeof(BcrKept)) &&
              A((void**)&b->init, (init.size() + 1) * sizeof(BcrInit)) && A((void**)&b->node_of_sblock_dev, (size_t)(nown + 1) * 4);
    if (ok && b->pre) {
        const size_t no = (size_t)std::max(nown, 1);
        const size_t ni = b->sbk == 12 ? BcrPre<12>::NI : BcrPre<6>::NI, nk = b->sbk == 12 ? BcrPre<12>::NK : BcrPre<6>::NK;
        ok = A((void**)&b->preL, no * ni * ni * 8) && A((void**)&b->preU, no * nk * ni * 8) && A((void**)&b->prew, no * ni * 8);
    }
    if (!ok) { glio_set_error("batch solver: device allocation failed"); return nullptr; }
    hipMemset(b->ws, 0, (size_t)b->ws_doubles * 8);
    if (!elim.empty()) hipMemcpy(b->elim, elim.data(), elim.size() * sizeof(BcrElim), hipMemcpyHostToDevice);
    if (!kept.empty()) hipMemcpy(b->kept, kept.data(), kept.size() * sizeof(BcrKept), hipMemcpyHostToDevice);
    if (!init.empty()) hipMemcpy(b->init, init.data(), init.size() * sizeof(BcrInit), hipMemcpyHostToDevice);
    hipMemcpy(b->node_of_sblock_dev, b->node_of_sblock.data(), (size_t)nown * 4, hipMemcpyHostToDevice);
    b->h_elim = elim;
    bcr_allow_lds<54>(); bcr_allow_lds<72>(); bcr_allow_lds<90>();          // (M = 36 stays below the 64 KB every kernel may take)
    bcr_allow_lds(k_bcr_pre12, PRE12_LDS);
    bcr_allow_lds(k_bcr_post12, POST12_LDS);
    (void)hipGetLastError();
    return b;
}
void* glio_bcr_create(int K, int band) { return glio_bcr_create2(K, band, 6, 0, 1); }

void glio_bcr_destroy(void* h) {
    BcrDev* b = static_cast<BcrDev*>(h);
    if (!b) return;
    void* ptrs[] = {b->ws, b->L, b->Ua, b->Ub, b->w, b->z, b->elim, b->kept, b->init, b->node_of_sblock_dev, b->fail, b->preL, b->preU, b->prew};
    for (void* p : ptrs) if (p) hipFree(p);
    delete b;
}

void glio_bcr_owned_range(void* h, int* lo, int* hi) {
    BcrDev* b = static_cast<BcrDev*>(h);
    *lo = b->Slo * b->sbk; *hi = std::min(b->K, b->Shi * b->sbk);
}
double* glio_bcr_sepbuf(void* h, long long* count) {
    BcrDev* b = static_cast<BcrDev*>(h);
    *count = b->sep_doubles;
    return b->ws + b->sep_off;
}
int* glio_bcr_fail_flag(void* h) { return static_cast<BcrDev*>(h)->fail; }
void glio_bcr_view(void* h, BcrView* v) {
    BcrDev* b = static_cast<BcrDev*>(h);
    v->M = b->M; v->sbk = b->sbk; v->S = b->S; v->K = b->K; v->band = b->band; v->B = b->B; v->nnode = b->nnode; v->levels = b->levels_loc + b->levels_top;
    v->world = b->world; v->pre = b->pre ? 1 : 0;
    v->NI = !b->pre ? 0 : (b->sbk == 12 ? BcrPre<12>::NI : BcrPre<6>::NI); v->NK = !b->pre ? 0 : (b->sbk == 12 ? BcrPre<12>::NK : BcrPre<6>::NK);
    v->n_elim = (int)b->h_elim.size();
    v->L = b->L; v->Ua = b->Ua; v->Ub = b->Ub; v->preL = b->preL; v->preU = b->preU;
    v->h_elim = b->h_elim.data(); v->h_elim_off = b->h_elim_off.data();
    v->fail = b->fail;
}

// -1 (default): by size -- the blocked elimination (k_bcr_elim2) for M >= 54, one register step per pivot with a workgroup barrier each
// (k_bcr_elim) for M = 36, where it is the faster one (15 vs 19 us on MI355X); 1 / 0 force either (GLIO_BCR_ELIM, cross-checks)
void glio_bcr_debug_set_elim(int mode) { glio_switch_set<GLIO_SW_BCR_ELIM>(mode); }
template <int M>
static void bcr_levels(BcrDev* b, const BcrOp& op, int l0, int l1, hipStream_t stream) {
    const size_t lds_up = BcrUp<M>::lds_bytes;
    for (int l = l0; l < l1; ++l) {
        const int ne = b->h_elim_off[l + 1] - b->h_elim_off[l], nk = b->h_kept_off[l + 1] - b->h_kept_off[l];
        if (ne > 0) {
            if (const int mode = glio_switch<GLIO_SW_BCR_ELIM>(); mode == 0 || (mode < 0 && M < 54)) hipLaunchKernelGGL((k_bcr_elim<M>), dim3(ne), dim3(BcrCfg<M>::THREADS), 0, stream, op.skip, b->elim + b->h_elim_off[l], b->ws, b->L, b->Ua, b->Ub, b->w, b->fail);
            else hipLaunchKernelGGL((k_bcr_elim2<M>), dim3(ne), dim3(BCR_E2_THREADS), BcrE2<M>::lds_bytes, stream, op.skip, b->elim + b->h_elim_off[l], b->ws, b->L, b->Ua, b->Ub, b->w, b->fail);
        }
        if (nk > 0) hipLaunchKernelGGL((k_bcr_update<M>), dim3(2 * nk), dim3(BCR_UP_THREADS), lds_up, stream, op.skip, b->kept + b->h_kept_off[l], b->ws, b->Ua, b->Ub, b->w);
    }
}
template <int M>
static void bcr_back(BcrDev* b, const BcrOp& op, int l0, int l1, hipStream_t stream) {
    for (int l = l1 - 1; l >= l0; --l) {
        const int ne = b->h_elim_off[l + 1] - b->h_elim_off[l];
        if (ne > 0) hipLaunchKernelGGL((k_bcr_back<M>), dim3(ne), dim3(512), BcrBack<M>::lds_bytes, stream, op.skip, b->elim + b->h_elim_off[l], b->L, b->Ua, b->Ub, b->w, b->z);
    }
}
#define BCR_DISPATCH(fn, ...) do { if (b->M == 36) fn<36>(__VA_ARGS__); else if (b->M == 54) fn<54>(__VA_ARGS__); else if (b->M == 72) fn<72>(__VA_ARGS__); else fn<90>(__VA_ARGS__); } while (0)

// phase 1: operator -> blocks, local elimination; afterwards sepbuf holds this rank's share of the separator system (all-reduce it)
void glio_bcr_enqueue_local(void* h, const BcrOp& op, hipStream_t stream) {
    BcrDev* b = static_cast<BcrDev*>(h);
    hipMemsetAsync(b->fail, 0, 4, stream);
    if (b->sep_doubles > 16) hipMemsetAsync(b->ws + b->sep_off, 0, (size_t)(b->sep_doubles - 16) * 8, stream);      // (the 16 extra scalars belong to the caller)
    if (b->n_init > 0 && b->pre && b->sbk == 12)
        hipLaunchKernelGGL(k_bcr_pre12, dim3(b->n_init, 3), dim3(256), PRE12_LDS, stream, op, b->init, b->K, b->band, b->Slo, b->ws, b->preL, b->preU, b->prew, b->fail);
    else if (b->n_init > 0 && b->pre)
        hipLaunchKernelGGL(k_bcr_pre, dim3(b->n_init, 3), dim3(256), 0, stream, op, b->init, b->K, b->band, b->Slo, b->ws, b->preL, b->preU, b->prew, b->fail);
    else if (b->n_init > 0) hipLaunchKernelGGL(k_bcr_init, dim3(b->n_init, BCR_INIT_SPLIT), dim3(256), 0, stream, op, b->init, b->K, b->band, b->B, b->M, b->sbk, b->ws);
    BCR_DISPATCH(bcr_levels, b, op, 0, b->levels_loc, stream);
}
// phase 2 (after the all-reduce of sepbuf): the separator chain, then back through the local levels; delta = -z for the owned keyframes
void glio_bcr_enqueue_finish(void* h, const BcrOp& op, double* delta, hipStream_t stream) {
    BcrDev* b = static_cast<BcrDev*>(h);
    const int lt0 = b->levels_loc, lt1 = b->levels_loc + b->levels_top;
    BCR_DISPATCH(bcr_levels, b, op, lt0, lt1, stream);
    BCR_DISPATCH(bcr_back, b, op, lt0, lt1, stream);
    BCR_DISPATCH(bcr_back, b, op, 0, b->levels_loc, stream);
    int lo, hi;
    glio_bcr_owned_range(b, &lo, &hi);
    if (hi > lo && b->pre && b->sbk == 12)
        hipLaunchKernelGGL(k_bcr_post12, dim3(b->Shi - b->Slo), dim3(128), POST12_LDS, stream, op.skip, b->z, b->node_of_sblock_dev, b->Slo, b->K, b->preL, b->preU, b->prew, delta, b->fail);
    else if (hi > lo && b->pre)
        hipLaunchKernelGGL(k_bcr_post, dim3(b->Shi - b->Slo), dim3(64), 0, stream, op.skip, b->z, b->node_of_sblock_dev, b->Slo, b->K, b->preL, b->preU, b->prew, delta, b->fail);
    else if (hi > lo) hipLaunchKernelGGL(k_bcr_delta, dim3(((hi - lo) * b->B + 255) / 256), dim3(256), 0, stream, op.skip, b->z, b->node_of_sblock_dev, lo, hi, b->Slo, b->B, b->M,
                                    b->sbk, delta, b->fail);
}

// (H + lambda diag H) x = g (dadd: an explicit additive diagonal instead), delta = -x; the one-rank pose problem of the damped
// Gauss-Newton path (glio_batch_step_dev).  *fail_dev (int) is set non-zero on a non-positive pivot.
void glio_bcr_solve_shift(void* h, const double* Hg, double lambda, const double* dadd, double* delta, int** fail_dev, hipStream_t stream) {
    BcrDev* b = static_cast<BcrDev*>(h);
    BcrOp op;
    memset(&op, 0, sizeof op);
    op.Hg[0] = op.Hg[1] = Hg; op.lambda = lambda; op.dadd = dadd;
    glio_bcr_enqueue_local(h, op, stream);
    glio_bcr_enqueue_finish(h, op, delta, stream);
    *fail_dev = b->fail;
}
void glio_bcr_solve(void* h, const double* Hg, double lambda, double* delta, int** fail_dev, hipStream_t stream) { glio_bcr_solve_shift(h, Hg, lambda, nullptr, delta, fail_dev, stream); }
int glio_bcr_levels(void* h) { BcrDev* b = static_cast<BcrDev*>(h); return b->levels_loc + b->levels_top; }

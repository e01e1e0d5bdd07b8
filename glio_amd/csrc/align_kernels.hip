// align_kernels.hip -- the GNSS frame on the device (include/glio_align.h): yaw_enu_local and anc_ecef of a glio_gnss_frame from a local trajectory and the
// double-differenced pseudoranges along it.  A circle of yaw hypotheses at the start anchor (the cost is not convex in yaw), then Gauss-Newton on
// (d_e, d_n, d_u, d_psi) through the caller's threshold rounds.  The row and its derivatives are factor_math.h's fm_align_row; the whitening is fm_dd_whiten.
//
//   k_align_unpack         one lane per factor: its row records (factor, satellite, row in the factor, the factor's first lane in its workgroup)
//   k_align_start          the frames of the H hypotheses and of the start (device ecef2rotation), the state reset
//   k_align_rows<NS>       one lane per row: the raw row, the whitening through LDS (a factor's rows share a workgroup), NS products summed over the
//                          workgroup in a fixed order into this workgroup's partial.  NS = 10 for the search (grid.y = H), 16 for a linearisation
//   k_align_coarse_reduce  one wave per hypothesis: its partials in a fixed order, the 3 x 3 Cholesky, the reduced cost
//   k_align_pick           the lowest cost (lowest h on a tie), the runner-up, the state's frame
//   k_align_step           one workgroup: the partials in a fixed order, the 4 x 4 Cholesky, observability, the step, the round's end and the solve's end
//   k_align_cost_reduce    glio_align_cost: the partials' r^T r and down-weighted count
//
// The whole solve is enqueued ahead.  Every launch of round r tests state.round == r on the device and returns at once otherwise, so the launches behind
// the deciding iteration cost their launch only.  No atomic anywhere: every sum has a fixed place and order that depend on the factors' row counts and H only.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/glio_align.h"
#include "factor_math.h"
#include "glio_device.h"

#define AL_THREADS 256
#define AL_FR_STATE GLIO_ALIGN_MAX_HYPOTHESES          // frames[]: the hypotheses, then the solve's current frame, then glio_align_cost's
#define AL_FR_COST (GLIO_ALIGN_MAX_HYPOTHESES + 1)
#define AL_PI 3.14159265358979323846

struct AlFrame { double psi, c, s, anc[3], Ree[9], R[9]; };
struct AlArgs {                    // by value into the kernels: no upload
    double psi, anc[3];
    int32_t H, n_rounds, max_it, pad_;
    double thresholds[GLIO_ALIGN_MAX_ROUNDS], yaw_tol, pos_tol, max_yaw_sigma;
};
struct AlState { int32_t round, it, done, pad_; glio_align_info info; double psi, anc[3]; };

struct glio_align {
    int device, max_factors, max_positions;
    hipStream_t stream;
    hipEvent_t ev_t0, ev_t1;
    glio_dd_psr* d_fac; int4* d_rows; int32_t* d_blk; int2* d_unpack; double* d_pos; AlFrame* d_frames; double* d_part; double* d_coarse; AlState* d_state;
    double* d_cost;                // glio_align_cost: cost, count
    size_t part_cap;               // doubles
    AlState* h_state; double* h_cost;     // pinned
    glio_align_opts o;
    int n_fac, n_rows, n_blk, n_pos, max_slot, coarse_h, timed;
};

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(AL_THREADS) void k_align_unpack(const glio_dd_psr* __restrict__ fac, const int2* __restrict__ up, const int n_fac, int4* __restrict__ rows) {
    const int f = blockIdx.x * AL_THREADS + threadIdx.x;
    if (f >= n_fac) return;
    const int ns = fac[f].n_sat, m = fac[f].master;
    const int2 u = up[f];                                 // x: the factor's first row, y: its first lane in its workgroup
    for (int i = 0, ri = 0; i < ns; ++i) {
        if (i == m) continue;
        rows[u.x + ri] = make_int4(f, i, ri, u.y);
        ++ri;
    }
}

__device__ __forceinline__ void al_frame_set(AlFrame& fr, const double psi, const double anc[3], const double Ree[9]) {
    fr.psi = psi; fr.c = cos(psi); fr.s = sin(psi);
    for (int k = 0; k < 3; ++k) fr.anc[k] = anc[k];
    for (int k = 0; k < 9; ++k) fr.Ree[k] = Ree[k];
    fm_ecef_local(Ree, fr.c, fr.s, fr.R);
}

// which = AL_FR_STATE: the hypotheses and the start of a solve (and the state reset); AL_FR_COST: the one frame of glio_align_cost
__global__ __launch_bounds__(AL_THREADS) void k_align_start(const AlArgs a, const int which, const int n_rows, AlFrame* __restrict__ frames, AlState* __restrict__ st) {
    const int h = blockIdx.x * AL_THREADS + threadIdx.x;
    const int n = which == AL_FR_STATE ? a.H : 0;
    if (h > n) return;
    double Ree[9];
    fm_ecef2rotation(a.anc, Ree);
    if (h < n) { al_frame_set(frames[h], (2.0 * AL_PI * h) / n, a.anc, Ree); return; }
    al_frame_set(frames[which], a.psi, a.anc, Ree);
    if (which != AL_FR_STATE) return;
    st->round = 0; st->it = 0; st->done = 0; st->pad_ = 0;
    static_assert(sizeof(glio_align_info) % 8 == 0, "zeroed as doubles");
    double* z = reinterpret_cast<double*>(&st->info);
    for (int k = 0; k < (int)(sizeof(glio_align_info) / 8); ++k) z[k] = 0;
    st->info.winner = -1; st->info.n_rows = n_rows;
    st->psi = a.psi;
    for (int k = 0; k < 3; ++k) st->anc[k] = a.anc[k];
}

template <int NS>
__global__ __launch_bounds__(AL_THREADS) void k_align_rows(const glio_dd_psr* __restrict__ fac, const int4* __restrict__ rows, const int32_t* __restrict__ blk, const double* __restrict__ pos,
                                                           const AlFrame* __restrict__ frames, const int frame0, const double threshold, const AlState* __restrict__ st,
                                                           const int gate_round, double* __restrict__ part) {
    if (gate_round >= 0 && (st->done || st->round != gate_round)) return;          // behind the deciding iteration: nothing to do
    __shared__ double raw[AL_THREADS], Ja[3 * AL_THREADS], Jb[3 * AL_THREADS], red[AL_THREADS / GLIO_WAVE][NS];
    const int t = threadIdx.x, r0 = blk[blockIdx.x], nr = blk[blockIdx.x + 1] - r0;
    const AlFrame& fr = frames[frame0 + blockIdx.y];
    int4 rec = make_int4(0, 0, 0, 0);
    int down = 0;
    if (t < nr) {
        rec = rows[r0 + t];
        const glio_dd_psr& F = fac[rec.x];
        double R[9], anc[3], Pi[3], Pj[3], r, ja[3], jb[3];
        for (int k = 0; k < 9; ++k) R[k] = fr.R[k];
        for (int k = 0; k < 3; ++k) { anc[k] = fr.anc[k]; Pi[k] = pos[3 * F.slot_i + k]; Pj[k] = pos[3 * F.slot_j + k]; }
        fm_align_row(F, rec.y, threshold, Pi, Pj, R, anc, fr.c, fr.s, r, ja, jb, down);
        raw[t] = r;
        for (int k = 0; k < 3; ++k) { Ja[3 * t + k] = ja[k]; Jb[3 * t + k] = jb[k]; }
    }
    __syncthreads();
    double v[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) v[q] = 0;
    if (t < nr) {
        const glio_dd_psr& F = fac[rec.x];
        double sr, sa[3], sb[3];
        fm_dd_whiten(F.weight, rec.z, F.n_sat - 1, raw + rec.w, Ja + 3 * rec.w, Jb + 3 * rec.w, sr, sa, sb);
        if (NS == 10) {
            v[0] = sa[0] * sa[0]; v[1] = sa[0] * sa[1]; v[2] = sa[0] * sa[2]; v[3] = sa[1] * sa[1]; v[4] = sa[1] * sa[2]; v[5] = sa[2] * sa[2];
            v[6] = sa[0] * sr; v[7] = sa[1] * sr; v[8] = sa[2] * sr; v[9] = sr * sr;
        } else {
            const double J[4] = {sa[0], sa[1], sa[2], sb[0]};
            int q = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j) v[q++] = J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[10 + i] = J[i] * sr;
            v[NS - 2] = sr * sr; v[NS - 1] = (double)down;
        }
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) {
        const double w = wave_sum(v[q]);
        if ((t & (GLIO_WAVE - 1)) == 0) red[t / GLIO_WAVE][q] = w;
    }
    __syncthreads();
    if (t < NS) part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// L L^T = the n x n matrix in A (row major, lower triangle read), in place; the pivots before the root in piv.  false: a pivot not positive and finite
template <int N> __device__ __forceinline__ bool al_chol(double A[N * N], double piv[N]) {
    for (int j = 0; j < N; ++j) {
        double d = A[j * N + j];
        for (int k = 0; k < j; ++k) d -= A[j * N + k] * A[j * N + k];
        piv[j] = d;
        if (!(d > 0.0) || !isfinite(d)) return false;
        const double l = sqrt(d);
        A[j * N + j] = l;
        for (int i = j + 1; i < N; ++i) {
            double x = A[i * N + j];
            for (int k = 0; k < j; ++k) x -= A[i * N + k] * A[j * N + k];
            A[i * N + j] = x / l;
        }
    }
    return true;
}
template <int N> __device__ __forceinline__ void al_chol_solve(const double L[N * N], const double b[N], double x[N]) {
    double y[N];
    for (int i = 0; i < N; ++i) { double a = b[i]; for (int k = 0; k < i; ++k) a -= L[i * N + k] * y[k]; y[i] = a / L[i * N + i]; }
    for (int i = N - 1; i >= 0; --i) { double a = y[i]; for (int k = i + 1; k < N; ++k) a -= L[k * N + i] * x[k]; x[i] = a / L[i * N + i]; }
}

__global__ __launch_bounds__(GLIO_WAVE) void k_align_coarse_reduce(const double* __restrict__ part, const int n_blk, double* __restrict__ coarse) {
    const int h = blockIdx.x, lane = threadIdx.x;
    double v[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) v[q] = 0;
    for (int b = lane; b < n_blk; b += GLIO_WAVE)
#pragma unroll
        for (int q = 0; q < 10; ++q) v[q] += part[((size_t)h * n_blk + b) * 10 + q];
#pragma unroll
    for (int q = 0; q < 10; ++q) v[q] = wave_sum(v[q]);
    if (lane != 0) return;
    double A[9] = {v[0], 0, 0, v[1], v[3], 0, v[2], v[4], v[5]}, piv[3], x[3];
    const double b3[3] = {v[6], v[7], v[8]};
    double c = INFINITY;
    if (al_chol<3>(A, piv)) {
        al_chol_solve<3>(A, b3, x);
        c = 0.5 * (v[9] - (b3[0] * x[0] + b3[1] * x[1] + b3[2] * x[2]));
        if (!isfinite(c)) c = INFINITY;
    }
    coarse[h] = c;
}

__global__ __launch_bounds__(GLIO_WAVE) void k_align_pick(const double* __restrict__ coarse, const int H, AlFrame* __restrict__ frames, AlState* __restrict__ st) {
    __shared__ double c1[GLIO_WAVE], c2[GLIO_WAVE];
    __shared__ int h1[GLIO_WAVE];
    const int lane = threadIdx.x;
    double a = INFINITY, b = INFINITY;
    int ha = -1;
    for (int h = lane; h < H; h += GLIO_WAVE) {           // ascending h: a strict < keeps the lowest on a tie
        const double c = coarse[h];
        if (c < a) { b = a; a = c; ha = h; } else if (c < b) b = c;
    }
    c1[lane] = a; c2[lane] = b; h1[lane] = ha;
    __syncthreads();
    if (lane != 0) return;
    double best = INFINITY, second = INFINITY;
    int hb = -1;
    for (int l = 0; l < GLIO_WAVE; ++l) {
        const double c = c1[l];
        if (h1[l] >= 0 && (c < best || (c == best && h1[l] < hb))) { if (best < second) second = best; best = c; hb = h1[l]; }
        else if (c < second) second = c;
        if (c2[l] < second) second = c2[l];
    }
    st->info.winner = hb;
    if (hb < 0) { st->info.status = GLIO_ALIGN_UNOBSERVABLE; st->done = 1; return; }
    st->info.coarse_cost = best; st->info.runner_up_cost = second;
    frames[AL_FR_STATE] = frames[hb];
    st->psi = frames[hb].psi;
}

__global__ __launch_bounds__(AL_THREADS) void k_align_step(const AlArgs a, const int round, const double* __restrict__ part, const int n_blk, AlFrame* __restrict__ frames, AlState* __restrict__ st) {
    if (st->done || st->round != round) return;
    __shared__ double red[16][16], tot[16];
    const int t = threadIdx.x, q = t & 15, l = t >> 4;
    double acc = 0;
    for (int b = l; b < n_blk; b += 16) acc += part[(size_t)b * 16 + q];
    red[l][q] = acc;
    __syncthreads();
    if (t < 16) { double s = 0; for (int k = 0; k < 16; ++k) s += red[k][t]; tot[t] = s; }
    __syncthreads();
    if (t != 0) return;
    glio_align_info& info = st->info;
    double A[16], piv[4] = {0, 0, 0, 0}, g[4], d[4];
    { int k = 0; for (int i = 0; i < 4; ++i) for (int j = i; j < 4; ++j) { A[j * 4 + i] = tot[k]; A[i * 4 + j] = tot[k]; ++k; } }
    for (int i = 0; i < 4; ++i) g[i] = -tot[10 + i];
    const double hpp = A[15];
    const int it = st->it + 1;
    info.n_rounds = round + 1;
    info.round_iterations[round] = it; info.round_cost[round] = 0.5 * tot[14]; info.round_downweighted[round] = (int32_t)tot[15];
    info.h_yaw_yaw = hpp;
    if (!al_chol<4>(A, piv) || !(piv[3] > 1e-9 * hpp)) {
        info.status = GLIO_ALIGN_UNOBSERVABLE; info.yaw_schur = piv[3] == piv[3] ? piv[3] : 0.0; info.yaw_sigma = 0;
        for (int k = 0; k < 16; ++k) info.covariance[k] = 0;
        st->done = 1;
        return;
    }
    al_chol_solve<4>(A, g, d);
    for (int c = 0; c < 4; ++c) {                          // (J^T J)^-1, column by column; the lower triangle mirrored so that it is symmetric to the bit
        double e[4] = {0, 0, 0, 0}, x[4];
        e[c] = 1.0;
        al_chol_solve<4>(A, e, x);
        for (int r = c; r < 4; ++r) { info.covariance[r * 4 + c] = x[r]; info.covariance[c * 4 + r] = x[r]; }
    }
    info.yaw_schur = piv[3]; info.yaw_sigma = 1.0 / sqrt(piv[3]);
    AlFrame& fr = frames[AL_FR_STATE];
    double anc[3], Ree[9];
    for (int k = 0; k < 3; ++k) anc[k] = fr.anc[k] + (fr.Ree[3 * k] * d[0] + fr.Ree[3 * k + 1] * d[1] + fr.Ree[3 * k + 2] * d[2]);
    double psi = fr.psi + d[3];
    const bool conv = fabs(d[3]) <= a.yaw_tol && sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= a.pos_tol;
    st->it = it;
    if (conv || it >= a.max_it) {
        st->round = round + 1; st->it = 0;
        if (round + 1 >= a.n_rounds) {
            while (psi > AL_PI) psi -= 2.0 * AL_PI;
            while (psi <= -AL_PI) psi += 2.0 * AL_PI;
            info.status = (a.max_yaw_sigma > 0 && info.yaw_sigma > a.max_yaw_sigma) ? GLIO_ALIGN_WEAK : GLIO_ALIGN_OK;
            st->done = 1;
        }
    }
    fm_ecef2rotation(anc, Ree);                            // the rotation at the new anchor
    al_frame_set(fr, psi, anc, Ree);
    st->psi = psi;
    for (int k = 0; k < 3; ++k) st->anc[k] = anc[k];
}

__global__ __launch_bounds__(AL_THREADS) void k_align_cost_reduce(const double* __restrict__ part, const int n_blk, double* __restrict__ out) {
    __shared__ double red[2][AL_THREADS];
    const int t = threadIdx.x;
    double rr = 0, nd = 0;
    for (int b = t; b < n_blk; b += AL_THREADS) { rr += part[(size_t)b * 16 + 14]; nd += part[(size_t)b * 16 + 15]; }
    red[0][t] = rr; red[1][t] = nd;
    __syncthreads();
    for (int w = AL_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) { red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = 0.5 * red[0][0]; out[1] = red[1][0]; }
}

// ---------------------------------------------------------------------------------------------------------------- host
static bool al_finite(const double* v, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

static int al_part_room(glio_align* al, size_t doubles) {
    if (doubles <= al->part_cap) return GLIO_OK;
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    if (al->d_part) { GLIO_HIP_CHECK(hipFree(al->d_part)); al->d_part = nullptr; al->part_cap = 0; }
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_part, doubles * 8));
    al->part_cap = doubles;
    return GLIO_OK;
}

static int al_ready(glio_align* al, const char* who) {
    if (al->n_fac < 1) { glio_set_error("%s: no factors (glio_align_set_factors first)", who); return GLIO_E_ARG; }
    if (al->n_pos < 1) { glio_set_error("%s: no positions (glio_align_set_positions first)", who); return GLIO_E_ARG; }
    if (al->max_slot >= al->n_pos) { glio_set_error("%s: a factor reads position %d of a table of %d", who, al->max_slot, al->n_pos); return GLIO_E_ARG; }
    return GLIO_OK;
}

static AlArgs al_args(const glio_align* al, const glio_gnss_frame* f) {
    AlArgs a;
    memset(&a, 0, sizeof a);
    a.psi = f->yaw_enu_local;
    for (int k = 0; k < 3; ++k) a.anc[k] = f->anc_ecef[k];
    a.H = al->o.n_hypotheses; a.n_rounds = al->o.n_rounds; a.max_it = al->o.max_iterations_per_round;
    for (int k = 0; k < GLIO_ALIGN_MAX_ROUNDS; ++k) a.thresholds[k] = al->o.thresholds[k];
    a.yaw_tol = al->o.yaw_tolerance; a.pos_tol = al->o.pos_tolerance; a.max_yaw_sigma = al->o.max_yaw_sigma;
    return a;
}

extern "C" {

void glio_align_opts_default(glio_align_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->n_hypotheses = 72; o->n_rounds = 4; o->max_iterations_per_round = 10;
    o->thresholds[0] = 1e9; o->thresholds[1] = 10; o->thresholds[2] = 8; o->thresholds[3] = 6;
    o->yaw_tolerance = 1e-8; o->pos_tolerance = 1e-6; o->max_yaw_sigma = 0;
}
int glio_align_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_align_opts), (int32_t)sizeof(glio_align_info)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

static int align_create_body(glio_align* al) {
    const size_t F = (size_t)al->max_factors, rows = F * (GLIO_DD_MAX_SAT - 1);
    GLIO_HIP_CHECK(hipStreamCreateWithFlags(&al->stream, hipStreamNonBlocking));
    GLIO_HIP_CHECK(hipEventCreate(&al->ev_t0));
    GLIO_HIP_CHECK(hipEventCreate(&al->ev_t1));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_fac, F * sizeof(glio_dd_psr)));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_rows, rows * sizeof(int4)));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_blk, (F + 2) * sizeof(int32_t)));          // a workgroup holds at least one factor
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_unpack, F * sizeof(int2)));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_pos, (size_t)al->max_positions * 3 * 8));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_frames, (GLIO_ALIGN_MAX_HYPOTHESES + 2) * sizeof(AlFrame)));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_coarse, GLIO_ALIGN_MAX_HYPOTHESES * 8));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_state, sizeof(AlState)));
    GLIO_HIP_CHECK(hipMalloc((void**)&al->d_cost, 2 * 8));
    GLIO_HIP_CHECK(hipMemset(al->d_state, 0, sizeof(AlState)));
    GLIO_HIP_CHECK(hipHostMalloc((void**)&al->h_state, sizeof(AlState)));
    GLIO_HIP_CHECK(hipHostMalloc((void**)&al->h_cost, 2 * 8));
    return GLIO_OK;
}
int glio_align_create(int device, int max_factors, int max_positions, glio_align** out) {
    if (!out || max_factors < 1 || max_factors > (1 << 22) || max_positions < 1 || max_positions > (1 << 24)) {
        glio_set_error("glio_align_create: bad argument (max_factors 1 .. 2^22, max_positions 1 .. 2^24)"); return GLIO_E_ARG;
    }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) { glio_set_error("no HIP device visible: the alignment has no CPU fallback"); return GLIO_E_HIP; }
    if (device < 0 || device >= nd) { glio_set_error("glio_align_create: device %d of %d", device, nd); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(device));
    glio_align* al = new glio_align();
    memset(al, 0, sizeof *al);
    al->device = device; al->max_factors = max_factors; al->max_positions = max_positions; al->max_slot = -1;
    glio_align_opts_default(&al->o);
    const int rc = align_create_body(al);
    if (rc != GLIO_OK) { glio_align_destroy(al); return rc; }
    *out = al;
    return GLIO_OK;
}
void glio_align_destroy(glio_align* al) {
    if (!al) return;
    (void)hipSetDevice(al->device);
    if (al->stream) (void)hipStreamSynchronize(al->stream);
    void* dev[] = {al->d_fac, al->d_rows, al->d_blk, al->d_unpack, al->d_pos, al->d_frames, al->d_part, al->d_coarse, al->d_state, al->d_cost};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (al->h_state) (void)hipHostFree(al->h_state);
    if (al->h_cost) (void)hipHostFree(al->h_cost);
    if (al->ev_t0) (void)hipEventDestroy(al->ev_t0);
    if (al->ev_t1) (void)hipEventDestroy(al->ev_t1);
    if (al->stream) (void)hipStreamDestroy(al->stream);
    delete al;
}

int glio_align_set_opts(glio_align* al, const glio_align_opts* o) {
    if (!al || !o) { glio_set_error("glio_align_set_opts: null argument"); return GLIO_E_ARG; }
    if (o->n_hypotheses < 0 || o->n_hypotheses > GLIO_ALIGN_MAX_HYPOTHESES) { glio_set_error("glio_align_set_opts: n_hypotheses %d outside [0, %d]", o->n_hypotheses, GLIO_ALIGN_MAX_HYPOTHESES); return GLIO_E_ARG; }
    if (o->n_rounds < 1 || o->n_rounds > GLIO_ALIGN_MAX_ROUNDS) { glio_set_error("glio_align_set_opts: %d thresholds, 1 .. %d are taken", o->n_rounds, GLIO_ALIGN_MAX_ROUNDS); return GLIO_E_ARG; }
    if (o->max_iterations_per_round < 1 || o->max_iterations_per_round > GLIO_ALIGN_MAX_ITERATIONS) { glio_set_error("glio_align_set_opts: max_iterations_per_round %d outside [1, %d]", o->max_iterations_per_round, GLIO_ALIGN_MAX_ITERATIONS); return GLIO_E_ARG; }
    for (int k = 0; k < o->n_rounds; ++k)
        if (!(o->thresholds[k] > 0)) { glio_set_error("glio_align_set_opts: threshold %d is not positive", k); return GLIO_E_ARG; }
    const double tol[3] = {o->yaw_tolerance, o->pos_tolerance, o->max_yaw_sigma};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(tol[k]) || tol[k] < 0) { glio_set_error("glio_align_set_opts: a tolerance or max_yaw_sigma is negative or not finite"); return GLIO_E_ARG; }
    al->o = *o;
    return GLIO_OK;
}

int glio_align_set_factors(glio_align* al, int n_dd, const glio_dd_psr* dd) {
    if (!al || !dd) { glio_set_error("glio_align_set_factors: null argument"); return GLIO_E_ARG; }
    if (n_dd < 1 || n_dd > al->max_factors) { glio_set_error("glio_align_set_factors: %d factors, the object takes 1 .. %d", n_dd, al->max_factors); return GLIO_E_ARG; }
    std::vector<int2> up((size_t)n_dd);
    std::vector<int32_t> blk(1, 0);
    int rows = 0, in_blk = 0, max_slot = -1;
    for (int f = 0; f < n_dd; ++f) {
        const glio_dd_psr& F = dd[f];
        if (F.n_sat < 2 || F.n_sat > GLIO_DD_MAX_SAT || F.master < 0 || F.master >= F.n_sat) { glio_set_error("glio_align_set_factors: factor %d: n_sat %d, master %d", f, F.n_sat, F.master); return GLIO_E_ARG; }
        if (F.slot_i < 0 || F.slot_i >= al->max_positions || F.slot_j < 0 || F.slot_j >= al->max_positions) {
            glio_set_error("glio_align_set_factors: factor %d: slots %d, %d outside a table of %d", f, F.slot_i, F.slot_j, al->max_positions); return GLIO_E_ARG;
        }
        const int nw = F.n_sat - 1;
        if (in_blk + nw > AL_THREADS) { blk.push_back(rows); in_blk = 0; }             // a factor's rows stay together
        up[f] = make_int2(rows, in_blk);
        rows += nw; in_blk += nw;
        max_slot = F.slot_i > max_slot ? F.slot_i : max_slot;
        max_slot = F.slot_j > max_slot ? F.slot_j : max_slot;
    }
    blk.push_back(rows);
    const int n_blk = (int)blk.size() - 1;
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    { const int rc = al_part_room(al, (size_t)n_blk * 16); if (rc != GLIO_OK) return rc; }
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    GLIO_HIP_CHECK(hipMemcpyAsync(al->d_fac, dd, (size_t)n_dd * sizeof(glio_dd_psr), hipMemcpyHostToDevice, al->stream));
    GLIO_HIP_CHECK(hipMemcpyAsync(al->d_unpack, up.data(), (size_t)n_dd * sizeof(int2), hipMemcpyHostToDevice, al->stream));
    GLIO_HIP_CHECK(hipMemcpyAsync(al->d_blk, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, al->stream));
    hipLaunchKernelGGL(k_align_unpack, dim3((n_dd + AL_THREADS - 1) / AL_THREADS), dim3(AL_THREADS), 0, al->stream, al->d_fac, al->d_unpack, n_dd, al->d_rows);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));          // the host vectors die with this call
    al->n_fac = n_dd; al->n_rows = rows; al->n_blk = n_blk; al->max_slot = max_slot;
    return GLIO_OK;
}

int glio_align_set_positions(glio_align* al, int n, const double* base, int stride_doubles) {
    if (!al || !base) { glio_set_error("glio_align_set_positions: null argument"); return GLIO_E_ARG; }
    if (n < 1 || n > al->max_positions || stride_doubles < 3) { glio_set_error("glio_align_set_positions: %d positions (1 .. %d are taken), stride %d (at least 3)", n, al->max_positions, stride_doubles); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    GLIO_HIP_CHECK(hipMemcpy2DAsync(al->d_pos, 24, base, (size_t)stride_doubles * 8, 24, (size_t)n, hipMemcpyHostToDevice, al->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    al->n_pos = n;
    return GLIO_OK;
}

int glio_align_solve(glio_align* al, const glio_gnss_frame* start, glio_gnss_frame* out, glio_align_info* info) {
    if (!al || !start || !out) { glio_set_error("glio_align_solve: null argument"); return GLIO_E_ARG; }
    { const int rc = al_ready(al, "glio_align_solve"); if (rc != GLIO_OK) return rc; }
    if (!std::isfinite(start->yaw_enu_local) || !al_finite(start->anc_ecef, 3)) { glio_set_error("glio_align_solve: the start frame is not finite"); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    const AlArgs a = al_args(al, start);
    const int H = a.H, nb = al->n_blk;
    { const int rc = al_part_room(al, (size_t)nb * (H > 0 ? (size_t)H * 10 : 16) + (size_t)nb * 16); if (rc != GLIO_OK) return rc; }
    GLIO_HIP_CHECK(hipEventRecord(al->ev_t0, al->stream));
    hipLaunchKernelGGL(k_align_start, dim3(H / AL_THREADS + 1), dim3(AL_THREADS), 0, al->stream, a, AL_FR_STATE, al->n_rows, al->d_frames, al->d_state);
    if (H > 0) {
        hipLaunchKernelGGL(k_align_rows<10>, dim3(nb, H), dim3(AL_THREADS), 0, al->stream, al->d_fac, al->d_rows, al->d_blk, al->d_pos, al->d_frames, 0, (double)INFINITY,
                           al->d_state, -1, al->d_part);
        hipLaunchKernelGGL(k_align_coarse_reduce, dim3(H), dim3(GLIO_WAVE), 0, al->stream, al->d_part, nb, al->d_coarse);
        hipLaunchKernelGGL(k_align_pick, dim3(1), dim3(GLIO_WAVE), 0, al->stream, al->d_coarse, H, al->d_frames, al->d_state);
    }
    for (int r = 0; r < a.n_rounds; ++r)
        for (int it = 0; it < a.max_it; ++it) {
            hipLaunchKernelGGL(k_align_rows<16>, dim3(nb, 1), dim3(AL_THREADS), 0, al->stream, al->d_fac, al->d_rows, al->d_blk, al->d_pos, al->d_frames, AL_FR_STATE, a.thresholds[r],
                               al->d_state, r, al->d_part);
            hipLaunchKernelGGL(k_align_step, dim3(1), dim3(AL_THREADS), 0, al->stream, a, r, al->d_part, nb, al->d_frames, al->d_state);
        }
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(al->ev_t1, al->stream));
    GLIO_HIP_CHECK(hipMemcpyAsync(al->h_state, al->d_state, sizeof(AlState), hipMemcpyDeviceToHost, al->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));          // the one host wait
    al->timed = 1; al->coarse_h = H;
    const AlState& s = *al->h_state;
    if (info) *info = s.info;
    if (s.info.status == GLIO_ALIGN_UNOBSERVABLE) { *out = *start; return GLIO_OK; }
    out->yaw_enu_local = s.psi;
    for (int k = 0; k < 3; ++k) out->anc_ecef[k] = s.anc[k];
    return GLIO_OK;
}

int glio_align_cost(glio_align* al, const glio_gnss_frame* frame, double threshold, double* cost, int32_t* n_downweighted) {
    if (!al || !frame || !cost) { glio_set_error("glio_align_cost: null argument"); return GLIO_E_ARG; }
    { const int rc = al_ready(al, "glio_align_cost"); if (rc != GLIO_OK) return rc; }
    if (!std::isfinite(frame->yaw_enu_local) || !al_finite(frame->anc_ecef, 3) || !(threshold > 0)) { glio_set_error("glio_align_cost: a frame that is not finite or a threshold that is not positive"); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    const AlArgs a = al_args(al, frame);
    const int nb = al->n_blk;
    GLIO_HIP_CHECK(hipEventRecord(al->ev_t0, al->stream));
    hipLaunchKernelGGL(k_align_start, dim3(1), dim3(AL_THREADS), 0, al->stream, a, AL_FR_COST, al->n_rows, al->d_frames, al->d_state);
    hipLaunchKernelGGL(k_align_rows<16>, dim3(nb, 1), dim3(AL_THREADS), 0, al->stream, al->d_fac, al->d_rows, al->d_blk, al->d_pos, al->d_frames, AL_FR_COST, threshold, al->d_state, -1,
                       al->d_part);
    hipLaunchKernelGGL(k_align_cost_reduce, dim3(1), dim3(AL_THREADS), 0, al->stream, al->d_part, nb, al->d_cost);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(al->ev_t1, al->stream));
    GLIO_HIP_CHECK(hipMemcpyAsync(al->h_cost, al->d_cost, 16, hipMemcpyDeviceToHost, al->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    al->timed = 1;
    *cost = al->h_cost[0];
    if (n_downweighted) *n_downweighted = (int32_t)al->h_cost[1];
    return GLIO_OK;
}

int glio_align_read_coarse(glio_align* al, double* costs, int capacity, int32_t* n) {
    if (!al || (!costs && !n)) { glio_set_error("glio_align_read_coarse: null argument"); return GLIO_E_ARG; }
    if (al->coarse_h < 1) { glio_set_error("glio_align_read_coarse: no solve with a search yet"); return GLIO_E_STATE; }
    if (n) *n = al->coarse_h;
    if (!costs) return GLIO_OK;
    if (capacity < al->coarse_h) { glio_set_error("glio_align_read_coarse: room for %d costs, the last solve had %d hypotheses", capacity, al->coarse_h); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    GLIO_HIP_CHECK(hipMemcpyAsync(costs, al->d_coarse, (size_t)al->coarse_h * 8, hipMemcpyDeviceToHost, al->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(al->stream));
    return GLIO_OK;
}

int glio_align_last_device_ms(glio_align* al, float* ms) {
    if (!al || !ms) return GLIO_E_ARG;
    if (!al->timed) { glio_set_error("glio_align_solve first"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(al->device));
    GLIO_HIP_CHECK(hipEventSynchronize(al->ev_t1));
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, al->ev_t0, al->ev_t1));
    return GLIO_OK;
}

}  // extern "C"

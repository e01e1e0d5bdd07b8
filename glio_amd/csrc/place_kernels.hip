// place_kernels.hip -- place recognition on the device (include/glio_place.h): the Scan Context descriptor of resident keyframe clouds and the exact
// scan-context distance of a query place to every stored place.  The rules are stated in the header; they are the library's own (UNPINNED) and restated in
// numpy by the tests.
//
// Descriptor (k_pl_describe): one workgroup per frame, one launch per call.  The cells live in LDS as the order-preserving integer image of a float
// (f2ord); a point's value enters with an integer atomic max, its sector with an atomic or -- neither depends on the order of the points.  Behind a
// barrier the same workgroup writes the heights and forms the 60 unit columns (pl_unit_column: fp64 norm over ascending ring, float division), stored
// k-major with 64 columns per ring, the last four zero: the layout the pair kernel's MFMA operands are read from.
//
// Pairs (k_pl_pairs): one wavefront per (query, run of PL_RUN candidates).  G = Q^T C, 64 x 64 with K = 20, on v_mfma_f32_16x16x4_f32: 16 tiles x 5 steps.
// Lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and receives D[i = 4 (l >> 4) + r][j = l & 15] in register r.  The query's 20
// operand registers are loaded once per wavefront.  G goes to LDS (row stride 65: lane s reads the diagonal j -> (j, (j + s) mod 60) without a bank
// conflict); lane s < 60 sums its wrapped diagonal over ascending j; a butterfly takes the minimum by (distance, shift).  A pair's result is written to
// its own slot: nothing of it depends on the run it was computed in.
// Selection (k_pl_select): one workgroup per query behind the pair kernel; top_k rounds of "the smallest (distance, place) above the last one taken".
#include <cfloat>
#include <cmath>
#include <cstring>

#include "glio_device.h"
#include "../../include/glio_place.h"

// every product and sum rounds on its own, as the float32 restatement's do
#pragma clang fp contract(off)

#define PL_CELLS (GLIO_PLACE_RINGS * GLIO_PLACE_SECTORS)   /* 1200 */
#define PL_UCOLS 64                                        /* columns per ring in the unit-column layout */
#define PL_USIZE (GLIO_PLACE_RINGS * PL_UCOLS)             /* 1280 floats per place */
#define PL_RUN 16                                          /* candidates per wavefront of k_pl_pairs */
#define PL_GSTRIDE 65
#define PL_PAIR_BUDGET (1 << 22)                           /* pair slots per chunk of queries (32 MB) */
#define PL_MAX_PLACES (1 << 17)
#define PL_EMPTY ((int)0x80000000)                         /* no finite float has this image */
#define PL_MASK60 ((1ull << 60) - 1ull)

typedef unsigned long long pl_u64;
typedef float pl_f32x4 __attribute__((ext_vector_type(4)));

struct PlTables { float rb2[GLIO_PLACE_RINGS + 1]; float dir[2 * GLIO_PLACE_SECTORS]; };
struct PlFrame { const float4* src; int n, place; float R[9]; int pad_; double time; };
struct PlPair { float dist; int shift; };                  // shift < 0: not a candidate

struct glio_place {
    GlioBassocView v;
    glio_bassoc* owner_b; glio_dense* owner_d;
    glio_place_opts o;
    PlTables tab;
    hipStream_t stream;
    hipEvent_t ev_dep, ev_done, ev_up, ev_t0, ev_t1;
    float* d_h; pl_u64* d_mask; pl_u64* d_pmask; float* d_u; double* d_time; int* d_valid;
    PlFrame* h_fr; PlFrame* d_fr;
    PlPair* d_pair; size_t pair_cap;
    glio_place_match* d_match; glio_place_match* h_match; int* d_nfound; int* h_nfound;
    unsigned char* h_valid; double* h_time; unsigned* h_stamp; unsigned stamp;
    int n_hi, up_pending, have_ms;
};

// ---- the descriptor
// column j of the heights at h (stride GLIO_PLACE_SECTORS between rings) -> u[k * PL_UCOLS + j]; returns whether the column is present
__device__ __forceinline__ bool pl_unit_column(const float* h, const bool has_point, const int j, float* __restrict__ u) {
    double s = 0.0;
    float c[GLIO_PLACE_RINGS];
#pragma unroll
    for (int k = 0; k < GLIO_PLACE_RINGS; ++k) { c[k] = j < GLIO_PLACE_SECTORS ? h[k * GLIO_PLACE_SECTORS + j] : 0.f; s += (double)c[k] * (double)c[k]; }
    const float nrm = (float)sqrt(s);
    const bool present = j < GLIO_PLACE_SECTORS && has_point && nrm > 0.f && nrm <= FLT_MAX;
#pragma unroll
    for (int k = 0; k < GLIO_PLACE_RINGS; ++k) u[k * PL_UCOLS + j] = present ? c[k] / nrm : 0.f;
    return present;
}
// the cell of a levelled point; false: the point is skipped
__device__ __forceinline__ bool pl_cell_of(const PlTables& tab, const float x, const float y, int& ring, int& sector) {
    const float r2 = (x * x) + (y * y);
    if (!(r2 > 0.f && r2 < tab.rb2[GLIO_PLACE_RINGS])) return false;
    int r = 0;
#pragma unroll
    for (int k = 1; k < GLIO_PLACE_RINGS; ++k) r += tab.rb2[k] <= r2 ? 1 : 0;
    const int q = (x > 0.f && y >= 0.f) ? 0 : (x <= 0.f && y > 0.f) ? 1 : (x < 0.f && y <= 0.f) ? 2 : 3;
    int s = 0;
    for (int k = 1; k < 15; ++k) {
        const float dx = tab.dir[2 * (15 * q + k)], dy = tab.dir[2 * (15 * q + k) + 1];
        s += ((dx * y) - (dy * x)) >= 0.f ? 1 : 0;
    }
    ring = r; sector = 15 * q + s;
    return true;
}
__global__ __launch_bounds__(256) void k_pl_describe(const PlFrame* __restrict__ frames, const PlTables tab, const float lidar_height, float* __restrict__ heights,
                                                     pl_u64* __restrict__ mask, pl_u64* __restrict__ pmask, float* __restrict__ u, double* __restrict__ time,
                                                     int* __restrict__ valid) {
    __shared__ int s_cell[PL_CELLS];
    __shared__ float s_h[PL_CELLS];
    __shared__ unsigned s_col[2];
    __shared__ PlTables s_tab;
    const PlFrame f = frames[blockIdx.x];
    const int tid = threadIdx.x;
    for (int c = tid; c < PL_CELLS; c += 256) s_cell[c] = PL_EMPTY;
    if (tid < 2) s_col[tid] = 0u;
    for (int k = tid; k < (int)(sizeof(PlTables) / 4); k += 256) reinterpret_cast<float*>(&s_tab)[k] = reinterpret_cast<const float*>(&tab)[k];
    __syncthreads();
    for (int i = tid; i < f.n; i += 256) {
        const float4 p = f.src[i];
        if (!(fabsf(p.x) <= FLT_MAX && fabsf(p.y) <= FLT_MAX && fabsf(p.z) <= FLT_MAX)) continue;
        const float x = ((f.R[0] * p.x) + (f.R[1] * p.y)) + (f.R[2] * p.z);
        const float y = ((f.R[3] * p.x) + (f.R[4] * p.y)) + (f.R[5] * p.z);
        const float z = ((f.R[6] * p.x) + (f.R[7] * p.y)) + (f.R[8] * p.z);
        int ring, sector;
        if (!pl_cell_of(s_tab, x, y, ring, sector)) continue;
        float val = z + lidar_height;
        if (!(fabsf(val) <= FLT_MAX)) continue;
        if (val == 0.f) val = 0.f;                                     // (-0 is stored as +0)
        atomicMax(&s_cell[ring * GLIO_PLACE_SECTORS + sector], f2ord(val));          // (ring < 20, sector < 60 by construction)
        atomicOr(&s_col[sector >> 5], 1u << (sector & 31));
    }
    __syncthreads();
    float* hp = heights + (size_t)f.place * PL_CELLS;
    for (int c = tid; c < PL_CELLS; c += 256) { const int im = s_cell[c]; const float hv = im == PL_EMPTY ? 0.f : ord2f(im); s_h[c] = hv; hp[c] = hv; }
    __syncthreads();
    if (tid < 64) {
        const pl_u64 m = ((pl_u64)s_col[1] << 32 | (pl_u64)s_col[0]) & PL_MASK60;
        const bool present = pl_unit_column(s_h, tid < GLIO_PLACE_SECTORS && ((m >> tid) & 1ull), tid, u + (size_t)f.place * PL_USIZE);
        const pl_u64 pm = __ballot(present);
        if (tid == 0) { mask[f.place] = m; pmask[f.place] = pm & PL_MASK60; time[f.place] = f.time; valid[f.place] = 1; }
    }
}
// the same normalisation for a descriptor that came from the host (glio_place_set_descriptor): heights and mask are in place
__global__ __launch_bounds__(64) void k_pl_normalise(const int place, const double t, const float* __restrict__ heights, const pl_u64* __restrict__ mask,
                                                     pl_u64* __restrict__ pmask, float* __restrict__ u, double* __restrict__ time, int* __restrict__ valid) {
    const int tid = threadIdx.x;
    const pl_u64 m = mask[place];
    const bool present = pl_unit_column(heights + (size_t)place * PL_CELLS, tid < GLIO_PLACE_SECTORS && ((m >> tid) & 1ull), tid, u + (size_t)place * PL_USIZE);
    const pl_u64 pm = __ballot(present);
    if (tid == 0) { pmask[place] = pm & PL_MASK60; time[place] = t; valid[place] = 1; }
}

// ---- the query
__global__ __launch_bounds__(64) void k_pl_pairs(const float* __restrict__ u, const pl_u64* __restrict__ pmask, const double* __restrict__ time,
                                                 const int* __restrict__ valid, const int q0, const int P, const double gap, const int earlier,
                                                 PlPair* __restrict__ out) {
    __shared__ float G[64 * PL_GSTRIDE];
    const int lane = threadIdx.x, q = q0 + (int)blockIdx.y;
    const int c0 = (int)blockIdx.x * PL_RUN, c1 = min(P, c0 + PL_RUN);
    PlPair* row = out + (size_t)blockIdx.y * P;
    const bool qv = valid[q] != 0;                                     // (q < P <= max_places: the host's range check)
    if (!qv) { if (lane < c1 - c0) { PlPair r; r.dist = INFINITY; r.shift = -1; row[c0 + lane] = r; } return; }
    const double tq = time[q];
    const pl_u64 qm = pmask[q];
    const int lo = lane & 15, hi = lane >> 4;
    float qa[4][5];
    {
        const float* uq = u + (size_t)q * PL_USIZE;
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) qa[ti][kk] = uq[(4 * kk + hi) * PL_UCOLS + 16 * ti + lo];
        }
    }
    for (int c = c0; c < c1; ++c) {
        // (uniform over the wavefront)
        bool ok = c != q && valid[c] != 0;
        if (ok) { const double tc = time[c]; ok = fabs(tc - tq) > gap && (!earlier || tc < tq); }
        if (!ok) { if (lane == 0) { PlPair r; r.dist = INFINITY; r.shift = -1; row[c] = r; } continue; }
        const float* uc = u + (size_t)c * PL_USIZE;
        float cb[4][5];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) cb[tj][kk] = uc[(4 * kk + hi) * PL_UCOLS + 16 * tj + lo];
        }
        const pl_u64 cm = pmask[c];
        pl_f32x4 acc[4][4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = (pl_f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) {
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
                for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[ti][kk], cb[tj][kk], acc[ti][tj], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
#pragma unroll
                for (int r = 0; r < 4; ++r) G[(16 * ti + 4 * hi + r) * PL_GSTRIDE + 16 * tj + lo] = acc[ti][tj][r];
            }
        }
        GLIO_WAVE_LDS_SYNC();
        const int s = lane < GLIO_PLACE_SECTORS ? lane : 0;
        float sum = 0.f;
        int jj = s;
        for (int j = 0; j < GLIO_PLACE_SECTORS; ++j) {
            sum += G[j * PL_GSTRIDE + jj];
            jj = jj + 1 == GLIO_PLACE_SECTORS ? 0 : jj + 1;
        }
        const pl_u64 rot = s == 0 ? cm : ((cm >> s) | (cm << (GLIO_PLACE_SECTORS - s))) & PL_MASK60;      // bit j = the candidate's column (j + s) mod 60
        const int cnt = __popcll(qm & rot);
        float d = cnt > 0 ? 1.0f - sum / (float)cnt : 1.0f;
        int sh = s;
        if (lane >= GLIO_PLACE_SECTORS) { d = INFINITY; sh = 0x7fffffff; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(d, off, 64); const int os = __shfl_xor(sh, off, 64);
            if (od < d || (od == d && os < sh)) { d = od; sh = os; }
        }
        if (lane == 0) { PlPair r; r.dist = d; r.shift = sh; row[c] = r; }
        GLIO_WAVE_LDS_SYNC();                                           // (the next candidate overwrites G)
    }
}
// the top_k of a query's row by ascending (distance, place): round r takes the smallest pair above the one round r - 1 took
__global__ __launch_bounds__(256) void k_pl_select(const PlPair* __restrict__ pairs, const int P, const int top_k, const int qoff, glio_place_match* __restrict__ matches,
                                                   int* __restrict__ n_found) {
    __shared__ float s_d[4]; __shared__ int s_i[4];
    const PlPair* row = pairs + (size_t)blockIdx.x * P;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    glio_place_match* mo = matches + (size_t)(qoff + (int)blockIdx.x) * top_k;
    float ld = -INFINITY; int li = -1, found = 0;
    for (int r = 0; r < top_k; ++r) {
        float bd = INFINITY; int bi = 0x7fffffff;
        for (int c = tid; c < P; c += 256) {
            const PlPair p = row[c];
            if (p.shift < 0) continue;
            const bool above = p.dist > ld || (p.dist == ld && c > li);
            if (above && (p.dist < bd || (p.dist == bd && c < bi))) { bd = p.dist; bi = c; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(bd, off, 64); const int oi = __shfl_xor(bi, off, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        __syncthreads();
        if (lane == 0) { s_d[w] = bd; s_i[w] = bi; }
        __syncthreads();
        bd = s_d[0]; bi = s_i[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) if (s_d[k] < bd || (s_d[k] == bd && s_i[k] < bi)) { bd = s_d[k]; bi = s_i[k]; }
        if (bi == 0x7fffffff) break;                                     // (uniform: every thread holds the same pair)
        if (tid == 0) {
            glio_place_match m;
            m.place = bi; m.shift = row[bi].shift; m.distance = bd; m.yaw = (float)((double)m.shift * (6.283185307179586 / 60.0));
            mo[r] = m;
        }
        ld = bd; li = bi; found = r + 1;
    }
    if (tid == 0) n_found[qoff + (int)blockIdx.x] = found;
}

#define PL_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

static bool pl_finite(const double v) { return fabs(v) <= DBL_MAX; }
static void pl_tables(const double max_radius, PlTables* t) {
    for (int k = 0; k <= GLIO_PLACE_RINGS; ++k) { const double r = (double)k * max_radius / 20.0; t->rb2[k] = (float)(r * r); }
    for (int s = 0; s < GLIO_PLACE_SECTORS; ++s) {
        const double a = (6.283185307179586 * (double)s) / 60.0;
        t->dir[2 * s] = (float)cos(a); t->dir[2 * s + 1] = (float)sin(a);
    }
}
// the rotation matrix of q / |q| (w first), formed in double, stored as float; q null: the identity.  false: q is not finite or zero
static bool pl_level_matrix(const double* q, float* R) {
    double w = 1.0, x = 0.0, y = 0.0, z = 0.0;
    if (q) {
        for (int k = 0; k < 4; ++k) if (!pl_finite(q[k])) return false;
        const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        if (!(n > 0.0) || !pl_finite(n)) return false;
        w = q[0] / n; x = q[1] / n; y = q[2] / n; z = q[3] / n;
    }
    const double m[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)};
    for (int k = 0; k < 9; ++k) R[k] = (float)m[k];
    return true;
}
// the pinned argument array is free again once the previous call's upload has left it
static int pl_wait_upload(glio_place* pl) {
    if (pl->up_pending) { PL_CHECK(hipEventSynchronize(pl->ev_up)); pl->up_pending = 0; }
    return GLIO_OK;
}

extern "C" {

void glio_place_opts_default(glio_place_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->max_places = 4096;
    o->top_k_max = GLIO_PLACE_TOP_K_MAX;
    o->max_radius = 80.0f;
    o->lidar_height = 2.0f;
}
int glio_place_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_place_opts), (int32_t)sizeof(glio_place_match)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}
int glio_place_tables(float max_radius, float* rb2, float* dir) {
    if (!rb2 || !dir || !(max_radius > 0.f) || !(max_radius <= FLT_MAX)) { glio_set_error("glio_place_tables: max_radius %g / null pointer", (double)max_radius); return GLIO_E_ARG; }
    PlTables t;
    pl_tables((double)max_radius, &t);
    memcpy(rb2, t.rb2, sizeof t.rb2);
    memcpy(dir, t.dir, sizeof t.dir);
    return GLIO_OK;
}

void glio_place_destroy(glio_place* pl) {
    if (!pl) return;
    hipSetDevice(pl->v.device);
    if (pl->stream) hipStreamSynchronize(pl->stream);
    void* p[] = {pl->d_h, pl->d_mask, pl->d_pmask, pl->d_u, pl->d_time, pl->d_valid, pl->d_fr, pl->d_pair, pl->d_match, pl->d_nfound};
    for (void* q : p) if (q) hipFree(q);
    void* h[] = {pl->h_fr, pl->h_match, pl->h_nfound};
    for (void* q : h) if (q) hipHostFree(q);
    hipEvent_t ev[] = {pl->ev_dep, pl->ev_done, pl->ev_up, pl->ev_t0, pl->ev_t1};
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (pl->stream) hipStreamDestroy(pl->stream);
    delete[] pl->h_valid; delete[] pl->h_time; delete[] pl->h_stamp;
    delete pl;
}

static int pl_create_body(glio_place* pl) {
    const size_t np = (size_t)pl->o.max_places, nk = (size_t)pl->o.top_k_max;
    PL_CHECK(hipSetDevice(pl->v.device));
    PL_CHECK(hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking));
    PL_CHECK(hipEventCreateWithFlags(&pl->ev_dep, hipEventDisableTiming));
    PL_CHECK(hipEventCreateWithFlags(&pl->ev_done, hipEventDisableTiming | hipEventBlockingSync));
    PL_CHECK(hipEventCreateWithFlags(&pl->ev_up, hipEventDisableTiming | hipEventBlockingSync));
    PL_CHECK(hipEventCreate(&pl->ev_t0)); PL_CHECK(hipEventCreate(&pl->ev_t1));
    PL_CHECK(hipMalloc((void**)&pl->d_h, np * PL_CELLS * 4)); PL_CHECK(hipMalloc((void**)&pl->d_u, np * PL_USIZE * 4));
    PL_CHECK(hipMalloc((void**)&pl->d_mask, np * 8)); PL_CHECK(hipMalloc((void**)&pl->d_pmask, np * 8));
    PL_CHECK(hipMalloc((void**)&pl->d_time, np * 8)); PL_CHECK(hipMalloc((void**)&pl->d_valid, np * 4));
    PL_CHECK(hipMalloc((void**)&pl->d_fr, np * sizeof(PlFrame))); PL_CHECK(hipHostMalloc((void**)&pl->h_fr, np * sizeof(PlFrame)));
    pl->pair_cap = np > (size_t)PL_PAIR_BUDGET ? np : (size_t)PL_PAIR_BUDGET;
    if (pl->pair_cap > np * np) pl->pair_cap = np * np;
    PL_CHECK(hipMalloc((void**)&pl->d_pair, pl->pair_cap * sizeof(PlPair)));
    PL_CHECK(hipMalloc((void**)&pl->d_match, np * nk * sizeof(glio_place_match))); PL_CHECK(hipHostMalloc((void**)&pl->h_match, np * nk * sizeof(glio_place_match)));
    PL_CHECK(hipMalloc((void**)&pl->d_nfound, np * 4)); PL_CHECK(hipHostMalloc((void**)&pl->h_nfound, np * 4));
    PL_CHECK(hipMemsetAsync(pl->d_valid, 0, np * 4, pl->stream));
    PL_CHECK(hipMemsetAsync(pl->d_h, 0, np * PL_CELLS * 4, pl->stream));
    PL_CHECK(hipMemsetAsync(pl->d_mask, 0, np * 8, pl->stream));
    PL_CHECK(hipMemsetAsync(pl->d_time, 0, np * 8, pl->stream));
    pl->h_valid = new unsigned char[np](); pl->h_time = new double[np](); pl->h_stamp = new unsigned[np]();
    PL_CHECK(hipStreamSynchronize(pl->stream));
    return GLIO_OK;
}
static int pl_create(glio_bassoc* b, glio_dense* d, const glio_place_opts* opts, glio_place** out) {
    if ((!b && !d) || !opts || !out) return GLIO_E_ARG;
    const glio_place_opts& o = *opts;
    if (o.max_places < 1 || o.max_places > PL_MAX_PLACES || o.top_k_max < 1 || o.top_k_max > GLIO_PLACE_TOP_K_MAX || !(o.max_radius > 0.f) || !(o.max_radius <= FLT_MAX) ||
        !(fabsf(o.lidar_height) <= FLT_MAX)) {
        glio_set_error("bad glio_place_opts (max_places %d, top_k_max %d, max_radius %g, lidar_height %g)", o.max_places, o.top_k_max, (double)o.max_radius, (double)o.lidar_height);
        return GLIO_E_ARG;
    }
    glio_place* pl = new glio_place();
    memset(pl, 0, sizeof *pl);
    pl->o = o;
    pl->owner_b = b; pl->owner_d = d;
    pl_tables((double)o.max_radius, &pl->tab);
    { const int rv = d ? glio_dense_view(d, &pl->v) : glio_bassoc_view(b, &pl->v); if (rv != GLIO_OK) { delete pl; return rv; } }
    const int rc = pl_create_body(pl);
    if (rc != GLIO_OK) { glio_place_destroy(pl); return rc; }
    *out = pl;
    return GLIO_OK;
}
int glio_place_create(glio_bassoc* b, const glio_place_opts* opts, glio_place** out) { return pl_create(b, nullptr, opts, out); }
int glio_place_create_on_dense(glio_dense* d, const glio_place_opts* opts, glio_place** out) { return pl_create(nullptr, d, opts, out); }

int glio_place_add_frames(glio_place* pl, int n, const int32_t* frame_idx, const int32_t* place_idx, const double* level_q, const double* times) {
    GLIO_TRACE("glio_place_add_frames");
    if (!pl) return GLIO_E_ARG;
    if (n < 1 || n > pl->o.max_places) { glio_set_error("glio_place_add_frames: %d frames, a call takes 1 .. %d", n, pl->o.max_places); return GLIO_E_ARG; }
    if (!frame_idx || !place_idx || !times) { glio_set_error("glio_place_add_frames: null frame list / place list / times"); return GLIO_E_ARG; }
    PL_CHECK(hipSetDevice(pl->v.device));
    { const int rw = pl_wait_upload(pl); if (rw != GLIO_OK) return rw; }
    pl->stamp += 1u;
    if (pl->stamp == 0u) { memset(pl->h_stamp, 0, (size_t)pl->o.max_places * sizeof(unsigned)); pl->stamp = 1u; }
    for (int f = 0; f < n; ++f) {
        const int k = frame_idx[f], p = place_idx[f];
        if (k < 0 || k >= pl->v.K) { glio_set_error("glio_place_add_frames: frame %d outside [0, %d)", k, pl->v.K); return GLIO_E_ARG; }
        if (p < 0 || p >= pl->o.max_places) { glio_set_error("glio_place_add_frames: place %d outside [0, %d)", p, pl->o.max_places); return GLIO_E_ARG; }
        const int nk = pl->v.h_n[k];
        if (nk < 1) { glio_set_error("glio_place_add_frames: frame %d was never set (or holds no point)", k); return GLIO_E_ARG; }
        if (!pl_finite(times[f])) { glio_set_error("glio_place_add_frames: time %d is not finite", f); return GLIO_E_ARG; }
        if (pl->h_stamp[p] == pl->stamp) { glio_set_error("glio_place_add_frames: place %d twice in one call", p); return GLIO_E_ARG; }
        pl->h_stamp[p] = pl->stamp;
        PlFrame& fr = pl->h_fr[f];
        if (!pl_level_matrix(level_q ? level_q + 4 * f : nullptr, fr.R)) { glio_set_error("glio_place_add_frames: quaternion %d is not finite (or zero)", f); return GLIO_E_ARG; }
        fr.src = pl->v.d_local + (size_t)k * pl->v.cap; fr.n = nk; fr.place = p; fr.pad_ = 0; fr.time = times[f];
    }
    hipStream_t s = pl->stream;
    // the owner's pending frame copies come first -- for this stream, not for the host
    PL_CHECK(hipEventRecord(pl->ev_dep, pl->v.stream));
    PL_CHECK(hipStreamWaitEvent(s, pl->ev_dep, 0));
    PL_CHECK(hipEventRecord(pl->ev_t0, s));
    PL_CHECK(hipMemcpyAsync(pl->d_fr, pl->h_fr, (size_t)n * sizeof(PlFrame), hipMemcpyHostToDevice, s));
    PL_CHECK(hipEventRecord(pl->ev_up, s));
    pl->up_pending = 1;
    hipLaunchKernelGGL(k_pl_describe, dim3(n), dim3(256), 0, s, pl->d_fr, pl->tab, pl->o.lidar_height, pl->d_h, pl->d_mask, pl->d_pmask, pl->d_u, pl->d_time, pl->d_valid);
    PL_CHECK(hipGetLastError());
    PL_CHECK(hipEventRecord(pl->ev_t1, s));
    // the owner's next write to one of these frames comes behind this read
    { const int re = pl->owner_d ? glio_dense_external_read(pl->owner_d, s) : glio_bassoc_external_read(pl->owner_b, s); if (re != GLIO_OK) return re; }
    for (int f = 0; f < n; ++f) {
        const int p = place_idx[f];
        pl->h_valid[p] = 1; pl->h_time[p] = times[f];
        if (p + 1 > pl->n_hi) pl->n_hi = p + 1;
    }
    pl->have_ms = 1;
    return GLIO_OK;
}

int glio_place_read_descriptor(glio_place* pl, int place, float* heights, uint64_t* mask, double* time, int32_t* valid) {
    if (!pl || place < 0 || place >= pl->o.max_places) { glio_set_error("glio_place_read_descriptor: place out of range"); return GLIO_E_ARG; }
    const int ok = pl->h_valid[place];
    if (valid) *valid = ok;
    if (time) *time = ok ? pl->h_time[place] : 0.0;
    if (!ok) {
        if (heights) memset(heights, 0, PL_CELLS * 4);
        if (mask) *mask = 0;
        return GLIO_OK;
    }
    PL_CHECK(hipSetDevice(pl->v.device));
    PL_CHECK(hipStreamSynchronize(pl->stream));
    if (heights) PL_CHECK(hipMemcpy(heights, pl->d_h + (size_t)place * PL_CELLS, PL_CELLS * 4, hipMemcpyDeviceToHost));
    if (mask) { pl_u64 m = 0; PL_CHECK(hipMemcpy(&m, pl->d_mask + place, 8, hipMemcpyDeviceToHost)); *mask = (uint64_t)m; }
    return GLIO_OK;
}

int glio_place_set_descriptor(glio_place* pl, int place, const float* heights, uint64_t mask, double time) {
    if (!pl || !heights) return GLIO_E_ARG;
    if (place < 0 || place >= pl->o.max_places) { glio_set_error("glio_place_set_descriptor: place %d outside [0, %d)", place, pl->o.max_places); return GLIO_E_ARG; }
    if ((mask & ~(uint64_t)PL_MASK60) != 0 || !pl_finite(time)) { glio_set_error("glio_place_set_descriptor: a mask bit above 59 or a time that is not finite"); return GLIO_E_ARG; }
    for (int c = 0; c < PL_CELLS; ++c) if (!(fabsf(heights[c]) <= FLT_MAX)) { glio_set_error("glio_place_set_descriptor: height %d is not finite", c); return GLIO_E_ARG; }
    PL_CHECK(hipSetDevice(pl->v.device));
    hipStream_t s = pl->stream;
    const pl_u64 m = (pl_u64)mask;
    PL_CHECK(hipMemcpyAsync(pl->d_h + (size_t)place * PL_CELLS, heights, PL_CELLS * 4, hipMemcpyHostToDevice, s));
    PL_CHECK(hipMemcpyAsync(pl->d_mask + place, &m, 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pl_normalise, dim3(1), dim3(64), 0, s, place, time, pl->d_h, pl->d_mask, pl->d_pmask, pl->d_u, pl->d_time, pl->d_valid);
    PL_CHECK(hipGetLastError());
    PL_CHECK(hipStreamSynchronize(s));                  // the caller's buffers may be reused after return
    pl->h_valid[place] = 1; pl->h_time[place] = time;
    if (place + 1 > pl->n_hi) pl->n_hi = place + 1;
    return GLIO_OK;
}

int glio_place_clear(glio_place* pl) {
    if (!pl) return GLIO_E_ARG;
    PL_CHECK(hipSetDevice(pl->v.device));
    PL_CHECK(hipMemsetAsync(pl->d_valid, 0, (size_t)pl->o.max_places * 4, pl->stream));
    memset(pl->h_valid, 0, (size_t)pl->o.max_places);
    pl->n_hi = 0;
    return GLIO_OK;
}

static int pl_query(glio_place* pl, const char* who, int first, int n, double min_time_gap, int earlier_only, int top_k, glio_place_match* matches, int32_t* n_found) {
    if (top_k < 1 || top_k > pl->o.top_k_max) { glio_set_error("%s: top_k %d outside [1, %d]", who, top_k, pl->o.top_k_max); return GLIO_E_ARG; }
    if (!(min_time_gap >= 0.0) || !pl_finite(min_time_gap)) { glio_set_error("%s: min_time_gap is negative or not finite", who); return GLIO_E_ARG; }
    PL_CHECK(hipSetDevice(pl->v.device));
    // a query beyond the highest place ever set is not valid and finds nothing: the kernels see the places below n_hi only
    const int P = pl->n_hi, nq = first + n <= P ? n : (first < P ? P - first : 0);
    for (int i = nq; i < n; ++i) n_found[i] = 0;
    if (nq == 0) return GLIO_OK;
    hipStream_t s = pl->stream;
    PL_CHECK(hipEventRecord(pl->ev_t0, s));
    size_t per = pl->pair_cap / (size_t)P;
    if (per > 32768) per = 32768;
    const int chunk = (int)per;                          // >= 1: pair_cap >= max_places >= P
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int m = nq - q0 < chunk ? nq - q0 : chunk;
        hipLaunchKernelGGL(k_pl_pairs, dim3((P + PL_RUN - 1) / PL_RUN, m), dim3(64), 0, s, pl->d_u, pl->d_pmask, pl->d_time, pl->d_valid, first + q0, P, min_time_gap,
                           earlier_only ? 1 : 0, pl->d_pair);
        hipLaunchKernelGGL(k_pl_select, dim3(m), dim3(256), 0, s, pl->d_pair, P, top_k, q0, pl->d_match, pl->d_nfound);
    }
    PL_CHECK(hipGetLastError());
    PL_CHECK(hipEventRecord(pl->ev_t1, s));
    PL_CHECK(hipMemcpyAsync(pl->h_match, pl->d_match, (size_t)nq * top_k * sizeof(glio_place_match), hipMemcpyDeviceToHost, s));
    PL_CHECK(hipMemcpyAsync(pl->h_nfound, pl->d_nfound, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    PL_CHECK(hipEventRecord(pl->ev_done, s));
    PL_CHECK(hipEventSynchronize(pl->ev_done));
    pl->have_ms = 1;
    for (int i = 0; i < nq; ++i) {
        const int nf = pl->h_nfound[i];
        n_found[i] = nf;
        for (int r = 0; r < nf; ++r) matches[(size_t)i * top_k + r] = pl->h_match[(size_t)i * top_k + r];
    }
    return GLIO_OK;
}
int glio_place_query(glio_place* pl, int place, double min_time_gap, int top_k, glio_place_match* matches, int32_t* n_found) {
    GLIO_TRACE("glio_place_query");
    if (!pl || !matches || !n_found) return GLIO_E_ARG;
    if (place < 0 || place >= pl->o.max_places || !pl->h_valid[place]) { glio_set_error("glio_place_query: place %d is out of range or not valid", place); return GLIO_E_ARG; }
    return pl_query(pl, "glio_place_query", place, 1, min_time_gap, 0, top_k, matches, n_found);
}
int glio_place_query_many(glio_place* pl, int first, int n, double min_time_gap, int earlier_only, int top_k, glio_place_match* matches, int32_t* n_found) {
    GLIO_TRACE("glio_place_query_many");
    if (!pl || !matches || !n_found) return GLIO_E_ARG;
    if (first < 0 || n < 1 || (long long)first + n > (long long)pl->o.max_places) { glio_set_error("glio_place_query_many: places [%d, %d + %d) outside [0, %d)", first, first, n, pl->o.max_places); return GLIO_E_ARG; }
    return pl_query(pl, "glio_place_query_many", first, n, min_time_gap, earlier_only, top_k, matches, n_found);
}

int glio_place_last_device_ms(glio_place* pl, float* ms) {
    if (!pl || !ms) return GLIO_E_ARG;
    if (!pl->have_ms) { glio_set_error("glio_place_add_frames or a query first"); return GLIO_E_STATE; }
    PL_CHECK(hipSetDevice(pl->v.device));
    PL_CHECK(hipEventSynchronize(pl->ev_t1));
    PL_CHECK(hipEventElapsedTime(ms, pl->ev_t0, pl->ev_t1));
    return GLIO_OK;
}

}  // extern "C"

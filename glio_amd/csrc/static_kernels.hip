// static_kernels.hip -- the static map on the device (include/glio_static.h): range images of resident frames, the visibility votes of every point against
// its views, and the order-preserving compaction of the points that were not seen through.  The rules are stated in the header; they are the library's own
// (UNPINNED) and restated in numpy by the tests.
//
// Images.  LDS path (k_st_image_lds): one workgroup of 1024 threads per frame of the call; the cells live in dynamic LDS as the float's bits (all values are
// positive: the integer order is the float order), a point enters with an integer atomic min, and behind a barrier the same workgroup writes the raw image and
// the floor image -- each once, no global atomic.  Global path (k_st_fill, k_st_image_glb, k_st_floor_glb): the same cells in a global work buffer.
// Votes (k_st_votes): one thread per point loops over the frame's views.  The point is read once, the two counts stay in registers, the 3 x 4 transform and the
// view index are uniform over the workgroup (scalar loads), the two tables sit in LDS (3 KB at the default size) and the one gather per (point, view) goes to
// the view's floor image, which the L2 serves: a frame's views are the same few images for every one of its workgroups.
// Compaction (k_st_compact): one workgroup per frame walks the frame in runs of 256 points; a ballot and four wavefront totals give every kept point its place.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "glio_device.h"
#include "../../include/glio_static.h"

// every product and sum rounds on its own, as the float32 restatement's do
#pragma clang fp contract(off)

#define ST_EMPTY 0x7fffffff                                /* no cell value (a finite positive float) has these bits */
#define ST_IMG_THREADS 1024

struct StGeom { int rows, cpq, cols, cells, nb; float min2, max2, g2, m2; };
struct StFrame { const float4* src; int n, k, voff, nv; };

struct glio_static {
    GlioBassocView v;
    glio_bassoc* owner_b; glio_dense* owner_d;
    glio_static_opts o;
    StGeom g;
    int tab_n, lds_path; size_t lds_bytes;
    float* h_tab; float* d_tab;                            // s2 [rows + 1] | dir [cols][2]
    hipStream_t stream;
    hipEvent_t ev_dep, ev_done, ev_t[5];
    hipEvent_t ev_ext_read; int ext_read_pending;          // a map's stream is still READING the static store: the next classify comes behind this event
    float4* d_store; unsigned char* d_through; unsigned char* d_tested;
    float* d_raw; float* d_floor; int* d_work;             // [K][cells]; d_work: the global path's cells
    StFrame* h_fr; StFrame* d_fr; float* h_T; float* d_T; int* h_views; int* d_views;
    int* d_res; int* h_res;                                // [3 K]: kept, tested, dynamic per call-local frame
    int* h_n;                                              // [K] sizes of the static frames (0: never classified), what a map's view reads
    int* h_votes_n;                                        // [K] points the votes of frame k cover
    unsigned* h_stamp; unsigned stamp;
    int n_last, have_ms;
};

// ---- rule 2: the cell of a point, or -1 when it is skipped; r2 is its squared range.  s2 [rows + 1], dir [cols][2]
__device__ __forceinline__ int st_cell_of(const StGeom& g, const float* __restrict__ s2, const float* __restrict__ dir, const float x, const float y, const float z,
                                          float& r2) {
    if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) return -1;
    const float rho2 = (x * x) + (y * y);
    r2 = rho2 + (z * z);
    if (rho2 == 0.f || !(r2 >= g.min2 && r2 < g.max2)) return -1;
    const float a = z * fabsf(z);
    if (!((s2[0] * rho2) <= a && a < (s2[g.rows] * rho2))) return -1;
    int lo = 0, hi = g.rows;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((s2[mid] * rho2) <= a) lo = mid; else hi = mid;
    }
    const int row = lo;
    const int q = (x > 0.f && y >= 0.f) ? 0 : (x <= 0.f && y > 0.f) ? 1 : (x < 0.f && y <= 0.f) ? 2 : 3;
    lo = 0; hi = g.cpq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const float dx = dir[2 * (q * g.cpq + mid)], dy = dir[2 * (q * g.cpq + mid) + 1];
        if (((dx * y) - (dy * x)) >= 0.f) lo = mid; else hi = mid;
    }
    return row * g.cols + (q * g.cpq + lo);               // (row < rows, column < cols by construction)
}
// ---- rule 3 over the cells as bits (ST_EMPTY: no point)
__device__ __forceinline__ float st_floor_at(const StGeom& g, const int* cell, const int r, const int c) {
    int m = ST_EMPTY;
    for (int dr = -g.nb; dr <= g.nb; ++dr) {
        const int rr = r + dr;
        if (rr < 0 || rr >= g.rows) return 0.f;
        for (int dc = -g.nb; dc <= g.nb; ++dc) {
            int cc = c + dc;
            cc = cc < 0 ? cc + g.cols : (cc >= g.cols ? cc - g.cols : cc);
            const int vv = cell[rr * g.cols + cc];
            if (vv == ST_EMPTY) return 0.f;
            m = min(m, vv);
        }
    }
    return __int_as_float(m);
}

__global__ __launch_bounds__(ST_IMG_THREADS) void k_st_image_lds(const StFrame* __restrict__ frames, const float* __restrict__ tab, const StGeom g, const int tab_n,
                                                                 float* __restrict__ raw, float* __restrict__ floor_img) {
    extern __shared__ __attribute__((aligned(16))) int st_smem[];
    int* s_cell = st_smem;
    float* s_tab = reinterpret_cast<float*>(st_smem + g.cells);
    const StFrame f = frames[blockIdx.x];
    const int tid = threadIdx.x;
    for (int c = tid; c < g.cells; c += ST_IMG_THREADS) s_cell[c] = ST_EMPTY;
    for (int k = tid; k < tab_n; k += ST_IMG_THREADS) s_tab[k] = tab[k];
    __syncthreads();
    const float* s2 = s_tab; const float* dir = s_tab + g.rows + 1;
    for (int i = tid; i < f.n; i += ST_IMG_THREADS) {
        const float4 p = f.src[i];
        float r2;
        const int c = st_cell_of(g, s2, dir, p.x, p.y, p.z, r2);
        if (c >= 0) atomicMin(&s_cell[c], __float_as_int(r2));
    }
    __syncthreads();
    float* ro = raw + (size_t)blockIdx.x * g.cells; float* fo = floor_img + (size_t)blockIdx.x * g.cells;
    for (int c = tid; c < g.cells; c += ST_IMG_THREADS) {
        const int vv = s_cell[c];
        ro[c] = vv == ST_EMPTY ? 0.f : __int_as_float(vv);
        fo[c] = st_floor_at(g, s_cell, c / g.cols, c % g.cols);
    }
}
// the global path: n * cells work cells
__global__ __launch_bounds__(256) void k_st_fill(int* __restrict__ work, const size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) work[i] = ST_EMPTY;
}
__global__ __launch_bounds__(256) void k_st_image_glb(const StFrame* __restrict__ frames, const float* __restrict__ tab, const StGeom g, const int tab_n,
                                                      int* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) int st_smem[];
    float* s_tab = reinterpret_cast<float*>(st_smem);
    const StFrame f = frames[blockIdx.y];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x * 256 >= f.n) return;               // (uniform over the workgroup)
    for (int k = tid; k < tab_n; k += 256) s_tab[k] = tab[k];
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + tid;
    if (i >= f.n) return;
    const float4 p = f.src[i];
    float r2;
    const int c = st_cell_of(g, s_tab, s_tab + g.rows + 1, p.x, p.y, p.z, r2);
    if (c >= 0) atomicMin(&work[(size_t)blockIdx.y * g.cells + c], __float_as_int(r2));
}
__global__ __launch_bounds__(256) void k_st_floor_glb(const int* __restrict__ work, const StGeom g, float* __restrict__ raw, float* __restrict__ floor_img) {
    const int c = (int)blockIdx.x * 256 + threadIdx.x;
    if (c >= g.cells) return;
    const int* cell = work + (size_t)blockIdx.y * g.cells;
    const int vv = cell[c];
    raw[(size_t)blockIdx.y * g.cells + c] = vv == ST_EMPTY ? 0.f : __int_as_float(vv);
    floor_img[(size_t)blockIdx.y * g.cells + c] = st_floor_at(g, cell, c / g.cols, c % g.cols);
}

// ---- rules 4, 5: the counts of every point of every frame of the call
__global__ __launch_bounds__(256) void k_st_votes(const StFrame* __restrict__ frames, const int* __restrict__ views, const float* __restrict__ T,
                                                  const float* __restrict__ tab, const StGeom g, const int tab_n, const float* __restrict__ floor_img, const int cap,
                                                  unsigned char* __restrict__ through, unsigned char* __restrict__ tested) {
    extern __shared__ __attribute__((aligned(16))) int st_smem[];
    float* s_tab = reinterpret_cast<float*>(st_smem);
    const StFrame f = frames[blockIdx.y];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x * 256 >= f.n) return;               // (uniform over the workgroup)
    for (int k = tid; k < tab_n; k += 256) s_tab[k] = tab[k];
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + tid;
    if (i >= f.n) return;
    const float* s2 = s_tab; const float* dir = s_tab + g.rows + 1;
    const float4 p = f.src[i];
    int th = 0, te = 0;
    for (int j = 0; j < f.nv; ++j) {
        const int v = views[f.voff + j];                    // (0 <= v < n: the host's check)
        const float* M = T + 12 * (size_t)(f.voff + j);
        const float x = (((M[0] * p.x) + (M[1] * p.y)) + (M[2] * p.z)) + M[3];
        const float y = (((M[4] * p.x) + (M[5] * p.y)) + (M[6] * p.z)) + M[7];
        const float z = (((M[8] * p.x) + (M[9] * p.y)) + (M[10] * p.z)) + M[11];
        float r2;
        const int c = st_cell_of(g, s2, dir, x, y, z, r2);
        if (c < 0) continue;
        const float F = floor_img[(size_t)v * g.cells + c];
        if (F > 0.f) {
            te += 1;
            if (F > ((g.g2 * r2) + g.m2)) th += 1;
        }
    }
    through[(size_t)f.k * cap + i] = (unsigned char)th;     // (i < f.n <= cap, f.k < K)
    tested[(size_t)f.k * cap + i] = (unsigned char)te;
}

// ---- rule 6: the kept points in their order; res [3 n]: kept, tested, dynamic of the call-local frame
__global__ __launch_bounds__(256) void k_st_compact(const StFrame* __restrict__ frames, const unsigned char* __restrict__ through, const unsigned char* __restrict__ tested,
                                                    const int min_votes, const int cap, float4* __restrict__ store, int* __restrict__ res) {
    __shared__ int s_w[4];
    __shared__ int s_te;
    const StFrame f = frames[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_te = 0;
    const unsigned char* th = through + (size_t)f.k * cap; const unsigned char* te = tested + (size_t)f.k * cap;
    float4* dst = store + (size_t)f.k * cap;
    int base = 0, nte = 0;
    for (int i0 = 0; i0 < f.n; i0 += 256) {
        const int i = i0 + tid;
        const bool in = i < f.n;
        const bool keep = in && (int)th[in ? i : 0] < min_votes;
        nte += (in && te[i] > 0) ? 1 : 0;
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();                                    // (the previous run's totals have been read)
        if (lane == 0) s_w[w] = __popcll(b);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { off += k < w ? s_w[k] : 0; tot += s_w[k]; }
        if (keep) dst[base + off + before] = f.src[i];      // (base + off + before < f.n <= cap)
        base += tot;
    }
    if (nte) atomicAdd(&s_te, nte);                         // (an integer sum)
    __syncthreads();
    if (tid == 0) { res[3 * blockIdx.x] = base; res[3 * blockIdx.x + 1] = s_te; res[3 * blockIdx.x + 2] = f.n - base; }
}

#define ST_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

static bool st_finite(const double v) { return fabs(v) <= DBL_MAX; }
static bool st_opts_ok(const glio_static_opts& o) {
    return o.rows >= 1 && o.rows <= GLIO_STATIC_MAX_ROWS && o.cols_per_quadrant >= 1 && o.cols_per_quadrant <= GLIO_STATIC_MAX_COLS_PER_QUADRANT &&
           (o.neighbourhood == 0 || o.neighbourhood == 1) && o.max_views >= 1 && o.max_views <= GLIO_STATIC_MAX_VIEWS && o.min_votes >= 1 && o.min_votes <= o.max_views &&
           (o.image_path == GLIO_STATIC_PATH_AUTO || o.image_path == GLIO_STATIC_PATH_GLOBAL) && o.elev_min_deg >= -89.f && o.elev_max_deg <= 89.f &&
           o.elev_min_deg < o.elev_max_deg && o.min_range > 0.f && o.max_range > o.min_range && o.max_range <= 1e18f && o.range_gain >= 0.f && o.range_gain <= 1e18f &&
           o.range_margin >= 0.f && o.range_margin <= 1e18f;
}
static void st_tables(const glio_static_opts& o, float* s2, float* dir) {
    for (int k = 0; k <= o.rows; ++k) {
        const double e = (double)o.elev_min_deg + (((double)o.elev_max_deg - (double)o.elev_min_deg) * (double)k) / (double)o.rows;
        const double t = tan((e * 3.141592653589793) / 180.0);
        s2[k] = (float)(t * fabs(t));
    }
    const int cols = 4 * o.cols_per_quadrant;
    for (int s = 0; s < cols; ++s) {
        const double a = (6.283185307179586 * (double)s) / (double)cols;
        dir[2 * s] = (float)cos(a); dir[2 * s + 1] = (float)sin(a);
    }
}
// the rotation matrix of q / |q| (w first) in double; false: q is not finite or zero
static bool st_rotation(const double* q, double* m) {
    for (int k = 0; k < 4; ++k) if (!st_finite(q[k])) return false;
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    if (!(n > 0.0) || !st_finite(n)) return false;
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    m[0] = 1.0 - 2.0 * (y * y + z * z); m[1] = 2.0 * (x * y - w * z); m[2] = 2.0 * (x * z + w * y);
    m[3] = 2.0 * (x * y + w * z); m[4] = 1.0 - 2.0 * (x * x + z * z); m[5] = 2.0 * (y * z - w * x);
    m[6] = 2.0 * (x * z - w * y); m[7] = 2.0 * (y * z + w * x); m[8] = 1.0 - 2.0 * (x * x + y * y);
    return true;
}
static bool st_pose_ok(const double* p) {
    double m[9];
    for (int k = 0; k < 3; ++k) if (!st_finite(p[k])) return false;
    return st_rotation(p + 3, m);
}
static bool st_relative_pose(const double* pv, const double* pf, float* T) {
    double Rv[9], Rf[9];
    for (int k = 0; k < 3; ++k) if (!st_finite(pv[k]) || !st_finite(pf[k])) return false;
    if (!st_rotation(pv + 3, Rv) || !st_rotation(pf + 3, Rf)) return false;
    const double d[3] = {pf[0] - pv[0], pf[1] - pv[1], pf[2] - pv[2]};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)((Rv[i] * Rf[j] + Rv[3 + i] * Rf[3 + j]) + Rv[6 + i] * Rf[6 + j]);
        T[4 * i + 3] = (float)((Rv[i] * d[0] + Rv[3 + i] * d[1]) + Rv[6 + i] * d[2]);
    }
    return true;
}

int glio_static_view(glio_static* st, GlioBassocView* out) {
    if (!st || !out) return GLIO_E_ARG;
    out->device = st->v.device; out->K = st->v.K; out->cap = st->v.cap; out->d_local = st->d_store; out->h_n = st->h_n; out->stream = st->stream;
    return GLIO_OK;
}
int glio_static_external_read(glio_static* st, hipStream_t reader) {
    if (st->ext_read_pending) GLIO_HIP_CHECK(hipStreamWaitEvent(reader, st->ev_ext_read, 0));      // (another map's read: the new record covers it)
    GLIO_HIP_CHECK(hipEventRecord(st->ev_ext_read, reader));
    st->ext_read_pending = 1;
    return GLIO_OK;
}

extern "C" {

void glio_static_opts_default(glio_static_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->rows = 44; o->cols_per_quadrant = 90; o->neighbourhood = 1; o->min_votes = 2; o->max_views = 16; o->image_path = GLIO_STATIC_PATH_AUTO;
    o->elev_min_deg = -31.0f; o->elev_max_deg = 13.0f; o->min_range = 1.0f; o->max_range = 80.0f; o->range_gain = 1.05f; o->range_margin = 0.3f;
}
int glio_static_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_static_opts), (int32_t)sizeof(glio_static_info)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}
int glio_static_tables(const glio_static_opts* opts, float* s2, float* dir) {
    if (!opts || !s2 || !dir || !st_opts_ok(*opts)) { glio_set_error("glio_static_tables: options out of range / null pointer"); return GLIO_E_ARG; }
    st_tables(*opts, s2, dir);
    return GLIO_OK;
}
int glio_static_relative_pose(const double* pose_v, const double* pose_f, float* T) {
    if (!pose_v || !pose_f || !T) { glio_set_error("glio_static_relative_pose: null pointer"); return GLIO_E_ARG; }
    float m[12];
    if (!st_relative_pose(pose_v, pose_f, m)) { glio_set_error("glio_static_relative_pose: a pose is not finite (or its quaternion zero)"); return GLIO_E_ARG; }
    memcpy(T, m, sizeof m);
    return GLIO_OK;
}

void glio_static_destroy(glio_static* st) {
    if (!st) return;
    hipSetDevice(st->v.device);
    if (st->stream) hipStreamSynchronize(st->stream);
    if (st->ext_read_pending && st->ev_ext_read) hipEventSynchronize(st->ev_ext_read);
    void* p[] = {st->d_tab, st->d_store, st->d_through, st->d_tested, st->d_raw, st->d_floor, st->d_work, st->d_fr, st->d_T, st->d_views, st->d_res};
    for (void* q : p) if (q) hipFree(q);
    void* h[] = {st->h_fr, st->h_T, st->h_views, st->h_res};
    for (void* q : h) if (q) hipHostFree(q);
    hipEvent_t ev[] = {st->ev_dep, st->ev_done, st->ev_ext_read, st->ev_t[0], st->ev_t[1], st->ev_t[2], st->ev_t[3], st->ev_t[4]};
    for (hipEvent_t e : ev) if (e) hipEventDestroy(e);
    if (st->stream) hipStreamDestroy(st->stream);
    delete[] st->h_tab; delete[] st->h_n; delete[] st->h_votes_n; delete[] st->h_stamp;
    delete st;
}

static int st_create_body(glio_static* st) {
    const size_t K = (size_t)st->v.K, cap = (size_t)st->v.cap, cells = (size_t)st->g.cells, nv = K * (size_t)st->o.max_views;
    ST_CHECK(hipSetDevice(st->v.device));
    ST_CHECK(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    ST_CHECK(hipEventCreateWithFlags(&st->ev_dep, hipEventDisableTiming));
    ST_CHECK(hipEventCreateWithFlags(&st->ev_ext_read, hipEventDisableTiming));
    ST_CHECK(hipEventCreateWithFlags(&st->ev_done, hipEventDisableTiming | hipEventBlockingSync));
    for (int k = 0; k < 5; ++k) ST_CHECK(hipEventCreate(&st->ev_t[k]));
    ST_CHECK(hipMalloc((void**)&st->d_tab, (size_t)st->tab_n * 4));
    ST_CHECK(hipMalloc((void**)&st->d_store, K * cap * 16)); ST_CHECK(hipMalloc((void**)&st->d_through, K * cap)); ST_CHECK(hipMalloc((void**)&st->d_tested, K * cap));
    ST_CHECK(hipMalloc((void**)&st->d_raw, K * cells * 4)); ST_CHECK(hipMalloc((void**)&st->d_floor, K * cells * 4));
    if (!st->lds_path) ST_CHECK(hipMalloc((void**)&st->d_work, K * cells * 4));
    ST_CHECK(hipMalloc((void**)&st->d_fr, K * sizeof(StFrame))); ST_CHECK(hipHostMalloc((void**)&st->h_fr, K * sizeof(StFrame)));
    ST_CHECK(hipMalloc((void**)&st->d_T, nv * 48)); ST_CHECK(hipHostMalloc((void**)&st->h_T, nv * 48));
    ST_CHECK(hipMalloc((void**)&st->d_views, nv * 4)); ST_CHECK(hipHostMalloc((void**)&st->h_views, nv * 4));
    ST_CHECK(hipMalloc((void**)&st->d_res, K * 12)); ST_CHECK(hipHostMalloc((void**)&st->h_res, K * 12));
    ST_CHECK(hipMemcpyAsync(st->d_tab, st->h_tab, (size_t)st->tab_n * 4, hipMemcpyHostToDevice, st->stream));
    ST_CHECK(hipMemsetAsync(st->d_store, 0, K * cap * 16, st->stream));
    ST_CHECK(hipMemsetAsync(st->d_through, 0, K * cap, st->stream)); ST_CHECK(hipMemsetAsync(st->d_tested, 0, K * cap, st->stream));
    if (st->lds_path)                                       // (beyond 64 KB the dynamic LDS has to be asked for)
        ST_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_st_image_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)st->lds_bytes));
    st->h_n = new int[K](); st->h_votes_n = new int[K](); st->h_stamp = new unsigned[K]();
    ST_CHECK(hipStreamSynchronize(st->stream));
    return GLIO_OK;
}
static int st_create(glio_bassoc* b, glio_dense* d, const glio_static_opts* opts, glio_static** out) {
    if ((!b && !d) || !opts || !out) return GLIO_E_ARG;
    const glio_static_opts& o = *opts;
    if (!st_opts_ok(o)) {
        glio_set_error("bad glio_static_opts (rows %d, cols_per_quadrant %d, neighbourhood %d, min_votes %d, max_views %d, image_path %d, elevation %g .. %g, range %g .. %g, "
                       "gain %g, margin %g)", o.rows, o.cols_per_quadrant, o.neighbourhood, o.min_votes, o.max_views, o.image_path, (double)o.elev_min_deg,
                       (double)o.elev_max_deg, (double)o.min_range, (double)o.max_range, (double)o.range_gain, (double)o.range_margin);
        return GLIO_E_ARG;
    }
    glio_static* st = new glio_static();
    memset(st, 0, sizeof *st);
    st->o = o;
    st->owner_b = b; st->owner_d = d;
    StGeom& g = st->g;
    g.rows = o.rows; g.cpq = o.cols_per_quadrant; g.cols = 4 * o.cols_per_quadrant; g.cells = g.rows * g.cols; g.nb = o.neighbourhood;
    g.min2 = (float)((double)o.min_range * (double)o.min_range); g.max2 = (float)((double)o.max_range * (double)o.max_range);
    g.g2 = (float)((double)o.range_gain * (double)o.range_gain); g.m2 = (float)((double)o.range_margin * (double)o.range_margin);
    st->tab_n = g.rows + 1 + 2 * g.cols;
    st->lds_bytes = 4 * (size_t)g.cells + 4 * (size_t)st->tab_n;
    st->lds_path = o.image_path == GLIO_STATIC_PATH_AUTO && st->lds_bytes <= (size_t)GLIO_STATIC_LDS_LIMIT;
    st->h_tab = new float[st->tab_n];
    st_tables(o, st->h_tab, st->h_tab + g.rows + 1);
    { const int rv = d ? glio_dense_view(d, &st->v) : glio_bassoc_view(b, &st->v); if (rv != GLIO_OK) { delete[] st->h_tab; delete st; return rv; } }
    const int rc = st_create_body(st);
    if (rc != GLIO_OK) { glio_static_destroy(st); return rc; }
    *out = st;
    return GLIO_OK;
}
int glio_static_create(glio_bassoc* b, const glio_static_opts* opts, glio_static** out) { return st_create(b, nullptr, opts, out); }
int glio_static_create_on_dense(glio_dense* d, const glio_static_opts* opts, glio_static** out) { return st_create(nullptr, d, opts, out); }

int glio_static_classify(glio_static* st, int n, const int32_t* frame_idx, const double* poses, const int32_t* view_offsets, const int32_t* views,
                         glio_static_info* info) {
    GLIO_TRACE("glio_static_classify");
    if (!st) return GLIO_E_ARG;
    const int K = st->v.K, cap = st->v.cap;
    if (n < 1 || n > K) { glio_set_error("glio_static_classify: %d frames, a call takes 1 .. %d", n, K); return GLIO_E_ARG; }
    if (!frame_idx || !poses || !view_offsets) { glio_set_error("glio_static_classify: null frame list / poses / view offsets"); return GLIO_E_ARG; }
    if (view_offsets[0] != 0) { glio_set_error("glio_static_classify: view_offsets[0] is not 0"); return GLIO_E_ARG; }
    st->stamp += 1u;
    if (st->stamp == 0u) { memset(st->h_stamp, 0, (size_t)K * sizeof(unsigned)); st->stamp = 1u; }
    long long total = 0;
    int max_n = 0;
    for (int f = 0; f < n; ++f) {
        const int k = frame_idx[f];
        if (k < 0 || k >= K) { glio_set_error("glio_static_classify: frame %d outside [0, %d)", k, K); return GLIO_E_ARG; }
        const int nk = st->v.h_n[k];
        if (nk < 1 || nk > cap) { glio_set_error("glio_static_classify: frame %d was never set (or holds no point)", k); return GLIO_E_ARG; }
        if (st->h_stamp[k] == st->stamp) { glio_set_error("glio_static_classify: frame %d twice in one call", k); return GLIO_E_ARG; }
        st->h_stamp[k] = st->stamp;
        if (!st_pose_ok(poses + 7 * f)) { glio_set_error("glio_static_classify: pose %d is not finite (or its quaternion zero)", f); return GLIO_E_ARG; }
        const int v0 = view_offsets[f], v1 = view_offsets[f + 1];
        if (v1 < v0 || v1 - v0 > st->o.max_views) { glio_set_error("glio_static_classify: frame %d has %d views, 0 .. %d are taken", f, v1 - v0, st->o.max_views); return GLIO_E_ARG; }
        if (v1 > v0 && !views) { glio_set_error("glio_static_classify: null view list"); return GLIO_E_ARG; }
        for (int j = v0; j < v1; ++j) {
            const int v = views[j];
            if (v < 0 || v >= n || v == f) { glio_set_error("glio_static_classify: view %d of frame %d is outside [0, %d) or the frame itself", v, f, n); return GLIO_E_ARG; }
        }
        StFrame& fr = st->h_fr[f];
        fr.src = st->v.d_local + (size_t)k * cap; fr.n = nk; fr.k = k; fr.voff = v0; fr.nv = v1 - v0;
        total += nk;
        if (nk > max_n) max_n = nk;
    }
    // (every pose of the call is fine: the relative poses cannot fail)
    const int nviews = view_offsets[n];
    for (int f = 0; f < n; ++f)
        for (int j = view_offsets[f]; j < view_offsets[f + 1]; ++j) {
            st->h_views[j] = views[j];
            st_relative_pose(poses + 7 * views[j], poses + 7 * f, st->h_T + 12 * (size_t)j);
        }
    ST_CHECK(hipSetDevice(st->v.device));
    hipStream_t s = st->stream;
    const StGeom g = st->g;
    const size_t tab_bytes = (size_t)st->tab_n * 4;
    // the owner's pending frame writes come first -- for this stream, not for the host; and a map that still reads the static store
    ST_CHECK(hipEventRecord(st->ev_dep, st->v.stream));
    ST_CHECK(hipStreamWaitEvent(s, st->ev_dep, 0));
    if (st->ext_read_pending) { ST_CHECK(hipStreamWaitEvent(s, st->ev_ext_read, 0)); st->ext_read_pending = 0; }
    ST_CHECK(hipMemcpyAsync(st->d_fr, st->h_fr, (size_t)n * sizeof(StFrame), hipMemcpyHostToDevice, s));
    if (nviews > 0) {
        ST_CHECK(hipMemcpyAsync(st->d_T, st->h_T, (size_t)nviews * 48, hipMemcpyHostToDevice, s));
        ST_CHECK(hipMemcpyAsync(st->d_views, st->h_views, (size_t)nviews * 4, hipMemcpyHostToDevice, s));
    }
    const int nblk = (max_n + 255) / 256;
    ST_CHECK(hipEventRecord(st->ev_t[0], s));
    if (st->lds_path) {
        hipLaunchKernelGGL(k_st_image_lds, dim3(n), dim3(ST_IMG_THREADS), st->lds_bytes, s, st->d_fr, st->d_tab, g, st->tab_n, st->d_raw, st->d_floor);
        ST_CHECK(hipEventRecord(st->ev_t[1], s));
    } else {
        const size_t nw = (size_t)n * g.cells;
        hipLaunchKernelGGL(k_st_fill, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, st->d_work, nw);
        hipLaunchKernelGGL(k_st_image_glb, dim3(nblk, n), dim3(256), tab_bytes, s, st->d_fr, st->d_tab, g, st->tab_n, st->d_work);
        ST_CHECK(hipEventRecord(st->ev_t[1], s));
        hipLaunchKernelGGL(k_st_floor_glb, dim3((g.cells + 255) / 256, n), dim3(256), 0, s, st->d_work, g, st->d_raw, st->d_floor);
    }
    ST_CHECK(hipEventRecord(st->ev_t[2], s));
    hipLaunchKernelGGL(k_st_votes, dim3(nblk, n), dim3(256), tab_bytes, s, st->d_fr, st->d_views, st->d_T, st->d_tab, g, st->tab_n, st->d_floor, cap, st->d_through,
                       st->d_tested);
    ST_CHECK(hipEventRecord(st->ev_t[3], s));
    hipLaunchKernelGGL(k_st_compact, dim3(n), dim3(256), 0, s, st->d_fr, st->d_through, st->d_tested, st->o.min_votes, cap, st->d_store, st->d_res);
    ST_CHECK(hipGetLastError());
    ST_CHECK(hipEventRecord(st->ev_t[4], s));
    // the owner's next write to one of these frames comes behind this read
    { const int re = st->owner_d ? glio_dense_external_read(st->owner_d, s) : glio_bassoc_external_read(st->owner_b, s); if (re != GLIO_OK) return re; }
    ST_CHECK(hipMemcpyAsync(st->h_res, st->d_res, (size_t)n * 12, hipMemcpyDeviceToHost, s));
    ST_CHECK(hipEventRecord(st->ev_done, s));
    ST_CHECK(hipEventSynchronize(st->ev_done));
    st->have_ms = 1; st->n_last = n;
    long long n_te = 0, n_dyn = 0;
    for (int f = 0; f < n; ++f) {
        const int k = frame_idx[f];
        st->h_n[k] = st->h_res[3 * f]; st->h_votes_n[k] = st->h_fr[f].n;
        n_te += st->h_res[3 * f + 1]; n_dyn += st->h_res[3 * f + 2];
    }
    if (info) { info->n_points = total; info->n_tested = n_te; info->n_dynamic = n_dyn; info->n_frames = n; info->lds_path = st->lds_path; }
    return GLIO_OK;
}

int glio_static_frame_count(glio_static* st, int k, int* n) {
    if (!st || !n || k < 0 || k >= st->v.K) { glio_set_error("glio_static_frame_count: frame out of range / null pointer"); return GLIO_E_ARG; }
    *n = st->h_n[k];
    return GLIO_OK;
}
int glio_static_read_frame(glio_static* st, int k, float* out_xyzi, int capacity, int* n) {
    if (!st || k < 0 || k >= st->v.K) { glio_set_error("glio_static_read_frame: frame out of range"); return GLIO_E_ARG; }
    const int nk = st->h_n[k];
    if (n) *n = nk;
    if (!out_xyzi) return GLIO_OK;
    if (capacity < nk) { glio_set_error("glio_static_read_frame: capacity %d < %d points", capacity, nk); return GLIO_E_ARG; }
    if (nk == 0) return GLIO_OK;
    ST_CHECK(hipSetDevice(st->v.device));
    ST_CHECK(hipStreamSynchronize(st->stream));
    ST_CHECK(hipMemcpy(out_xyzi, st->d_store + (size_t)k * st->v.cap, (size_t)nk * 16, hipMemcpyDeviceToHost));
    return GLIO_OK;
}
int glio_static_read_votes(glio_static* st, int k, uint8_t* through, uint8_t* tested, int capacity, int* n) {
    if (!st || k < 0 || k >= st->v.K) { glio_set_error("glio_static_read_votes: frame out of range"); return GLIO_E_ARG; }
    const int nk = st->h_votes_n[k];
    if (n) *n = nk;
    if (!through && !tested) return GLIO_OK;
    if (capacity < nk) { glio_set_error("glio_static_read_votes: capacity %d < %d points", capacity, nk); return GLIO_E_ARG; }
    if (nk == 0) return GLIO_OK;
    ST_CHECK(hipSetDevice(st->v.device));
    ST_CHECK(hipStreamSynchronize(st->stream));
    if (through) ST_CHECK(hipMemcpy(through, st->d_through + (size_t)k * st->v.cap, (size_t)nk, hipMemcpyDeviceToHost));
    if (tested) ST_CHECK(hipMemcpy(tested, st->d_tested + (size_t)k * st->v.cap, (size_t)nk, hipMemcpyDeviceToHost));
    return GLIO_OK;
}
int glio_static_read_image(glio_static* st, int view, float* raw, float* floor) {
    if (!st) return GLIO_E_ARG;
    if (!st->have_ms) { glio_set_error("glio_static_classify first"); return GLIO_E_STATE; }
    if (view < 0 || view >= st->n_last) { glio_set_error("glio_static_read_image: view %d outside the last call's [0, %d)", view, st->n_last); return GLIO_E_ARG; }
    ST_CHECK(hipSetDevice(st->v.device));
    ST_CHECK(hipStreamSynchronize(st->stream));
    const size_t cells = (size_t)st->g.cells;
    if (raw) ST_CHECK(hipMemcpy(raw, st->d_raw + (size_t)view * cells, cells * 4, hipMemcpyDeviceToHost));
    if (floor) ST_CHECK(hipMemcpy(floor, st->d_floor + (size_t)view * cells, cells * 4, hipMemcpyDeviceToHost));
    return GLIO_OK;
}
int glio_static_last_device_ms(glio_static* st, float ms[4]) {
    if (!st || !ms) return GLIO_E_ARG;
    if (!st->have_ms) { glio_set_error("glio_static_classify first"); return GLIO_E_STATE; }
    ST_CHECK(hipSetDevice(st->v.device));
    ST_CHECK(hipEventSynchronize(st->ev_t[4]));
    for (int k = 0; k < 4; ++k) ST_CHECK(hipEventElapsedTime(&ms[k], st->ev_t[k], st->ev_t[k + 1]));
    if (st->lds_path) ms[1] = 0.f;
    return GLIO_OK;
}

}  // extern "C"

// globalmap_kernels.hip -- the global map on the device (glio_gmap_*): mapVisualizationThread's save_pcd part and publishCompleteMap (reference
// GLIO/src/Estimator.cpp:5315-5350, :5275-5313): every mapping_interval-th keyframe's surf cloud moved to the world by transformCloud at its final pose, the moved
// clouds concatenated, ONE pcl::VoxelGrid at 0.2 m (ds_filter_global_map, :856) over the concatenation.  The clouds are the ones resident in a batch association;
// the rules are stated in include/glio_hip.h.
//
// pcl::VoxelGrid sorts the points by voxel index and sums each run; so does this file -- every contribution is stored once and summed per destination in a
// fixed order, no atomic takes part in a sum.  PCL's linear index ix + iy dx + iz dx dy orders the voxels lexicographically by (iz, iy, ix) whatever the bounding box
// is, so a 63-bit ABSOLUTE key (21 biased bits per axis, iz highest) gives PCL's output order without a bounding-box pass.  One call:
//   k_gm_transform    blockIdx.y = frame: transformCloud (cloud_transform), the point's key, its rank in the concatenation; the call's bounding box
//                     in voxel coordinates (for the sort's plan and the overflow flag), the range check of the key
//   k_gm_plan         the digits of the call.  The absolute key is biased, so a cloud that straddles a coordinate's zero differs in all 21 bits of that axis -- all
//                     eight digits would vary.  Inside ONE call the order of (iz, iy, ix) is also the order of the coordinates counted from the call's own
//                     minimum and packed without gaps: bits(extent x) + bits(extent y) + bits(extent z) bits, 24 for a 100 m x 100 m x 10 m call at 0.2 m --
//                     three digits instead of eight.  The plan (minima, field shifts, number of digits) stays on the device: no host wait before the sort.
//   the sort          stable least-significant-digit radix sort of (key, rank) on the 8-bit digits of that packed form (computed from the absolute key where
//                     it is needed, never stored); per digit k_gm_hist (one wavefront per tile of GM_SORT_TILE pairs), the scan of the [tile][digit] counts
//                     in (digit, tile) order by k_gm_scan_a / _b / _c (workgroups of GM_SCAN_CHUNK tiles; only the middle kernel, over one number per
//                     workgroup and digit, is a single workgroup) and k_gm_scatter (ballot ranking inside a chunk of 64: stable).  All eight digits are
//                     enqueued; the kernels of a digit the plan does not have return at once.
//   k_gm_runs         run heads of the sorted keys; per head the lookup of its key in the map's sorted voxel array; exclusive scan of "opens a new voxel" (the
//                     block totals by k_gm_runs_top, which also decides whether the map would outgrow max_voxels)
//   k_gm_accum        per run: the accumulator STARTS FROM THE STORED SUM of its voxel and takes the run's points one at a time in rank order -- the float the
//                     whole concatenation summed from the start would give, which old + (sum of new) is not.  Written at its place in the other voxel array.
//   k_gm_merge        the voxels of the old array that no run touched, moved to their place in the other array
// The call then waits for the stream once, reads the control block and either swaps the two voxel arrays or -- a refusal -- leaves the map exactly as it was.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "glio_device.h"
#include "cloud_device.h"
#include "../../include/glio_static.h"

// transformCloud and the voxel sums must round like scalar float / double code: no FMA contraction in this file
#pragma clang fp contract(off)

#define GM_SORT_TILE 1024       /* pairs per wavefront (= per workgroup) of k_gm_hist / k_gm_scatter */
#define GM_SCAN_CHUNK 64        /* tiles per workgroup of k_gm_scan_a / k_gm_scan_c */
#define GM_RUN_BLOCK 1024       /* points per workgroup of k_gm_runs (the block scan of the run flags) */
#define GM_TOP_THREADS 128      /* threads of k_gm_runs_top: each scans a contiguous chunk of the workgroup totals */
#define GM_TF_THREADS 256
#define GM_TF_PER 4             /* points per thread of k_gm_transform: a workgroup covers 1024 points of one frame */
#define GM_BIAS (1 << 20)
#define GM_MAX_FRAMES 65535     /* grid.y of k_gm_transform */

typedef float gm_v4f __attribute__((ext_vector_type(4)));
typedef unsigned long long gm_u64;

// one frame of a call: its own-frame cloud (resident in the batch association), its size, where it starts in the call's concatenation, transformCloud's pose
struct GmFrame { const float4* src; int n, off; double q[4], t[3]; };
struct GmCtl {
    int bb[6];                  // voxel coordinates of the call: min x y z, max x y z
    int sh_y, sh_z, npass;      // the sort's plan (k_gm_plan): the packed key is (ix - min x) | (iy - min y) << sh_y | (iz - min z) << sh_z, npass digits of 8 bits
    int pad_;
    int bad;                    // a voxel coordinate outside [-2^20, 2^20) (or not finite)
    int n_new, nv_new, over;    // runs that open a voxel; the map's size after the call; nv_new > max_voxels
};
struct GmVox { gm_u64* key; float4* sum; int* cnt; float4* out; };      // sorted by key: the float sums in concatenation order, the counts, the centroids

struct glio_gmap {
    GlioBassocView v;                   // the resident clouds: a batch association's keyframes, or a dense store's frames (glio_gmap_create_on_dense)
    glio_dense* dense;                  // the dense store the view is of (null: a batch association)
    glio_static* stat;                  // the static store the view is of (glio_gmap_create_on_static), or null
    glio_gmap_opts o;
    float inv_leaf;
    hipStream_t stream;
    hipEvent_t ev_dep, ev_done, ev_t[5];
    GmVox vox[2]; int cur, n_vox;
    long long n_points;
    int bb[6]; int have_bb;
    float4* d_pts; gm_u64* d_key[2]; unsigned* d_val[2];
    int* d_hist; int* d_csum; int* d_blk;
    GmCtl* d_ctl; GmCtl* h_ctl;
    GmFrame* d_frames; GmFrame* h_frames; int frames_cap;
    int have_ms;
};

__global__ void k_gm_begin(GmCtl* ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ctl->sh_y = 0; ctl->sh_z = 0; ctl->npass = 0; ctl->pad_ = 0;
    for (int a = 0; a < 3; ++a) { ctl->bb[a] = 0x7fffffff; ctl->bb[3 + a] = (int)0x80000000; }
    ctl->bad = 0; ctl->n_new = 0; ctl->nv_new = 0; ctl->over = 0;
}

__global__ __launch_bounds__(GM_TF_THREADS) void k_gm_transform(const GmFrame* __restrict__ fr, const float inv_leaf, float4* __restrict__ pts, gm_u64* __restrict__ key,
                                                                unsigned* __restrict__ val, GmCtl* ctl) {
    __shared__ int s_box[GM_TF_THREADS / 64 * 6];
    const GmFrame d = fr[blockIdx.y];                            // (uniform over the workgroup)
    const int base = blockIdx.x * (GM_TF_THREADS * GM_TF_PER);
    if (base >= d.n) return;                                     // (the whole workgroup: the grid is sized for the largest frame)
    CloudBox b;
    b.init();
    bool bad = false;
    float4 p[GM_TF_PER];
    // the clouds are read once: all of a thread's loads in flight together, past the caches' retention
#pragma unroll
    for (int k = 0; k < GM_TF_PER; ++k) {
        const int i = base + k * GM_TF_THREADS + (int)threadIdx.x;
        if (i < d.n) { const gm_v4f r = __builtin_nontemporal_load(reinterpret_cast<const gm_v4f*>(d.src + i)); p[k] = make_float4(r.x, r.y, r.z, r.w); }
    }
#pragma unroll
    for (int k = 0; k < GM_TF_PER; ++k) {
        const int i = base + k * GM_TF_THREADS + (int)threadIdx.x;
        if (i >= d.n) continue;
        const float4 g = cloud_transform(d.q, d.t, p[k]);
        const float f[3] = {floorf(g.x * inv_leaf), floorf(g.y * inv_leaf), floorf(g.z * inv_leaf)};
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const bool ok = f[a] >= -(float)GM_BIAS && f[a] < (float)GM_BIAS;          // (false for NaN)
            if (!ok) bad = true;
            c[a] = ok ? (int)f[a] : 0;
            b.add(a, c[a]);
        }
        const gm_u64 kk = ((gm_u64)(unsigned)(c[2] + GM_BIAS) << 42) | ((gm_u64)(unsigned)(c[1] + GM_BIAS) << 21) | (gm_u64)(unsigned)(c[0] + GM_BIAS);
        const size_t e = (size_t)d.off + (size_t)i;
        pts[e] = g; key[e] = kk; val[e] = (unsigned)e;
    }
    if (bad) atomicOr(&ctl->bad, 1);
    b.commit<GM_TF_THREADS / 64>(s_box, ctl->bb);
}
__global__ void k_gm_plan(GmCtl* ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || ctl->bad) return;         // (a refused call sorts nothing: npass stays 0)
    int bits[3];
    for (int a = 0; a < 3; ++a) { const unsigned ext = (unsigned)(ctl->bb[3 + a] - ctl->bb[a]); bits[a] = ext ? 32 - __clz((int)ext) : 0; }      // (ext < 2^21)
    ctl->sh_y = bits[0]; ctl->sh_z = bits[0] + bits[1];
    ctl->npass = (bits[0] + bits[1] + bits[2] + 7) / 8;
}

// ---- the sort.  The plan's packed key of an absolute key, digit d of it; does the call have digit d, and which buffer holds its input
struct GmPlan { int mn[3], sh_y, sh_z; };
__device__ __forceinline__ GmPlan gm_plan(const GmCtl* __restrict__ ctl) { GmPlan p; p.mn[0] = ctl->bb[0]; p.mn[1] = ctl->bb[1]; p.mn[2] = ctl->bb[2]; p.sh_y = ctl->sh_y; p.sh_z = ctl->sh_z; return p; }
__device__ __forceinline__ int gm_digit_of(const GmPlan& p, const gm_u64 k, const int shift) {
    const int ix = (int)(k & 0x1fffffull) - GM_BIAS, iy = (int)((k >> 21) & 0x1fffffull) - GM_BIAS, iz = (int)((k >> 42) & 0x1fffffull) - GM_BIAS;
    const gm_u64 rel = (gm_u64)(unsigned)(ix - p.mn[0]) | ((gm_u64)(unsigned)(iy - p.mn[1]) << p.sh_y) | ((gm_u64)(unsigned)(iz - p.mn[2]) << p.sh_z);
    return (int)((rel >> shift) & 255ull);
}
__device__ __forceinline__ bool gm_digit(const GmCtl* __restrict__ ctl, const int d, int& par) { par = d & 1; return d < ctl->npass && !ctl->bad; }
struct GmDigit { GmPlan plan; int shift; __device__ __forceinline__ int operator()(const gm_u64 k) const { return gm_digit_of(plan, k, shift); } };
// the buffer that holds the sorted pairs
__device__ __forceinline__ int gm_sorted_par(const GmCtl* __restrict__ ctl) { return ctl->npass & 1; }

__global__ __launch_bounds__(64) void k_gm_hist(const gm_u64* __restrict__ key0, const gm_u64* __restrict__ key1, const int n, const int d, const GmCtl* __restrict__ ctl,
                                                int* __restrict__ hist) {
    __shared__ int h[256];
    int par;
    if (!gm_digit(ctl, d, par)) return;
    cloud_radix_hist<GM_SORT_TILE>(par ? key1 : key0, n, blockIdx.x, GmDigit{gm_plan(ctl), 8 * d}, h, hist + (size_t)blockIdx.x * 256);
}
// exclusive scan of hist over (digit value, tile) in that order.  a: per workgroup of GM_SCAN_CHUNK tiles and digit value, the sum; b (one workgroup over the
// nchunk x 256 sums): where each workgroup's tiles of each digit value start; c: the tiles' counts rewritten as running offsets
__global__ __launch_bounds__(256) void k_gm_scan_a(const int* __restrict__ hist, const int nt, const int d, const GmCtl* __restrict__ ctl, int* __restrict__ csum) {
    int par;
    if (!gm_digit(ctl, d, par)) return;
    const int ta = blockIdx.x * GM_SCAN_CHUNK, tb = min(nt, ta + GM_SCAN_CHUNK);
    int s = 0;
    for (int t = ta; t < tb; ++t) s += hist[(size_t)t * 256 + threadIdx.x];
    csum[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_gm_scan_b(int* __restrict__ csum, const int nchunk, const int d, const GmCtl* __restrict__ ctl) {
    __shared__ int dbase[256];
    int par;
    if (!gm_digit(ctl, d, par)) return;
    int run = 0;
    for (int b = 0; b < nchunk; ++b) { const int x = csum[(size_t)b * 256 + threadIdx.x]; csum[(size_t)b * 256 + threadIdx.x] = run; run += x; }
    dbase[threadIdx.x] = run;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < 256; ++k) { const int x = dbase[k]; dbase[k] = t; t += x; } }
    __syncthreads();
    const int add = dbase[threadIdx.x];
    for (int b = 0; b < nchunk; ++b) csum[(size_t)b * 256 + threadIdx.x] += add;
}
__global__ __launch_bounds__(256) void k_gm_scan_c(int* __restrict__ hist, const int nt, const int d, const GmCtl* __restrict__ ctl, const int* __restrict__ csum) {
    int par;
    if (!gm_digit(ctl, d, par)) return;
    const int ta = blockIdx.x * GM_SCAN_CHUNK, tb = min(nt, ta + GM_SCAN_CHUNK);
    int run = csum[(size_t)blockIdx.x * 256 + threadIdx.x];
    for (int t = ta; t < tb; ++t) { const int x = hist[(size_t)t * 256 + threadIdx.x]; hist[(size_t)t * 256 + threadIdx.x] = run; run += x; }
}
// one wavefront per tile: cloud_radix_scatter (stable)
__global__ __launch_bounds__(64) void k_gm_scatter(gm_u64* __restrict__ key0, gm_u64* __restrict__ key1, unsigned* __restrict__ val0, unsigned* __restrict__ val1, const int n,
                                                   const int d, const GmCtl* __restrict__ ctl, const int* __restrict__ hist) {
    __shared__ int base[256];
    int par;
    if (!gm_digit(ctl, d, par)) return;
    cloud_radix_scatter<GM_SORT_TILE>(par ? key1 : key0, par ? val1 : val0, n, blockIdx.x, GmDigit{gm_plan(ctl), 8 * d}, base, hist + (size_t)blockIdx.x * 256,
                                      par ? key0 : key1, par ? val0 : val1);
}

// ---- runs
// first index in a[0, n) with a[i] >= k
__device__ __forceinline__ int gm_lower_bound(const gm_u64* __restrict__ a, const int n, const gm_u64 k) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1); if (a[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
}
// per point: is it the head of a run, and does the run open a voxel the map does not hold; (place of the key in the old array) * 2 + found goes to the idle key
// buffer, the exclusive count of opening runs inside the workgroup to the idle rank buffer, the workgroup's total to blk
__global__ __launch_bounds__(GM_RUN_BLOCK) void k_gm_runs(gm_u64* __restrict__ key0, gm_u64* __restrict__ key1, unsigned* __restrict__ val0, unsigned* __restrict__ val1,
                                                          const int n, const GmCtl* __restrict__ ctl, const gm_u64* __restrict__ okeys, const int nv_old, int* __restrict__ blk) {
    __shared__ int s_w[GM_RUN_BLOCK / 64];
    if (ctl->bad) return;
    const int par = gm_sorted_par(ctl);
    const gm_u64* __restrict__ sk = par ? key1 : key0;
    gm_u64* __restrict__ enc = par ? key0 : key1; unsigned* __restrict__ pre = par ? val0 : val1;
    const int i = blockIdx.x * GM_RUN_BLOCK + threadIdx.x, wv = threadIdx.x >> 6;
    int c = 0;
    if (i < n) {
        const gm_u64 k = sk[i];
        if (i == 0 || sk[i - 1] != k) {
            const int lb = gm_lower_bound(okeys, nv_old, k);
            const int found = lb < nv_old && okeys[lb] == k;
            enc[i] = ((gm_u64)(unsigned)lb << 1) | (gm_u64)found;
            c = !found;
        }
    }
    // the workgroup scan written out: the wavefront totals chained by ONE thread.  cloud_wg_excl_scan (every thread sums the sixteen totals) measured
    // 1.093 -> 1.114 ms in the runs + sums stage of 667 frames x 32768 points, outside the parent's spread of 0.003 (profiles/cloud_dedup_ab.txt)
    const int incl = cloud_wave_incl_scan(c);
    if ((threadIdx.x & 63) == 63) s_w[wv] = incl;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < GM_RUN_BLOCK / 64; ++k) { const int x = s_w[k]; s_w[k] = t; t += x; } blk[blockIdx.x] = t; }
    __syncthreads();
    if (i < n) pre[i] = (unsigned)(s_w[wv] + incl - c);
}
// exclusive scan of the workgroup totals in place (one workgroup, a contiguous chunk per thread); the map's size after the call
__global__ __launch_bounds__(GM_TOP_THREADS) void k_gm_runs_top(int* __restrict__ blk, const int nblk, GmCtl* ctl, const int nv_old, const int max_vox) {
    __shared__ int part[GM_TOP_THREADS];
    if (ctl->bad) return;
    const int tid = threadIdx.x, chunk = (nblk + GM_TOP_THREADS - 1) / GM_TOP_THREADS, b0 = min(nblk, tid * chunk), b1 = min(nblk, b0 + chunk);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += blk[b];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int k = 0; k < GM_TOP_THREADS; ++k) { const int x = part[k]; part[k] = t; t += x; }
        ctl->n_new = t;
        const long long nv = (long long)nv_old + t;
        ctl->nv_new = nv > 0x7fffffffLL ? 0x7fffffff : (int)nv;
        ctl->over = nv > (long long)max_vox;
    }
    __syncthreads();
    int run = part[tid];
    for (int b = b0; b < b1; ++b) { const int x = blk[b]; blk[b] = run; run += x; }
}
__global__ __launch_bounds__(256) void k_gm_accum(const gm_u64* __restrict__ key0, const gm_u64* __restrict__ key1, const unsigned* __restrict__ val0,
                                                  const unsigned* __restrict__ val1, const int n, const GmCtl* __restrict__ ctl, const float4* __restrict__ pts,
                                                  const int* __restrict__ blk, const GmVox ov, const GmVox nv) {
    if (ctl->bad || ctl->over) return;
    const int par = gm_sorted_par(ctl);
    const gm_u64* __restrict__ sk = par ? key1 : key0; const unsigned* __restrict__ sr = par ? val1 : val0;
    const gm_u64* __restrict__ enc = par ? key0 : key1; const unsigned* __restrict__ pre = par ? val0 : val1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const gm_u64 k = sk[i];
    if (i > 0 && sk[i - 1] == k) return;
    const gm_u64 e = enc[i];
    const int lb = (int)(e >> 1), found = (int)(e & 1ull);
    const int pos = lb + blk[i / GM_RUN_BLOCK] + (int)pre[i];       // (< nv_new <= max_voxels: the voxels below this key, old and new)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int cnt = 0;
    if (found) { acc = ov.sum[lb]; cnt = ov.cnt[lb]; }
    for (int j = i; j < n && sk[j] == k; ++j) {                      // ascending rank: the stable sort left the run in concatenation order
        const float4 p = pts[sr[j]];
        acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
        ++cnt;
    }
    const float c = (float)cnt;
    nv.key[pos] = k; nv.sum[pos] = acc; nv.cnt[pos] = cnt;
    nv.out[pos] = make_float4(acc.x / c, acc.y / c, acc.z / c, acc.w / c);
}
__global__ __launch_bounds__(256) void k_gm_merge(const gm_u64* __restrict__ key0, const gm_u64* __restrict__ key1, const unsigned* __restrict__ val0,
                                                  const unsigned* __restrict__ val1, const int n, const GmCtl* __restrict__ ctl, const int* __restrict__ blk,
                                                  const GmVox ov, const int nv_old, const GmVox nv) {
    if (ctl->bad || ctl->over) return;
    const int par = gm_sorted_par(ctl);
    const gm_u64* __restrict__ sk = par ? key1 : key0; const unsigned* __restrict__ pre = par ? val0 : val1;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nv_old) return;
    const gm_u64 k = ov.key[j];
    const int p = gm_lower_bound(sk, n, k);
    if (p < n && sk[p] == k) return;                                 // a run of this call owns the voxel
    const int pos = j + (p < n ? blk[p / GM_RUN_BLOCK] + (int)pre[p] : ctl->n_new);
    nv.key[pos] = k; nv.sum[pos] = ov.sum[j]; nv.cnt[pos] = ov.cnt[j]; nv.out[pos] = ov.out[j];
}

#define GM_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

static int gm_frames_reserve(glio_gmap* gm, int n) {
    if (n <= gm->frames_cap) return GLIO_OK;
    int cap = gm->frames_cap > 0 ? gm->frames_cap : 64;
    while (cap < n) cap *= 2;
    if (gm->h_frames) { hipHostFree(gm->h_frames); gm->h_frames = nullptr; }
    if (gm->d_frames) { hipFree(gm->d_frames); gm->d_frames = nullptr; }
    gm->frames_cap = 0;
    GM_CHECK(hipHostMalloc((void**)&gm->h_frames, (size_t)cap * sizeof(GmFrame)));
    GM_CHECK(hipMalloc((void**)&gm->d_frames, (size_t)cap * sizeof(GmFrame)));
    gm->frames_cap = cap;
    return GLIO_OK;
}
static void gm_reset(glio_gmap* gm) {
    gm->n_vox = 0; gm->n_points = 0; gm->have_bb = 0;
    for (int a = 0; a < 3; ++a) { gm->bb[a] = 0x7fffffff; gm->bb[3 + a] = (int)0x80000000; }
}
static int gm_box_overflows(const int* bb) {
    const double cells = ((double)bb[3] - bb[0] + 1.0) * ((double)bb[4] - bb[1] + 1.0) * ((double)bb[5] - bb[2] + 1.0);
    return cells > 2147483647.0;
}

extern "C" {

void glio_gmap_opts_default(glio_gmap_opts* o) {
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->leaf = 0.2f;                       // ds_filter_global_map.setLeafSize(0.2 ...), Estimator.cpp:856
    o->max_voxels = 1 << 22;
    o->max_points_per_add = 1 << 22;
}
int glio_gmap_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_gmap_opts), (int32_t)sizeof(glio_gmap_info)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

void glio_gmap_destroy(glio_gmap* gm) {
    if (!gm) return;
    hipSetDevice(gm->v.device);
    if (gm->stream) hipStreamSynchronize(gm->stream);
    for (int b = 0; b < 2; ++b) {
        void* p[] = {gm->vox[b].key, gm->vox[b].sum, gm->vox[b].cnt, gm->vox[b].out, gm->d_key[b], gm->d_val[b]};
        for (void* q : p) if (q) hipFree(q);
    }
    void* p[] = {gm->d_pts, gm->d_hist, gm->d_csum, gm->d_blk, gm->d_ctl, gm->d_frames};
    for (void* q : p) if (q) hipFree(q);
    if (gm->h_ctl) hipHostFree(gm->h_ctl);
    if (gm->h_frames) hipHostFree(gm->h_frames);
    if (gm->ev_dep) hipEventDestroy(gm->ev_dep);
    if (gm->ev_done) hipEventDestroy(gm->ev_done);
    for (hipEvent_t e : gm->ev_t) if (e) hipEventDestroy(e);
    if (gm->stream) hipStreamDestroy(gm->stream);
    delete gm;
}

static int gm_create_body(glio_gmap* gm) {
    GM_CHECK(hipSetDevice(gm->v.device));
    GM_CHECK(hipStreamCreateWithFlags(&gm->stream, hipStreamNonBlocking));
    GM_CHECK(hipEventCreateWithFlags(&gm->ev_dep, hipEventDisableTiming));
    GM_CHECK(hipEventCreateWithFlags(&gm->ev_done, hipEventDisableTiming | hipEventBlockingSync));
    for (int k = 0; k < 5; ++k) GM_CHECK(hipEventCreate(&gm->ev_t[k]));
    const size_t nv = (size_t)gm->o.max_voxels, np = (size_t)gm->o.max_points_per_add;
    for (int b = 0; b < 2; ++b) {
        GM_CHECK(hipMalloc((void**)&gm->vox[b].key, nv * 8)); GM_CHECK(hipMalloc((void**)&gm->vox[b].sum, nv * 16));
        GM_CHECK(hipMalloc((void**)&gm->vox[b].cnt, nv * 4)); GM_CHECK(hipMalloc((void**)&gm->vox[b].out, nv * 16));
        GM_CHECK(hipMalloc((void**)&gm->d_key[b], np * 8)); GM_CHECK(hipMalloc((void**)&gm->d_val[b], np * 4));
    }
    GM_CHECK(hipMalloc((void**)&gm->d_pts, np * 16));
    const size_t nt = (np + GM_SORT_TILE - 1) / GM_SORT_TILE, nchunk = (nt + GM_SCAN_CHUNK - 1) / GM_SCAN_CHUNK, nblk = (np + GM_RUN_BLOCK - 1) / GM_RUN_BLOCK;
    GM_CHECK(hipMalloc((void**)&gm->d_hist, nt * 256 * 4)); GM_CHECK(hipMalloc((void**)&gm->d_csum, nchunk * 256 * 4)); GM_CHECK(hipMalloc((void**)&gm->d_blk, nblk * 4));
    GM_CHECK(hipMalloc((void**)&gm->d_ctl, sizeof(GmCtl))); GM_CHECK(hipHostMalloc((void**)&gm->h_ctl, sizeof(GmCtl)));
    { const int rf = gm_frames_reserve(gm, 64); if (rf != GLIO_OK) return rf; }
    GM_CHECK(hipStreamSynchronize(gm->stream));
    return GLIO_OK;
}
// b or d: the source of the clouds
static int gm_create(glio_bassoc* b, glio_dense* d, glio_static* st, const glio_gmap_opts* opts, glio_gmap** out) {
    if ((!b && !d && !st) || !opts || !out) return GLIO_E_ARG;
    const glio_gmap_opts& o = *opts;
    if (!(o.leaf > 0.f) || !(o.leaf <= FLT_MAX) || o.max_voxels < 1 || o.max_points_per_add < 1) {
        glio_set_error("bad glio_gmap_opts (leaf %g, max_voxels %d, max_points_per_add %d)", (double)o.leaf, o.max_voxels, o.max_points_per_add);
        return GLIO_E_ARG;
    }
    glio_gmap* gm = new glio_gmap();
    memset(gm, 0, sizeof *gm);
    gm->o = o;
    gm->inv_leaf = 1.0f / o.leaf;
    gm_reset(gm);
    gm->dense = d; gm->stat = st;
    { const int rv = st ? glio_static_view(st, &gm->v) : d ? glio_dense_view(d, &gm->v) : glio_bassoc_view(b, &gm->v); if (rv != GLIO_OK) { delete gm; return rv; } }
    const int rc = gm_create_body(gm);
    if (rc != GLIO_OK) { glio_gmap_destroy(gm); return rc; }
    *out = gm;
    return GLIO_OK;
}
int glio_gmap_create(glio_bassoc* b, const glio_gmap_opts* opts, glio_gmap** out) { return gm_create(b, nullptr, nullptr, opts, out); }
int glio_gmap_create_on_dense(glio_dense* d, const glio_gmap_opts* opts, glio_gmap** out) { return gm_create(nullptr, d, nullptr, opts, out); }
int glio_gmap_create_on_static(glio_static* st, const glio_gmap_opts* opts, glio_gmap** out) { return gm_create(nullptr, nullptr, st, opts, out); }

int glio_gmap_clear(glio_gmap* gm) {
    if (!gm) return GLIO_E_ARG;
    gm_reset(gm);
    return GLIO_OK;
}

int glio_gmap_add_frames(glio_gmap* gm, int n_frames, const int32_t* frame_idx, const double* poses, glio_gmap_info* info) {
    GLIO_TRACE("glio_gmap_add_frames");
    if (!gm) return GLIO_E_ARG;
    if (n_frames < 1 || n_frames > GM_MAX_FRAMES) { glio_set_error("glio_gmap_add_frames: %d frames, a call takes 1 .. %d", n_frames, GM_MAX_FRAMES); return GLIO_E_ARG; }
    if (!frame_idx || !poses) { glio_set_error("glio_gmap_add_frames: null frame list / poses"); return GLIO_E_ARG; }
    GM_CHECK(hipSetDevice(gm->v.device));
    { const int rf = gm_frames_reserve(gm, n_frames); if (rf != GLIO_OK) return rf; }
    long long total = 0;
    int max_n = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int k = frame_idx[f];
        if (k < 0 || k >= gm->v.K) { glio_set_error("glio_gmap_add_frames: frame %d outside [0, %d)", k, gm->v.K); return GLIO_E_ARG; }
        const int nk = gm->v.h_n[k];
        if (nk < 1) { glio_set_error("glio_gmap_add_frames: frame %d was never set (or holds no point)", k); return GLIO_E_ARG; }
        for (int c = 0; c < 7; ++c) if (!(fabs(poses[7 * f + c]) <= DBL_MAX)) { glio_set_error("glio_gmap_add_frames: pose %d is not finite", f); return GLIO_E_ARG; }
        GmFrame& fr = gm->h_frames[f];
        fr.src = gm->v.d_local + (size_t)k * gm->v.cap; fr.n = nk; fr.off = (int)total;
        for (int c = 0; c < 3; ++c) fr.t[c] = poses[7 * f + c];
        for (int c = 0; c < 4; ++c) fr.q[c] = poses[7 * f + 3 + c];
        total += nk;
        if (total > (long long)gm->o.max_points_per_add) { glio_set_error("glio_gmap_add_frames: more than max_points_per_add = %d points", gm->o.max_points_per_add); return GLIO_E_ARG; }
        if (nk > max_n) max_n = nk;
    }
    const int n = (int)total, nv_old = gm->n_vox;
    const int nt = (n + GM_SORT_TILE - 1) / GM_SORT_TILE, nchunk = (nt + GM_SCAN_CHUNK - 1) / GM_SCAN_CHUNK, nblk = (n + GM_RUN_BLOCK - 1) / GM_RUN_BLOCK;
    hipStream_t s = gm->stream;
    // the association's pending frame copies come first -- for this stream, not for the host
    GM_CHECK(hipEventRecord(gm->ev_dep, gm->v.stream));
    GM_CHECK(hipStreamWaitEvent(s, gm->ev_dep, 0));
    GM_CHECK(hipMemcpyAsync(gm->d_frames, gm->h_frames, (size_t)n_frames * sizeof(GmFrame), hipMemcpyHostToDevice, s));
    GM_CHECK(hipEventRecord(gm->ev_t[0], s));
    hipLaunchKernelGGL(k_gm_begin, dim3(1), dim3(64), 0, s, gm->d_ctl);
    hipLaunchKernelGGL(k_gm_transform, dim3((max_n + GM_TF_THREADS * GM_TF_PER - 1) / (GM_TF_THREADS * GM_TF_PER), n_frames), dim3(GM_TF_THREADS), 0, s, gm->d_frames,
                       gm->inv_leaf, gm->d_pts, gm->d_key[0], gm->d_val[0], gm->d_ctl);
    hipLaunchKernelGGL(k_gm_plan, dim3(1), dim3(64), 0, s, gm->d_ctl);
    GM_CHECK(hipEventRecord(gm->ev_t[1], s));
    for (int d = 0; d < 8; ++d) {
        hipLaunchKernelGGL(k_gm_hist, dim3(nt), dim3(64), 0, s, gm->d_key[0], gm->d_key[1], n, d, gm->d_ctl, gm->d_hist);
        hipLaunchKernelGGL(k_gm_scan_a, dim3(nchunk), dim3(256), 0, s, gm->d_hist, nt, d, gm->d_ctl, gm->d_csum);
        hipLaunchKernelGGL(k_gm_scan_b, dim3(1), dim3(256), 0, s, gm->d_csum, nchunk, d, gm->d_ctl);
        hipLaunchKernelGGL(k_gm_scan_c, dim3(nchunk), dim3(256), 0, s, gm->d_hist, nt, d, gm->d_ctl, gm->d_csum);
        hipLaunchKernelGGL(k_gm_scatter, dim3(nt), dim3(64), 0, s, gm->d_key[0], gm->d_key[1], gm->d_val[0], gm->d_val[1], n, d, gm->d_ctl, gm->d_hist);
    }
    GM_CHECK(hipEventRecord(gm->ev_t[2], s));
    const GmVox ov = gm->vox[gm->cur], nv = gm->vox[gm->cur ^ 1];
    hipLaunchKernelGGL(k_gm_runs, dim3(nblk), dim3(GM_RUN_BLOCK), 0, s, gm->d_key[0], gm->d_key[1], gm->d_val[0], gm->d_val[1], n, gm->d_ctl, ov.key, nv_old, gm->d_blk);
    hipLaunchKernelGGL(k_gm_runs_top, dim3(1), dim3(GM_TOP_THREADS), 0, s, gm->d_blk, nblk, gm->d_ctl, nv_old, gm->o.max_voxels);
    hipLaunchKernelGGL(k_gm_accum, dim3((n + 255) / 256), dim3(256), 0, s, gm->d_key[0], gm->d_key[1], gm->d_val[0], gm->d_val[1], n, gm->d_ctl, gm->d_pts, gm->d_blk, ov, nv);
    GM_CHECK(hipEventRecord(gm->ev_t[3], s));
    if (nv_old > 0)
        hipLaunchKernelGGL(k_gm_merge, dim3((nv_old + 255) / 256), dim3(256), 0, s, gm->d_key[0], gm->d_key[1], gm->d_val[0], gm->d_val[1], n, gm->d_ctl, gm->d_blk, ov, nv_old, nv);
    GM_CHECK(hipGetLastError());
    // (a dense store writes its frames without waiting for the host: its next write comes behind this read)
    if (gm->dense) { const int re = glio_dense_external_read(gm->dense, s); if (re != GLIO_OK) return re; }
    if (gm->stat) { const int re = glio_static_external_read(gm->stat, s); if (re != GLIO_OK) return re; }
    GM_CHECK(hipEventRecord(gm->ev_t[4], s));
    GM_CHECK(hipMemcpyAsync(gm->h_ctl, gm->d_ctl, sizeof(GmCtl), hipMemcpyDeviceToHost, s));
    GM_CHECK(hipEventRecord(gm->ev_done, s));
    GM_CHECK(hipEventSynchronize(gm->ev_done));      // (nothing of this call reads the association's clouds after this point: its next write needs no event)
    gm->have_ms = 1;
    const GmCtl c = *gm->h_ctl;
    if (c.bad) { glio_set_error("glio_gmap_add_frames: a voxel coordinate outside [-2^20, 2^20) (leaf %g)", (double)gm->o.leaf); return GLIO_E_ARG; }
    if (c.over) { glio_set_error("glio_gmap_add_frames: more than max_voxels = %d voxels", gm->o.max_voxels); return GLIO_E_ARG; }
    gm->cur ^= 1; gm->n_vox = c.nv_new; gm->n_points += n;
    for (int a = 0; a < 3; ++a) { gm->bb[a] = std::min(gm->bb[a], c.bb[a]); gm->bb[3 + a] = std::max(gm->bb[3 + a], c.bb[3 + a]); }
    gm->have_bb = 1;
    if (info) {
        info->n_points_total = gm->n_points; info->n_voxels = gm->n_vox; info->radix_passes = c.npass; info->pcl_index_overflow = gm_box_overflows(gm->bb); info->reserved_ = 0;
    }
    return GLIO_OK;
}

int glio_gmap_size(glio_gmap* gm, int* n_voxels) {
    if (!gm || !n_voxels) return GLIO_E_ARG;
    *n_voxels = gm->n_vox;
    return GLIO_OK;
}
int glio_gmap_read(glio_gmap* gm, int first, int n, float* out_xyzi) {
    if (!gm || first < 0 || n < 0 || (long long)first + n > (long long)gm->n_vox || (n > 0 && !out_xyzi)) { glio_set_error("glio_gmap_read: bad range"); return GLIO_E_ARG; }
    if (n == 0) return GLIO_OK;
    GM_CHECK(hipSetDevice(gm->v.device));
    GM_CHECK(hipStreamSynchronize(gm->stream));
    GM_CHECK(hipMemcpy(out_xyzi, gm->vox[gm->cur].out + first, (size_t)n * 16, hipMemcpyDeviceToHost));
    return GLIO_OK;
}
int glio_gmap_points_dev(glio_gmap* gm, const void** points_dev, int* n_voxels) {
    if (!gm || !points_dev) return GLIO_E_ARG;
    *points_dev = gm->vox[gm->cur].out;
    if (n_voxels) *n_voxels = gm->n_vox;
    return GLIO_OK;
}
int glio_gmap_last_device_ms(glio_gmap* gm, float* ms) {
    if (!gm || !ms) return GLIO_E_ARG;
    if (!gm->have_ms) { glio_set_error("glio_gmap_add_frames first"); return GLIO_E_STATE; }
    GM_CHECK(hipSetDevice(gm->v.device));
    GM_CHECK(hipEventElapsedTime(ms, gm->ev_t[0], gm->ev_t[4]));
    return GLIO_OK;
}
int glio_gmap_last_stage_ms(glio_gmap* gm, float* ms4) {
    if (!gm || !ms4) return GLIO_E_ARG;
    if (!gm->have_ms) { glio_set_error("glio_gmap_add_frames first"); return GLIO_E_STATE; }
    GM_CHECK(hipSetDevice(gm->v.device));
    for (int k = 0; k < 4; ++k) GM_CHECK(hipEventElapsedTime(ms4 + k, gm->ev_t[k], gm->ev_t[k + 1]));
    return GLIO_OK;
}

}  // extern "C"

// localmap_kernels.hip -- device-resident local surf map.
//
// Replaces, for the sliding-window path, buildLocalMapWithLandMark + downSampleCloud + the kd-tree input
// (reference GLIO/src/Estimator.cpp:3529-3631, 2056): the last `local_map_width` keyframe clouds are kept ON THE
// DEVICE in the map frame (transformCloud(surf_frames[idx], q_po * q_bl, q_po * t_bl + t_po), :3569-3574), so that per
// keyframe only ONE new scan (16 B/point) crosses PCIe instead of the whole down-sampled map; the concatenation is
// voxel-averaged on the device (pcl::VoxelGrid semantics: bounding box, floor(p * inv_leaf) - min_b, centroid per
// voxel, output ordered by linear voxel index) and handed to K1 without leaving HBM.
//
// The ring holds width x cap x 16 B (50 x 64k points = 52 MB).  The voxel table is PERSISTENT and keyed by absolute voxel
// coordinates; sums are kept in 2^-20 m fixed point (int64 atomics), i.e. they are exact integers: pushing a keyframe adds
// its points, evicting the oldest subtracts them again and the table is exactly what a rebuild from scratch would give
// (bit for bit, whatever the atomic order) -- insert/evict costs two keyframes of traffic instead of re-streaming the
// whole ring (3.3 M points).  Emptied voxels stay as tombstones (count 0) until they fill half the table, then the table
// is rebuilt once.  PCL's float accumulation (whose order std::sort leaves unspecified) is matched to ~1e-6 m.
//
// A push is the reference's steady state (:3580-3610).  Its other branch (:3545-3579: the deque below local_map_width -- the first 50 keyframes and, SURVEY Q17,
// every call after a loop closure -- is thrown away and refilled from surf_frames at the CURRENT poses) is glio_localmap_rebuild_from_frames: ring and table
// rebuilt from the keyframe clouds resident in a batch association, two launches whatever the number of keyframes (k_lm_rebuild_*).
#include <cfloat>
#include <algorithm>
#include <cstring>
#include <chrono>

#include "glio_device.h"
#include "cloud_device.h"

// the transform must round like the reference's scalar code (and the oracle): no FMA contraction in this file
#pragma clang fp contract(off)

struct LocalMap {
    int width, cap;                 // keyframes in the ring, points per keyframe
    float leaf;
    float4* d_ring;                 // [width][cap] clouds in the map frame
    int* h_n;                       // [width] points per ring entry
    int* d_n;                       // [width] the same, on the device (grid.y = ring slot)
    int head, count;                // ring: entries [head, head+count) modulo width, oldest first
    long long pushed;               // keyframes pushed so far
    // voxel grid workspace
    int table_cap;                  // power of two >= 2 * max voxels
    unsigned long long* d_keys;     // voxel linear index or EMPTY
    long long* d_sum;               // [table_cap][4] fixed-point sums x,y,z,intensity
    int* d_cnt;                     // [table_cap]
    int* d_bbox;                    // [6] ordered-int encoded min xyz / max xyz of the whole ring
    int* d_slot_bbox;               // [width][6] the same per ring slot
    int* d_nkeys;                   // [1] voxel keys ever claimed in the table (live + tombstones)
    int nkeys_seen;                 // host copy after the last build
    int* d_nvox;                    // [1]
    unsigned long long* d_vkey; unsigned long long* d_vkey_sorted; int* d_vslot; int* d_vslot_sorted;
    void* d_sort_tmp; size_t sort_tmp_bytes;
    float4* d_out;                  // [max voxels] down-sampled map, ordered by voxel index
    int max_vox;
    int* h_pin;                     // pinned scalar read-back
    unsigned* d_bm; int* d_bm_pre; int* d_bm_blk; int* d_bm_over; int bm_dirty; int force_sort;      // occupancy bitmap over the bounding box (ordered output without a sort, see k_bm_*)
    unsigned long long* h_pub; unsigned long long* d_h_pub; unsigned pub_seq;      // the same three scalars published by a kernel into mapped host memory (k_lm_publish)
    // accumulation = 1 (glio_localmap_set_accumulation): centroids as pcl::VoxelGrid forms them -- FLOAT sums over a voxel's points in the order of the
    // concatenated cloud (keyframes oldest first, points in scan order: the order a stable sort by voxel index leaves, and what the oracle's restatement
    // does) -- instead of the exact fixed-point sums.  Same voxels, same output order; the centroids then equal the oracle's bit for bit.
    int accumulation;
    // what glio_debug_localmap_stats reports (host counters since glio_localmap_config; nothing reads them on the way)
    int n_table_rebuilds, n_bm_wipes, last_path, last_passes, last_nv;
    int* d_fill; int* d_slot_start; int* d_plist;      // [table_cap], [table_cap], [width * cap]: per-voxel fill counters, list starts, point lists
    // glio_localmap_rebuild_from_frames: the frame table [width] (pinned, its device mirror, the event of its last upload) and the event that orders the context's
    // stream behind the frame copies of the batch association
    struct LmFrame* h_frames; struct LmFrame* d_frames; hipEvent_t ev_frames; int frames_in_flight; hipEvent_t ev_dep;
    // glio_vg_staged_*: PCL's overflow rule is applied (a box of more than INT32_MAX cells passes the cloud through: the keyframe cloud's filter, as
    // ft_voxel_grid); last_passthrough = the last build met it
    int pcl_overflow, last_passthrough;
    int wave_emit;                  // accumulation = 1 emits through k_lm_emit_wave (glio_vg_set_wave_emit: the dense store's VoxelGrid only)
    hipEvent_t ev_rb0, ev_rb1; int time_rebuild, have_rebuild_ms;      // GLIO_LM_REBUILD_TIMING=1: timing events around the rebuild's two launches (glio_localmap_last_rebuild_device_ms)
};
// one keyframe of a rebuild: its own-frame cloud (resident in a batch association), its size and transformCloud's pose
struct LmFrame { const float4* src; int n, pad_; double q[4], t[3]; };

#define LM_EMPTY (~0ull)
#define LM_FIX 1048576.0            /* 2^20: fixed-point scale of the voxel sums */

static inline float h_ord2f(int i) { const int u = i >= 0 ? i : i ^ 0x7fffffff; float f; memcpy(&f, &u, 4); return f; }     // the same on the host

__global__ void k_lm_transform(const float4* __restrict__ in, int n, const double q0, const double q1, const double q2, const double q3,
                               const double t0, const double t1, const double t2, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q[4] = {q0, q1, q2, q3}, t[3] = {t0, t1, t2};
    out[i] = cloud_transform(q, t, in[i]);
}

// the same from a cloud that is already on the device in the LiDAR frame: p_body = p - off in FLOAT (what a caller's float cloud minus the
// extrinsic translation gives), then transformCloud as above
__global__ void k_lm_transform_off(const float4* __restrict__ in, int n, const float ox, const float oy, const float oz, const double q0, const double q1, const double q2,
                                   const double q3, const double t0, const double t1, const double t2, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    const double q[4] = {q0, q1, q2, q3}, t[3] = {t0, t1, t2};
    out[i] = cloud_transform(q, t, make_float4(p.x - ox, p.y - oy, p.z - oz, p.w));
}

// one slot of the voxel table emptied (thread i of a grid that covers cap slots); the key counter with slot 0
__device__ __forceinline__ void lm_table_reset(const int i, unsigned long long* keys, long long* sum, int* cnt, const int cap, int* nkeys) {
    if (i < cap) { keys[i] = LM_EMPTY; cnt[i] = 0; sum[4 * (size_t)i] = 0; sum[4 * (size_t)i + 1] = 0; sum[4 * (size_t)i + 2] = 0; sum[4 * (size_t)i + 3] = 0; }
    if (i == 0) *nkeys = 0;
}
__global__ void k_lm_clear(unsigned long long* keys, long long* sum, int* cnt, int cap, int* nkeys) {
    lm_table_reset(blockIdx.x * blockDim.x + threadIdx.x, keys, sum, cnt, cap, nkeys);
}
// (also records the slot's point count on the device: the build used to upload all `width` counts from pageable memory -- an API call of ~8 us in a
//  chain of launches that is bound by the host's launch rate)
__global__ void k_lm_bbox_init(int* bbox, int* n_slot, const int n) {
    const int i = threadIdx.x;
    if (i < 3) bbox[i] = 0x7fffffff; else if (i < 6) bbox[i] = (int)0x80000000; else if (i == 6) *n_slot = n;
}
// bounding box of one ring slot (ordered-int atomics)
__global__ __launch_bounds__(1024) void k_lm_bbox(const float4* __restrict__ pts, int n, int* bbox) {
    __shared__ int s_box[16 * 6];
    CloudBox b;
    b.init();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        b.add(f2ord(p.x), f2ord(p.y), f2ord(p.z));
    }
    b.commit<16>(s_box, bbox);
}
// union of the slot boxes (slots with n = 0 are skipped)
__global__ void k_lm_bbox_union(const int* __restrict__ slot_bbox, const int* __restrict__ ns, int width, int* bbox, int* bm_over, int* nvox) {
    const int c = threadIdx.x;
    if (c == 6) *bm_over = 0;
    if (c == 7) *nvox = 0;                 // (k_lm_list counts the voxels from zero: was a hipMemsetAsync of its own)
    if (c >= 6) return;
    int v = c < 3 ? 0x7fffffff : (int)0x80000000;
    for (int k = 0; k < width; ++k) if (ns[k] > 0) v = c < 3 ? min(v, slot_bbox[6 * k + c]) : max(v, slot_bbox[6 * k + c]);
    bbox[c] = v;
}
// (the voxel's key = cloud_cell_key of its absolute voxel coordinates, hashed by cloud_key_hash: cloud_device.h)
// add (sign = +1) or remove (sign = -1) one point.
// A removal may assume that its key is in the table only while every insertion since the last table reset found a place.  After an overflow (bit 30 of
// *nkeys) some points of a keyframe were never inserted: their removal meets an empty slot, or walks a table without one, and then leaves every slot
// as it is -- the table is no longer what the ring holds anyway, and the host reconstructs it from the ring at the next build (lm_voxelize).
__device__ __forceinline__ void lm_table_add(const float4 p, const float inv_leaf, const int sign, unsigned long long* keys, long long* sum, int* cnt, const int cap, int* nkeys) {
    const unsigned long long key = cloud_cell_key((int)floorf(p.x * inv_leaf), (int)floorf(p.y * inv_leaf), (int)floorf(p.z * inv_leaf));
    unsigned s = cloud_key_hash(key) & (cap - 1);
    int probes = 0;
    for (;;) {
        const unsigned long long k = sign > 0 ? atomicCAS(keys + s, LM_EMPTY, key) : keys[s];
        if (k == LM_EMPTY) { if (sign < 0) return; atomicAdd(nkeys, 1); break; }      // (a removal that does not find its key touches nothing)
        if (k == key) break;
        s = (s + 1) & (cap - 1);
        if (++probes >= cap) { if (sign > 0) atomicOr(nkeys, 0x40000000); return; }          // table full: reported by glio_localmap_build
    }
    const long long f[4] = {llrint((double)p.x * LM_FIX), llrint((double)p.y * LM_FIX), llrint((double)p.z * LM_FIX), llrint((double)p.w * LM_FIX)};
#pragma unroll
    for (int c = 0; c < 4; ++c) atomicAdd(reinterpret_cast<unsigned long long*>(sum + 4 * (size_t)s + c), (unsigned long long)(sign > 0 ? f[c] : -f[c]));
    atomicAdd(cnt + s, sign);
}
// the points of one keyframe added or removed
__global__ void k_lm_accumulate(const float4* __restrict__ pts, int n, float inv_leaf, int sign, unsigned long long* keys, long long* sum, int* cnt,
                                int cap, int* nkeys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lm_table_add(pts[i], inv_leaf, sign, keys, sum, cnt, cap, nkeys);
}
// list the live voxels with their pcl::VoxelGrid linear index (relative to the ring's bounding box) for the ordered output
__global__ __launch_bounds__(1024) void k_lm_list(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt, int cap, float inv_leaf,
                                                  const int* __restrict__ bbox, int* nvox, unsigned long long* vkey, int* vslot, int max_vox,
                                                  unsigned* __restrict__ bm, const unsigned long long bm_bits, int* bm_over) {
    // one list position per live voxel: positions come from a block-wide count (ballot per wavefront, 16 wavefront totals through LDS)
    // and ONE atomic per 1024 slots -- an atomic per voxel (~1e5 on one address) made this kernel 100-500 us
    __shared__ int s_w[16], s_base;
    const int s = blockIdx.x * 1024 + threadIdx.x;
    const bool live = s < cap && cnt[s] > 0;
    int tot;
    const int rk = cloud_wg_rank<16>(live, s_w, tot);
    if (threadIdx.x == 0) s_base = tot > 0 ? atomicAdd(nvox, tot) : 0;
    __syncthreads();
    if (!live) return;
    int min_b[3], div_b[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { min_b[c] = (int)floorf(ord2f(bbox[c]) * inv_leaf); div_b[c] = (int)floorf(ord2f(bbox[3 + c]) * inv_leaf) - min_b[c] + 1; }
    const unsigned long long k = keys[s];
    int ix, iy, iz;
    cloud_cell_of_key(k, ix, iy, iz);
    const unsigned long long lin = (unsigned long long)((long long)(ix - min_b[0]) + (long long)(iy - min_b[1]) * div_b[0] + (long long)(iz - min_b[2]) * div_b[0] * (long long)div_b[1]);
    const int v = s_base + rk;
    if (v < max_vox) { vkey[v] = lin; vslot[v] = s; }
    // the voxel's bit in the occupancy bitmap of the bounding box (k_bm_*: its rank among the set bits is its place in the ordered output)
    if (bm) { if (lin < bm_bits) atomicOr(&bm[lin >> 5], 1u << (unsigned)(lin & 31ull)); else *bm_over = 1; }
}
// ------------------------------------------------------------------------------------------------
// Ordered output WITHOUT a sort.  pcl::VoxelGrid emits the voxels by ascending linear index; the indices are distinct and bounded by the cell count
// of the bounding box, so a voxel's place in the output is the number of occupied cells below it: the rank of its bit among the set bits of an occupancy
// bitmap over the box.  k_lm_list sets the bits; k_bm_scan1 / k_bm_scan2 turn the per-word popcounts into running counts (per word inside a block of
// 1024 words, per block); k_bm_rank writes every voxel's table slot at its rank; the emit kernel clears the words it used.  Three launches behind
// the build's synchronisation instead of the nine of a three-pass radix sort (~58 -> ~15 us for 1e5 voxels).  A bounding box of more than 2^27
// cells (16 MB of bits) takes the radix sort below, as does GLIO_LM_SORT=1.
// ------------------------------------------------------------------------------------------------
#define BM_MAX_BITS (1ull << 27)
__global__ __launch_bounds__(1024) void k_bm_scan1(const unsigned* __restrict__ bm, const int nwords, int* __restrict__ pre, int* __restrict__ blk) {
    __shared__ int s_w[16];
    const int w = blockIdx.x * 1024 + threadIdx.x;
    int tot;
    const int ex = cloud_wg_excl_scan<16>(w < nwords ? __popc(bm[w]) : 0, s_w, tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
    if (w < nwords) pre[w] = ex;
}
// exclusive scan of the block totals in place (one workgroup; nblk <= 4096: four per thread)
__global__ __launch_bounds__(1024) void k_bm_scan2(int* __restrict__ blk, const int nblk) {
    __shared__ int s_w[16];
    const int t = threadIdx.x;
    int a[4], tot = 0, all;
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = 4 * t + k < nblk ? blk[4 * t + k] : 0; tot += a[k]; }
    int run = cloud_wg_excl_scan<16>(tot, s_w, all);
#pragma unroll
    for (int k = 0; k < 4; ++k) { if (4 * t + k < nblk) blk[4 * t + k] = run; run += a[k]; }
}
__global__ void k_bm_rank(const unsigned long long* __restrict__ vkey, const int* __restrict__ vslot, const int nv, const unsigned* __restrict__ bm,
                          const int* __restrict__ pre, const int* __restrict__ blk, int* __restrict__ vslot_sorted) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const unsigned long long lin = vkey[v];
    const int w = (int)(lin >> 5);
    const unsigned below = bm[w] & ((1u << (unsigned)(lin & 31ull)) - 1u);
    vslot_sorted[blk[w >> 10] + pre[w] + __popc(below)] = vslot[v];
}
// (the words of the bitmap this build set, zero again for the next one: by the emit kernels, which run over the same nv voxels)
__device__ __forceinline__ void bm_clear_word(unsigned* __restrict__ bm, const unsigned long long* __restrict__ vkey, const int v, const unsigned long long bm_bits) {
    if (bm) { const unsigned long long lin = vkey[v]; if (lin < bm_bits) bm[lin >> 5] = 0u; }
}
// ------------------------------------------------------------------------------------------------
// Ordered output: the live voxels sorted by their pcl::VoxelGrid linear index.  A least-significant-digit radix sort on 8-bit
// digits, hand-written for this case: the keys are bounded by the ring's bounding box (typically < 2^24), so the host -- which
// reads the voxel count back anyway -- asks for only ceil(bits / 8) passes (3 instead of the 8 a generic 64-bit sort runs).
//   k_rs_hist     one wavefront per tile of 1024 pairs: cloud_radix_hist -> hist[tile][digit]
//   k_rs_scan     exclusive scan over (digit, tile) in that order: where each tile's run of each digit starts
//   k_rs_scatter  the same wavefront per tile: cloud_radix_scatter
#define RS_TILE 1024
struct RsDigit { int shift; __device__ __forceinline__ int operator()(const unsigned long long k) const { return (int)((k >> shift) & 255ull); } };
__global__ __launch_bounds__(64) void k_rs_hist(const unsigned long long* __restrict__ key, const int n, const int shift, const int nt, int* __restrict__ hist) {
    __shared__ int h[256];
    cloud_radix_hist<RS_TILE>(key, n, blockIdx.x, RsDigit{shift}, h, hist + (size_t)blockIdx.x * 256);
}
#define RS_SCAN_PER 64          /* tiles of one (digit, quarter) held in registers: up to 256 tiles = 262144 voxels */
__global__ __launch_bounds__(1024) void k_rs_scan(int* __restrict__ hist, const int nt) {
    // 256 digits x 4 quarters of the tiles: every thread sums its quarter (coalesced over the digits), the quarters and then the digits are chained
    // through LDS, and the thread rewrites its quarter as running offsets.  The quarter is read ONCE, all loads in flight together, and kept in
    // registers for the rewrite (it used to be two loops of dependent round trips: 10 us per pass for 103 tiles, three passes per map build).
    __shared__ int part[4][256], dbase[256];
    const int d = threadIdx.x & 255, q = threadIdx.x >> 8;
    const int per = (nt + 3) / 4, ta = min(nt, q * per), tb = min(nt, ta + per);
    const bool in_regs = per <= RS_SCAN_PER;
    int v[RS_SCAN_PER];
    int s = 0;
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < RS_SCAN_PER; ++k) v[k] = ta + k < tb ? hist[(ta + k) * 256 + d] : 0;
#pragma unroll
        for (int k = 0; k < RS_SCAN_PER; ++k) s += v[k];
    } else {
        for (int t = ta; t < tb; ++t) s += hist[t * 256 + d];
    }
    part[q][d] = s;
    __syncthreads();
    if (threadIdx.x < 256) dbase[d] = part[0][d] + part[1][d] + part[2][d] + part[3][d];
    __syncthreads();
    if (threadIdx.x < 64) {            // exclusive scan of the 256 digit totals by one wavefront: four per lane, then across the lanes
        const int l = threadIdx.x;
        const int a0 = dbase[4 * l], a1 = dbase[4 * l + 1], a2 = dbase[4 * l + 2], a3 = dbase[4 * l + 3];
        const int tot = a0 + a1 + a2 + a3;
        const int ex = cloud_wave_incl_scan(tot) - tot;
        dbase[4 * l] = ex; dbase[4 * l + 1] = ex + a0; dbase[4 * l + 2] = ex + a0 + a1; dbase[4 * l + 3] = ex + a0 + a1 + a2;
    }
    __syncthreads();
    int run = dbase[d];
    for (int k = 0; k < q; ++k) run += part[k][d];
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < RS_SCAN_PER; ++k) if (ta + k < tb) { hist[(ta + k) * 256 + d] = run; run += v[k]; }
    } else {
        for (int t = ta; t < tb; ++t) { const int x = hist[t * 256 + d]; hist[t * 256 + d] = run; run += x; }
    }
}
__global__ __launch_bounds__(64) void k_rs_scatter(const unsigned long long* __restrict__ key, const int* __restrict__ val, const int n, const int shift, const int nt,
                                                   const int* __restrict__ hist, unsigned long long* __restrict__ okey, int* __restrict__ oval) {
    __shared__ int base[256];
    cloud_radix_scatter<RS_TILE>(key, val, n, blockIdx.x, RsDigit{shift}, base, hist + (size_t)blockIdx.x * 256, okey, oval);
}

__global__ void k_lm_emit(const int* __restrict__ vslot_sorted, int nv, const long long* __restrict__ sum, const int* __restrict__ cnt,
                          float4* __restrict__ out, unsigned* __restrict__ bm, const unsigned long long* __restrict__ vkey, const unsigned long long bm_bits) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    bm_clear_word(bm, vkey, v, bm_bits);
    const int s = vslot_sorted[v];
    const double c = (double)cnt[s];
    out[v] = make_float4((float)((double)sum[4 * (size_t)s] / LM_FIX / c), (float)((double)sum[4 * (size_t)s + 1] / LM_FIX / c),
                         (float)((double)sum[4 * (size_t)s + 2] / LM_FIX / c), (float)((double)sum[4 * (size_t)s + 3] / LM_FIX / c));
}

// ---- float accumulation in concatenation order (accumulation = 1)
// exclusive scan of the live voxels' counts in OUTPUT order -> where each voxel's point list starts (one workgroup: a contiguous chunk per thread)
__global__ __launch_bounds__(1024) void k_lm_starts(const int* __restrict__ vslot_sorted, const int nv, const int* __restrict__ cnt, int* __restrict__ slot_start) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, chunk = (nv + 1023) / 1024, v0 = tid * chunk, v1 = min(nv, v0 + chunk);
    int sum = 0;
    for (int v = v0; v < v1; ++v) sum += cnt[vslot_sorted[v]];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int k = 0; k < 1024; ++k) { const int x = part[k]; part[k] = t; t += x; } }
    __syncthreads();
    int run = part[tid];
    for (int v = v0; v < v1; ++v) { const int sl = vslot_sorted[v]; slot_start[sl] = run; run += cnt[sl]; }
}
// every ring point -> its voxel's list (arbitrary position; the entry is the point's index in the concatenated cloud: age * cap + j)
__global__ void k_lm_scatter_idx(const float4* __restrict__ ring, const int* __restrict__ ns, const int cap, const int width, const int head, const int count,
                                 const float inv_leaf, const unsigned long long* __restrict__ keys, const int table_cap, const int* __restrict__ slot_start,
                                 int* __restrict__ fill, int* __restrict__ plist) {
    const int slot = blockIdx.y, age = (slot - head + width) % width;
    if (age >= count) return;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ns[slot]) return;
    const float4 p = ring[(size_t)slot * cap + j];
    const unsigned long long key = cloud_cell_key((int)floorf(p.x * inv_leaf), (int)floorf(p.y * inv_leaf), (int)floorf(p.z * inv_leaf));
    unsigned s = cloud_key_hash(key) & (table_cap - 1);
    while (keys[s] != key) s = (s + 1) & (table_cap - 1);              // (every ring point's voxel is in the table)
    const int pos = atomicAdd(fill + s, 1);
    plist[slot_start[s] + pos] = age * cap + j;
}
// one thread per voxel: its list sorted by concatenated index in the thread's own segment, then the float sums in that order and the centroid =
// sum / (float) count, as pcl::VoxelGrid.  A voxel holds tens of points: insertion sort.  One that holds thousands (a wall next to a standing vehicle, seen by
// every keyframe of the ring) would cost n^2 / 4 dependent round trips in one thread -- seconds -- so long lists take an in-place heapsort; the entries
// are distinct, so both leave the same list.
#define LM_LIST_INSERTION_MAX 64
__device__ __forceinline__ void lm_sift_down(int* __restrict__ L, int root, const int end) {       // max-heap over L[0, end)
    const int x = L[root];
    for (;;) {
        int ch = 2 * root + 1;
        if (ch >= end) break;
        if (ch + 1 < end && L[ch + 1] > L[ch]) ++ch;
        if (L[ch] <= x) break;
        L[root] = L[ch];
        root = ch;
    }
    L[root] = x;
}
__global__ void k_lm_emit_float(const int* __restrict__ vslot_sorted, const int nv, const int* __restrict__ cnt, const int* __restrict__ slot_start,
                                int* __restrict__ plist, const float4* __restrict__ ring, const int cap, const int width, const int head, float4* __restrict__ out,
                                unsigned* __restrict__ bm, const unsigned long long* __restrict__ vkey, const unsigned long long bm_bits) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    bm_clear_word(bm, vkey, v, bm_bits);
    const int s = vslot_sorted[v], n = cnt[s];
    int* L = plist + slot_start[s];
    if (n <= LM_LIST_INSERTION_MAX) {
        for (int a = 1; a < n; ++a) {
            const int x = L[a];
            int b = a - 1;
            while (b >= 0 && L[b] > x) { L[b + 1] = L[b]; --b; }
            L[b + 1] = x;
        }
    } else {
        for (int r = n / 2 - 1; r >= 0; --r) lm_sift_down(L, r, n);
        for (int e = n - 1; e > 0; --e) { const int top = L[0]; L[0] = L[e]; L[e] = top; lm_sift_down(L, 0, e); }
    }
    float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
    for (int a = 0; a < n; ++a) {
        const int idx = L[a], age = idx / cap, j = idx - age * cap;
        const float4 p = ring[(size_t)((head + age) % width) * cap + j];
        ax += p.x; ay += p.y; az += p.z; aw += p.w;
    }
    const float c = (float)n;
    out[v] = make_float4(ax / c, ay / c, az / c, aw / c);
}

// ---- the same emit for clouds with LONG lists (glio_vg_set_wave_emit: the dense store's full clouds, whose voxels next to the sensor hold hundreds of points).
// k_lm_emit_float gives a voxel's whole list to one thread: n^2 / 4 (or n log n) dependent round trips for the sort and n more for the points, while 63 lanes
// wait.  Here a wavefront owns LM_WAVE_VOX voxels.  Lists of up to LM_WAVE_LIST_MIN entries keep one thread each (the insertion sort above).  The longer ones are
// taken one after the other by the WHOLE wavefront: the list is sorted cooperatively -- a bitonic network in LDS, or in place in global memory for a list
// longer than LM_WAVE_LIST_LDS -- the points are fetched 64 at a time (one load per lane, the next 64 already in flight), and the four float sums take them
// from the lanes' registers one at a time in list order (v_readlane + v_add, every lane the same sum).  The adds are the same adds in the same order, the entries
// are distinct so every sort leaves the same list: the bytes are k_lm_emit_float's.  No atomic, no scratch.
#define LM_WAVE_VOX 16            /* voxels per wavefront (lanes 0 .. 15 hold one each) */
#define LM_WAVE_LIST_MIN 16       /* longest list that stays with one thread */
#define LM_WAVE_LIST_LDS 2048     /* longest list that is sorted in LDS (8 KB per wavefront: five wavefronts per SIMD keep their lists there) */
// Bitonic merge sort in the form whose every exchange is ascending (the first step of a stage pairs i with its mirror image inside the block of k, the later
// ones i with i + j): elements behind the end behave as +inf and never move, so a list of ANY length is sorted without padding.  One wavefront, `a` in LDS or
// in global memory; every step ends with the ordering point that fits.
template <bool IN_LDS> __device__ __forceinline__ void lm_wave_sync() {
    if (IN_LDS) GLIO_WAVE_LDS_SYNC();
    else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
}
template <bool IN_LDS> __device__ __forceinline__ void lm_wave_bitonic(int* a, const int n, const int lane) {
    for (int k = 2; (k >> 1) < n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane;; t += 64) {
                const int i = (t / j) * 2 * j + (t % j);                     // (j is a power of two)
                if (i >= n) break;
                const int p = (j == (k >> 1)) ? (i - (i % j)) + (k - 1 - (i % j)) : i + j;      // (i % j < j: the mirror image lies in the upper half of i's block)
                if (p < n) { const int x = a[i], y = a[p]; if (x > y) { a[i] = y; a[p] = x; } }
            }
            lm_wave_sync<IN_LDS>();
        }
    }
}
__device__ __forceinline__ float4 lm_ring_point(const float4* __restrict__ ring, const int idx, const int cap, const int width, const int head) {
    const int age = idx / cap, j = idx - age * cap;
    return ring[(size_t)((head + age) % width) * cap + j];
}
__global__ __launch_bounds__(64) void k_lm_emit_wave(const int* __restrict__ vslot_sorted, const int nv, const int* __restrict__ cnt, const int* __restrict__ slot_start,
                                                     int* plist, const float4* __restrict__ ring, const int cap, const int width, const int head, float4* __restrict__ out,
                                                     unsigned* __restrict__ bm, const unsigned long long* __restrict__ vkey, const unsigned long long bm_bits) {
    __shared__ int s_list[LM_WAVE_LIST_LDS];
    const int lane = threadIdx.x, v = blockIdx.x * LM_WAVE_VOX + lane;
    const bool mine = lane < LM_WAVE_VOX && v < nv;
    int n = 0, st = 0;
    if (mine) {
        bm_clear_word(bm, vkey, v, bm_bits);
        const int s = vslot_sorted[v];
        n = cnt[s]; st = slot_start[s];
    }
    if (mine && n <= LM_WAVE_LIST_MIN) {
        int* L = plist + st;
        for (int a = 1; a < n; ++a) {
            const int x = L[a];
            int b = a - 1;
            while (b >= 0 && L[b] > x) { L[b + 1] = L[b]; --b; }
            L[b + 1] = x;
        }
        float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
        for (int a = 0; a < n; ++a) {
            const float4 p = lm_ring_point(ring, L[a], cap, width, head);
            ax += p.x; ay += p.y; az += p.z; aw += p.w;
        }
        const float c = (float)n;
        out[v] = make_float4(ax / c, ay / c, az / c, aw / c);
    }
    unsigned long long todo = __ballot(mine && n > LM_WAVE_LIST_MIN);
    while (todo) {                                                           // (uniform over the wavefront)
        const int l = __ffsll(todo) - 1;
        todo &= todo - 1ull;
        const int ln = __builtin_amdgcn_readlane(n, l), lst = __builtin_amdgcn_readlane(st, l);
        int* L = plist + lst;
        const bool in_lds = ln <= LM_WAVE_LIST_LDS;
        if (in_lds) {
            for (int a = lane; a < ln; a += 64) s_list[a] = L[a];
            GLIO_WAVE_LDS_SYNC();
            lm_wave_bitonic<true>(s_list, ln, lane);
        } else lm_wave_bitonic<false>(L, ln, lane);
        float ax = 0.f, ay = 0.f, az = 0.f, aw = 0.f;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < ln) p = lm_ring_point(ring, in_lds ? s_list[lane] : L[lane], cap, width, head);
        for (int a0 = 0; a0 < ln; a0 += 64) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);                      // the next 64 points: in flight while these are summed
            const int an = a0 + 64 + lane;
            if (an < ln) q = lm_ring_point(ring, in_lds ? s_list[an] : L[an], cap, width, head);
            const int m = min(64, ln - a0);
            for (int i = 0; i < m; ++i) {
                ax += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.x), i)); ay += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.y), i));
                az += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.z), i)); aw += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.w), i));
            }
            p = q;
        }
        const float c = (float)ln;
        if (lane == l) out[v] = make_float4(ax / c, ay / c, az / c, aw / c);
        GLIO_WAVE_LDS_SYNC();                                                // (s_list is refilled by the next list)
    }
}

// ------------------------------------------------------------------------------------------------
// Rebuild of the whole ring from resident keyframe clouds (glio_localmap_rebuild_from_frames): what n_frames pushes into a fresh ring do -- per frame a slot
// initialisation, transformCloud, the row's bounding box and the voxel accumulation, three to four launches each -- in TWO launches whatever n_frames is:
//   k_lm_rebuild_clear    the voxel table emptied; every slot's box and count initialised (slots behind n_frames: empty)
//   k_lm_rebuild_frames   blockIdx.y = frame: cloud_transform from the frame's cloud into ring row blockIdx.y, the row's box (one set of six atomics
//                         per workgroup), lm_table_add.  The sums are exact integers: whatever order the frames' workgroups run in, the table
//                         holds what the pushes would have left (keys may sit in other slots of the table: no reader depends on where).
// ------------------------------------------------------------------------------------------------
typedef float lm_v4f __attribute__((ext_vector_type(4)));
#define LM_RB_THREADS 256
#define LM_RB_PER 4            /* points per thread: a workgroup covers 1024 points of one frame */
__global__ void k_lm_rebuild_clear(unsigned long long* keys, long long* sum, int* cnt, int cap, int* nkeys, const LmFrame* __restrict__ fr, int n_frames, int width,
                                   int* slot_bbox, int* ns) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    lm_table_reset(i, keys, sum, cnt, cap, nkeys);
    if (i < 6 * width) slot_bbox[i] = (i % 6) < 3 ? 0x7fffffff : (int)0x80000000;
    if (i < width) ns[i] = i < n_frames ? fr[i].n : 0;
}
__global__ __launch_bounds__(LM_RB_THREADS) void k_lm_rebuild_frames(const LmFrame* __restrict__ fr, float4* __restrict__ ring, const int ring_cap, const float inv_leaf,
                                                                     unsigned long long* keys, long long* sum, int* cnt, const int cap, int* nkeys, int* slot_bbox) {
    __shared__ int s_box[LM_RB_THREADS / 64 * 6];
    const int f = blockIdx.y;
    const LmFrame d = fr[f];                                     // (uniform over the workgroup)
    const int base = blockIdx.x * (LM_RB_THREADS * LM_RB_PER);
    if (base >= d.n) return;                                     // (the whole workgroup: the grid is sized for the largest frame)
    float4* __restrict__ row = ring + (size_t)f * ring_cap;
    CloudBox b;
    b.init();
    float4 p[LM_RB_PER];
    // the clouds are read once: all of a thread's loads in flight together, past the caches' retention
#pragma unroll
    for (int k = 0; k < LM_RB_PER; ++k) {
        const int i = base + k * LM_RB_THREADS + (int)threadIdx.x;
        if (i < d.n) { const lm_v4f r = __builtin_nontemporal_load(reinterpret_cast<const lm_v4f*>(d.src + i)); p[k] = make_float4(r.x, r.y, r.z, r.w); }
    }
#pragma unroll
    for (int k = 0; k < LM_RB_PER; ++k) {
        const int i = base + k * LM_RB_THREADS + (int)threadIdx.x;
        if (i >= d.n) continue;
        const float4 g = cloud_transform(d.q, d.t, p[k]);
        row[i] = g;
        b.add(f2ord(g.x), f2ord(g.y), f2ord(g.z));
        lm_table_add(g, inv_leaf, +1, keys, sum, cnt, cap, nkeys);
    }
    b.commit<LM_RB_THREADS / 64>(s_box, slot_bbox + 6 * f);
}

#define LM_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { glio_set_error("%s failed: %s", #expr, hipGetErrorString(e_)); return GLIO_E_HIP; } } while (0)

static void lm_free(LocalMap* m) {
    if (!m) return;
    void* p[] = {m->d_slot_bbox, m->d_nkeys, m->d_n, m->d_ring, m->d_keys, m->d_sum, m->d_cnt, m->d_bbox, m->d_nvox, m->d_vkey, m->d_vkey_sorted, m->d_vslot, m->d_vslot_sorted, m->d_sort_tmp, m->d_out, m->d_fill, m->d_slot_start, m->d_plist, m->d_bm, m->d_bm_pre, m->d_bm_blk, m->d_bm_over};
    for (void* q : p) if (q) hipFree(q);
    if (m->h_pin) hipHostFree(m->h_pin);
    if (m->h_pub) hipHostFree(m->h_pub);
    if (m->h_frames) hipHostFree(m->h_frames);
    if (m->d_frames) hipFree(m->d_frames);
    if (m->ev_frames) hipEventDestroy(m->ev_frames);
    if (m->ev_dep) hipEventDestroy(m->ev_dep);
    if (m->ev_rb0) hipEventDestroy(m->ev_rb0);
    if (m->ev_rb1) hipEventDestroy(m->ev_rb1);
    delete[] m->h_n;
    delete m;
}
void glio_localmap_destroy(glio_ctx* c) {
    lm_free(c->localmap);
    c->localmap = nullptr;
}

// the buffers of a ring of m->width x m->cap points and of a voxel table for m->max_vox voxels (width, cap, leaf, max_vox set by the caller), cleared on `stream`
static int lm_alloc(LocalMap* m, hipStream_t stream) {
    const int width = m->width;
    m->table_cap = next_pow2(2 * m->max_vox);
    m->h_n = new int[width]();
    LM_CHECK(hipMalloc((void**)&m->d_n, (size_t)width * 4));
    LM_CHECK(hipMalloc((void**)&m->d_ring, (size_t)width * m->cap * 16));
    LM_CHECK(hipMalloc((void**)&m->d_keys, (size_t)m->table_cap * 8)); LM_CHECK(hipMalloc((void**)&m->d_sum, (size_t)m->table_cap * 32));
    LM_CHECK(hipMalloc((void**)&m->d_cnt, (size_t)m->table_cap * 4)); LM_CHECK(hipMalloc((void**)&m->d_bbox, 32)); LM_CHECK(hipMalloc((void**)&m->d_nvox, 4));
    LM_CHECK(hipMalloc((void**)&m->d_slot_bbox, (size_t)width * 24)); LM_CHECK(hipMalloc((void**)&m->d_nkeys, 4));
    LM_CHECK(hipMalloc((void**)&m->d_vkey, (size_t)m->max_vox * 8)); LM_CHECK(hipMalloc((void**)&m->d_vkey_sorted, (size_t)m->max_vox * 8));
    LM_CHECK(hipMalloc((void**)&m->d_vslot, (size_t)m->max_vox * 4)); LM_CHECK(hipMalloc((void**)&m->d_vslot_sorted, (size_t)m->max_vox * 4));
    LM_CHECK(hipMalloc((void**)&m->d_out, (size_t)m->max_vox * 16));
    m->sort_tmp_bytes = (size_t)256 * ((m->max_vox + RS_TILE - 1) / RS_TILE) * 4;          // digit histogram [256][tiles] of the radix sort
    LM_CHECK(hipMalloc(&m->d_sort_tmp, m->sort_tmp_bytes + 16));
    LM_CHECK(hipHostMalloc((void**)&m->h_pin, 64));
    LM_CHECK(hipHostMalloc((void**)&m->h_pub, 64));
    memset(m->h_pub, 0, 64);
    LM_CHECK(hipHostGetDevicePointer((void**)&m->d_h_pub, m->h_pub, 0));
    {   // occupancy bitmap of the bounding box + its running counts (GLIO_LM_SORT=1: the radix sort only)
        m->force_sort = glio_switch_at_create<GLIO_SW_LM_SORT>();
        LM_CHECK(hipMalloc((void**)&m->d_bm_over, 4));
        LM_CHECK(hipMemsetAsync(m->d_bm_over, 0, 4, stream));
        if (!m->force_sort) {
            const size_t words = (size_t)(BM_MAX_BITS / 32);
            LM_CHECK(hipMalloc((void**)&m->d_bm, words * 4)); LM_CHECK(hipMalloc((void**)&m->d_bm_pre, words * 4)); LM_CHECK(hipMalloc((void**)&m->d_bm_blk, 4096 * 4));
            LM_CHECK(hipMemsetAsync(m->d_bm, 0, words * 4, stream));
        }
    }
    hipLaunchKernelGGL(k_lm_clear, dim3((m->table_cap + 255) / 256), dim3(256), 0, stream, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    LM_CHECK(hipMemsetAsync(m->d_n, 0, (size_t)width * 4, stream));
    LM_CHECK(hipStreamSynchronize(stream));
    return GLIO_OK;
}
static int lm_set_accumulation(LocalMap* m, int mode) {
    if (mode == 1 && !m->d_plist) {
        LM_CHECK(hipMalloc((void**)&m->d_fill, (size_t)m->table_cap * 4)); LM_CHECK(hipMalloc((void**)&m->d_slot_start, (size_t)m->table_cap * 4));
        LM_CHECK(hipMalloc((void**)&m->d_plist, (size_t)m->width * m->cap * 4));
    }
    m->accumulation = mode;
    return GLIO_OK;
}

extern "C" {

int glio_localmap_config(glio_ctx* c, int width, float leaf, int max_points_per_keyframe) {
    if (!c || width < 1 || !(leaf > 0.f) || max_points_per_keyframe < 1) return GLIO_E_ARG;
    LM_CHECK(hipSetDevice(c->device));
    const int keep_accumulation = c->localmap ? c->localmap->accumulation : 0;      // (the centroid arithmetic is a property of the context, not of one ring)
    glio_localmap_destroy(c);
    LocalMap* m = new LocalMap();
    memset(m, 0, sizeof *m);
    m->width = width; m->cap = max_points_per_keyframe; m->leaf = leaf;
    m->max_vox = c->opts.max_map_points > 0 ? c->opts.max_map_points : 1;
    { const int ra = lm_alloc(m, c->stream); if (ra != GLIO_OK) { lm_free(m); return ra; } }
    c->localmap = m;
    if (keep_accumulation) return glio_localmap_set_accumulation(c, keep_accumulation);
    return GLIO_OK;
}

int glio_localmap_push(glio_ctx* c, const float* cloud_xyzi, int n, const double q[4], const double t[3]) { return glio_localmap_push_strided(c, cloud_xyzi, n, 16, 12, q, t); }
int glio_localmap_push_strided(glio_ctx* c, const void* cloud_xyzi, int n, int stride_bytes, int intensity_offset, const double q[4], const double t[3]) {
    if (!c || !c->localmap) { glio_set_error("glio_localmap_config first"); return GLIO_E_STATE; }
    LocalMap* m = c->localmap;
    if (n < 0 || n > m->cap || (n > 0 && !cloud_xyzi) || !q || !t) return GLIO_E_ARG;
    if (!glio_point_layout_ok(stride_bytes, intensity_offset)) { glio_set_error("bad point layout (stride %d, intensity at %d)", stride_bytes, intensity_offset); return GLIO_E_ARG; }
    LM_CHECK(hipSetDevice(c->device));
    const float inv_leaf = 1.0f / m->leaf;
    int slot;
    if (m->count < m->width) { slot = (m->head + m->count) % m->width; ++m->count; }
    else {                                                                        // recent_surf_keyframes.pop_front() (:3585):
        slot = m->head; m->head = (m->head + 1) % m->width;                       // take the oldest keyframe's points out of the table
        const int no = m->h_n[slot];
        if (no > 0) hipLaunchKernelGGL(k_lm_accumulate, dim3((no + 255) / 256), dim3(256), 0, c->stream, m->d_ring + (size_t)slot * m->cap, no, inv_leaf, -1,
                                       m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    }
    float4* dst = m->d_ring + (size_t)slot * m->cap;
    hipLaunchKernelGGL(k_lm_bbox_init, dim3(1), dim3(64), 0, c->stream, m->d_slot_bbox + 6 * slot, m->d_n + slot, n);
    if (n > 0) {
        // stage the raw scan in the destination itself, transform in place, then add it to the voxel table
        { const int ru = glio_upload_points(c->stream, &c->raw_stage, cloud_xyzi, n, stride_bytes, intensity_offset, dst); if (ru != GLIO_OK) return ru; }
        hipLaunchKernelGGL(k_lm_transform, dim3((n + 255) / 256), dim3(256), 0, c->stream, dst, n, q[0], q[1], q[2], q[3], t[0], t[1], t[2], dst);
        hipLaunchKernelGGL(k_lm_bbox, dim3(std::min(64, (n + 1023) / 1024)), dim3(1024), 0, c->stream, dst, n, m->d_slot_bbox + 6 * slot);
        hipLaunchKernelGGL(k_lm_accumulate, dim3((n + 255) / 256), dim3(256), 0, c->stream, dst, n, inv_leaf, +1, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    }
    LM_CHECK(hipGetLastError());
    LM_CHECK(hipStreamSynchronize(c->stream));            // the caller's buffer may be reused after return
    m->h_n[slot] = n;
    ++m->pushed;
    return GLIO_OK;
}

// The newest keyframe's cloud is usually on the device already -- glio_set_scan put it into window slot `slot` for the association.  This pushes THAT
// copy (LiDAR frame) into the ring: body-frame point = scan point - lidar_offset (float, the extrinsic translation with R_lb = I as a caller's float
// cloud would hold it), pose (q, t) of the body in the world.  No second upload of the same megabyte, no synchronisation.
int glio_localmap_push_scan(glio_ctx* c, int scan_slot, const float lidar_offset[3], const double q[4], const double t[3]) {
    if (!c || !c->localmap) { glio_set_error("glio_localmap_config first"); return GLIO_E_STATE; }
    LocalMap* m = c->localmap;
    if (scan_slot < 0 || scan_slot >= c->W || !lidar_offset || !q || !t) return GLIO_E_ARG;
    const int n = c->h_scan_count[scan_slot];
    if (n < 0 || n > m->cap) { glio_set_error("scan of slot %d has %d points, the ring takes %d", scan_slot, n, m->cap); return GLIO_E_ARG; }
    LM_CHECK(hipSetDevice(c->device));
    const float inv_leaf = 1.0f / m->leaf;
    int slot;
    if (m->count < m->width) { slot = (m->head + m->count) % m->width; ++m->count; }
    else {
        slot = m->head; m->head = (m->head + 1) % m->width;
        const int no = m->h_n[slot];
        if (no > 0) hipLaunchKernelGGL(k_lm_accumulate, dim3((no + 255) / 256), dim3(256), 0, c->stream, m->d_ring + (size_t)slot * m->cap, no, inv_leaf, -1,
                                       m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    }
    float4* dst = m->d_ring + (size_t)slot * m->cap;
    hipLaunchKernelGGL(k_lm_bbox_init, dim3(1), dim3(64), 0, c->stream, m->d_slot_bbox + 6 * slot, m->d_n + slot, n);
    if (n > 0) {
        hipLaunchKernelGGL(k_lm_transform_off, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_scan + (size_t)glio_scan_row(c, scan_slot) * c->cap, n, lidar_offset[0], lidar_offset[1],
                           lidar_offset[2], q[0], q[1], q[2], q[3], t[0], t[1], t[2], dst);
        hipLaunchKernelGGL(k_lm_bbox, dim3(std::min(64, (n + 1023) / 1024)), dim3(1024), 0, c->stream, dst, n, m->d_slot_bbox + 6 * slot);
        hipLaunchKernelGGL(k_lm_accumulate, dim3((n + 255) / 256), dim3(256), 0, c->stream, dst, n, inv_leaf, +1, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    }
    LM_CHECK(hipGetLastError());
    m->h_n[slot] = n;
    ++m->pushed;
    return GLIO_OK;
}

// The build needs three scalars on the host in its middle (voxel count, table fill, bounding box: the sort's geometry).  Three device-to-host copies and
// a stream synchronisation cost ~40 us of idle GPU there; one thread writing them into MAPPED host memory -- four 8-byte words, then a tag that carries the
// build's sequence number and a checksum of the words (writes to host memory have been seen out of order under load: glio_device.h, glio_result_mix) --
// and the host polling the tag cost ~10.  No match within 2 ms: the copies and the synchronisation, as before.
__global__ void k_lm_publish(const int* __restrict__ nvox, const int* __restrict__ nkeys, const int* __restrict__ bbox, const int* __restrict__ bm_over,
                             unsigned long long* out, const unsigned seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long w[4];
    const unsigned nk = (unsigned)nkeys[0] | (bm_over[0] ? 0x20000000u : 0u);          // (bit 30: voxel table overflow; bit 29: a voxel outside the bitmap)
    w[0] = (unsigned long long)(unsigned)nvox[0] | ((unsigned long long)nk << 32);
#pragma unroll
    for (int k = 0; k < 3; ++k) w[1 + k] = (unsigned long long)(unsigned)bbox[2 * k] | ((unsigned long long)(unsigned)bbox[2 * k + 1] << 32);
    unsigned long long cs = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cs += glio_result_mix(w[k], (unsigned long long)k);
#pragma unroll
    for (int k = 0; k < 4; ++k) __hip_atomic_store(out + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __hip_atomic_store(out + 4, (cs & 0xffffffff00000000ull) | seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
static bool lm_wait_published(LocalMap* m, int* out8) {
    const unsigned seq = m->pub_seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 1;; ++spins) {
        const unsigned long long tag = __atomic_load_n(m->h_pub + 4, __ATOMIC_ACQUIRE);
        if ((unsigned)(tag & 0xffffffffull) == seq) {
            unsigned long long w[4], cs = 0;
            for (int k = 0; k < 4; ++k) { w[k] = __atomic_load_n(m->h_pub + k, __ATOMIC_RELAXED); cs += glio_result_mix(w[k], (unsigned long long)k); }
            if ((cs & 0xffffffff00000000ull) == (tag & 0xffffffff00000000ull)) {
                out8[0] = (int)(unsigned)(w[0] & 0xffffffffull); out8[1] = (int)(unsigned)(w[0] >> 32);
                for (int k = 0; k < 3; ++k) { out8[2 + 2 * k] = (int)(unsigned)(w[1 + k] & 0xffffffffull); out8[3 + 2 * k] = (int)(unsigned)(w[1 + k] >> 32); }
                return true;
            }
        }
        if ((spins & 0xff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
    }
}

// pcl::VoxelGrid of the ring's concatenation into m->d_out on `stream` (the whole of the down-sampling: glio_localmap_build hands the result to K1, a
// loop-closure submap -- glio_vg_build below -- keeps it as it is); *nv_out = the voxels
static int lm_voxelize(LocalMap* m, hipStream_t stream, int* nv_out) {
    const float inv_leaf = 1.0f / m->leaf;
    // (the slots' point counts are on the device already: every push records its own, k_lm_bbox_init)
    m->last_path = 0; m->last_passes = 0; m->last_nv = 0;
    if (m->nkeys_seen > m->table_cap / 2) {               // too many tombstones (or a refused build, below): rebuild the table from the ring once
        ++m->n_table_rebuilds;
        hipLaunchKernelGGL(k_lm_clear, dim3((m->table_cap + 255) / 256), dim3(256), 0, stream, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
        for (int k = 0; k < m->count; ++k) {
            const int slot = (m->head + k) % m->width, n = m->h_n[slot];
            if (n > 0) hipLaunchKernelGGL(k_lm_accumulate, dim3((n + 255) / 256), dim3(256), 0, stream, m->d_ring + (size_t)slot * m->cap, n, inv_leaf, +1,
                                          m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
        }
    }
    if (m->d_bm && m->bm_dirty) {          // a build that ended between k_lm_list and its emit kernel (an error return) left bits behind
        LM_CHECK(hipMemsetAsync(m->d_bm, 0, (size_t)(BM_MAX_BITS / 32) * 4, stream));
        m->bm_dirty = 0;
        ++m->n_bm_wipes;
    }
    hipLaunchKernelGGL(k_lm_bbox_union, dim3(1), dim3(64), 0, stream, m->d_slot_bbox, m->d_n, m->width, m->d_bbox, m->d_bm_over, m->d_nvox);
    hipLaunchKernelGGL(k_lm_list, dim3((m->table_cap + 1023) / 1024), dim3(1024), 0, stream, m->d_keys, m->d_cnt, m->table_cap, inv_leaf, m->d_bbox,
                       m->d_nvox, m->d_vkey, m->d_vslot, m->max_vox, m->d_bm, (unsigned long long)BM_MAX_BITS, m->d_bm_over);
    LM_CHECK(hipGetLastError());
    if (m->d_bm) m->bm_dirty = 1;
    m->pub_seq = m->pub_seq == 0xffffffffu ? 1u : m->pub_seq + 1u;
    hipLaunchKernelGGL(k_lm_publish, dim3(1), dim3(64), 0, stream, m->d_nvox, m->d_nkeys, m->d_bbox, m->d_bm_over, m->d_h_pub, m->pub_seq);
    LM_CHECK(hipGetLastError());
    if (!lm_wait_published(m, m->h_pin)) {
        LM_CHECK(hipMemcpyAsync(m->h_pin, m->d_nvox, 4, hipMemcpyDeviceToHost, stream));
        LM_CHECK(hipMemcpyAsync(m->h_pin + 1, m->d_nkeys, 4, hipMemcpyDeviceToHost, stream));
        LM_CHECK(hipMemcpyAsync(m->h_pin + 2, m->d_bbox, 24, hipMemcpyDeviceToHost, stream));
        LM_CHECK(hipMemcpyAsync(m->h_pin + 8, m->d_bm_over, 4, hipMemcpyDeviceToHost, stream));
        LM_CHECK(hipStreamSynchronize(stream));
        if (m->h_pin[8]) m->h_pin[1] |= 0x20000000;
    }
    const bool bm_over = (m->h_pin[1] & 0x20000000) != 0;
    m->h_pin[1] &= ~0x20000000;
    const int nv = m->h_pin[0];
    // A refused build leaves the ring (clouds, counts, slot boxes) as the pushes made it, and the table to be reconstructed from it: nkeys_seen = table_cap
    // sends the next build through the rebuild above, which clears the overflow bit with the table.  After an overflow the table holds only part of the
    // ring, so nothing less will do; it succeeds as soon as the ring fits again and is refused again while it does not.
    if (m->h_pin[1] & 0x40000000) { m->nkeys_seen = m->table_cap; glio_set_error("local map voxel table overflow (raise max_map_points)"); return GLIO_E_ARG; }
    m->nkeys_seen = m->h_pin[1];
    m->last_nv = nv;
    m->last_passthrough = 0;
    if (m->pcl_overflow && nv > 0) {
        // pcl::VoxelGrid::applyFilter: (int64)((max - min) * inverse_leaf) + 1 per axis in float, a product above INT32_MAX leaves the cloud as it is.  (A factor
        // beyond 2^31 settles it before the cast; two factors below 2^31 multiply without overflow.)
        long long cells = 1;
        bool over = false;
        for (int c3 = 0; c3 < 3 && !over; ++c3) {
            const float ext = (h_ord2f(m->h_pin[5 + c3]) - h_ord2f(m->h_pin[2 + c3])) * inv_leaf;
            if (!(ext < 2147483648.0f)) { over = true; break; }
            cells *= (long long)ext + 1;
            if (cells > 2147483647ll) over = true;
        }
        if (over) { m->last_passthrough = 1; *nv_out = nv; return GLIO_OK; }      // (bm_dirty stays set: the next build wipes the bits k_lm_list left)
    }
    if (nv > m->max_vox) { m->nkeys_seen = m->table_cap; glio_set_error("local map has %d voxels, max_map_points is %d", nv, m->max_vox); return GLIO_E_ARG; }
    if (nv > 0) {
        // number of key bits from the bounding box, exactly as k_lm_list forms the linear index
        double span = 1.0;
        for (int c3 = 0; c3 < 3; ++c3) {
            const int lo = (int)floorf(h_ord2f(m->h_pin[2 + c3]) * inv_leaf), hi = (int)floorf(h_ord2f(m->h_pin[5 + c3]) * inv_leaf);
            span *= (double)(hi - lo + 1);
        }
        int* va = m->d_vslot;
        const unsigned long long* keys_final = m->d_vkey;          // every voxel's linear index, in whatever order: what the emit kernels clear the bitmap by
        const bool by_rank = m->d_bm && !bm_over && span <= (double)BM_MAX_BITS;
        if (by_rank) {
            const int nwords = (int)(((unsigned long long)span + 31ull) / 32ull), nblk = (nwords + 1023) / 1024;
            hipLaunchKernelGGL(k_bm_scan1, dim3(nblk), dim3(1024), 0, stream, m->d_bm, nwords, m->d_bm_pre, m->d_bm_blk);
            hipLaunchKernelGGL(k_bm_scan2, dim3(1), dim3(1024), 0, stream, m->d_bm_blk, nblk);
            hipLaunchKernelGGL(k_bm_rank, dim3((nv + 255) / 256), dim3(256), 0, stream, m->d_vkey, m->d_vslot, nv, m->d_bm, m->d_bm_pre, m->d_bm_blk, m->d_vslot_sorted);
            va = m->d_vslot_sorted;
            m->last_path = 1;
        } else {
            int bits = 1;
            while (bits < 63 && (double)(1ull << bits) < span) ++bits;
            const int passes = (bits + 7) / 8, nt = (nv + RS_TILE - 1) / RS_TILE;
            unsigned long long* ka = m->d_vkey; unsigned long long* kb = m->d_vkey_sorted;
            int* vb = m->d_vslot_sorted;
            int* hist = reinterpret_cast<int*>(m->d_sort_tmp);
            for (int p = 0; p < passes; ++p) {
                hipLaunchKernelGGL(k_rs_hist, dim3(nt), dim3(64), 0, stream, ka, nv, 8 * p, nt, hist);
                hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, stream, hist, nt);
                hipLaunchKernelGGL(k_rs_scatter, dim3(nt), dim3(64), 0, stream, ka, va, nv, 8 * p, nt, hist, kb, vb);
                std::swap(ka, kb); std::swap(va, vb);
            }
            keys_final = ka;
            m->last_path = 2; m->last_passes = passes;
        }
        LM_CHECK(hipGetLastError());
        if (m->accumulation == 1) {
            hipLaunchKernelGGL(k_lm_starts, dim3(1), dim3(1024), 0, stream, va, nv, m->d_cnt, m->d_slot_start);
            LM_CHECK(hipMemsetAsync(m->d_fill, 0, (size_t)m->table_cap * 4, stream));
            hipLaunchKernelGGL(k_lm_scatter_idx, dim3((m->cap + 255) / 256, m->width), dim3(256), 0, stream, m->d_ring, m->d_n, m->cap, m->width, m->head, m->count,
                               inv_leaf, m->d_keys, m->table_cap, m->d_slot_start, m->d_fill, m->d_plist);
            if (m->wave_emit)
                hipLaunchKernelGGL(k_lm_emit_wave, dim3((nv + LM_WAVE_VOX - 1) / LM_WAVE_VOX), dim3(64), 0, stream, va, nv, m->d_cnt, m->d_slot_start, m->d_plist, m->d_ring, m->cap,
                                   m->width, m->head, m->d_out, m->d_bm, keys_final, (unsigned long long)BM_MAX_BITS);
            else
            hipLaunchKernelGGL(k_lm_emit_float, dim3((nv + 255) / 256), dim3(256), 0, stream, va, nv, m->d_cnt, m->d_slot_start, m->d_plist, m->d_ring, m->cap, m->width,
                               m->head, m->d_out, m->d_bm, keys_final, (unsigned long long)BM_MAX_BITS);
        } else
        hipLaunchKernelGGL(k_lm_emit, dim3((nv + 255) / 256), dim3(256), 0, stream, va, nv, m->d_sum, m->d_cnt, m->d_out, m->d_bm, keys_final,
                           (unsigned long long)BM_MAX_BITS);     // (va: the sorted side after the last swap)
        m->bm_dirty = 0;
    } else m->bm_dirty = 0;
    *nv_out = nv;
    return GLIO_OK;
}

int glio_localmap_build(glio_ctx* c, int* out_points) {
    GLIO_TRACE("K1 glio_localmap_build (voxel grid + hash)");
    if (!c || !c->localmap) { glio_set_error("glio_localmap_config first"); return GLIO_E_STATE; }
    LocalMap* m = c->localmap;
    LM_CHECK(hipSetDevice(c->device));
    int nv = 0;
    { const int rv = lm_voxelize(m, c->stream, &nv); if (rv != GLIO_OK) return rv; }
    const int rc = glio_assoc_build_map_dev(c, m->d_out, nv);          // K1: replaces setInputCloud(surf_local_map_ds) (:2056)
    if (rc) return rc;
    // (no wait here: the map's size is known since the synchronisation above, and everything that reads the map -- the searches, glio_localmap_read --
    //  is ordered behind the build on this stream or waits for it)
    if (out_points) *out_points = nv;
    return GLIO_OK;
}

// buildLocalMapWithLandMark's rebuild branch (Estimator.cpp:3545-3579): the ring becomes the keyframes frame_idx[0..n) of `frames`' resident clouds at the caller's
// poses -- what n_frames glio_localmap_push of those clouds into a fresh ring and a glio_localmap_build leave, bit for bit -- in two launches (k_lm_rebuild_*)
// and the build's chain.  Everything that can be refused is refused before the first launch: the ring is never left half-written.
int glio_localmap_rebuild_from_frames(glio_ctx* c, glio_bassoc* frames, int n_frames, const int32_t* frame_idx, const double* poses, int* out_points) {
    GLIO_TRACE("K1 glio_localmap_rebuild_from_frames");
    if (!c || !c->localmap) { glio_set_error("glio_localmap_config first"); return GLIO_E_STATE; }
    LocalMap* m = c->localmap;
    GlioBassocView v;
    if (!frames || glio_bassoc_view(frames, &v) != GLIO_OK) { glio_set_error("glio_localmap_rebuild_from_frames: no batch association"); return GLIO_E_ARG; }
    if (v.device != c->device) { glio_set_error("glio_localmap_rebuild_from_frames: the batch association is on device %d, the context on %d", v.device, c->device); return GLIO_E_ARG; }
    if (n_frames < 1 || n_frames > m->width) { glio_set_error("glio_localmap_rebuild_from_frames: %d frames, the ring holds 1 .. %d", n_frames, m->width); return GLIO_E_ARG; }
    if (!frame_idx || !poses) { glio_set_error("glio_localmap_rebuild_from_frames: null frame list / poses"); return GLIO_E_ARG; }
    int max_n = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int k = frame_idx[f];
        if (k < 0 || k >= v.K) { glio_set_error("glio_localmap_rebuild_from_frames: frame %d outside [0, %d)", k, v.K); return GLIO_E_ARG; }
        if (v.h_n[k] < 1) { glio_set_error("glio_localmap_rebuild_from_frames: frame %d was never set (or holds no point)", k); return GLIO_E_ARG; }
        if (v.h_n[k] > m->cap) { glio_set_error("glio_localmap_rebuild_from_frames: frame %d has %d points, the ring takes %d", k, v.h_n[k], m->cap); return GLIO_E_ARG; }
        for (int e = 0; e < 7; ++e) if (!(fabs(poses[7 * f + e]) <= DBL_MAX)) { glio_set_error("glio_localmap_rebuild_from_frames: pose %d is not finite", f); return GLIO_E_ARG; }
        if (v.h_n[k] > max_n) max_n = v.h_n[k];
    }
    LM_CHECK(hipSetDevice(c->device));
    if (!m->h_frames) {
        LM_CHECK(hipHostMalloc((void**)&m->h_frames, (size_t)m->width * sizeof(LmFrame))); LM_CHECK(hipMalloc((void**)&m->d_frames, (size_t)m->width * sizeof(LmFrame)));
        LM_CHECK(hipEventCreateWithFlags(&m->ev_frames, hipEventDisableTiming)); LM_CHECK(hipEventCreateWithFlags(&m->ev_dep, hipEventDisableTiming));
        m->time_rebuild = glio_switch_at_create<GLIO_SW_LM_REBUILD_TIMING>();
        if (m->time_rebuild) { LM_CHECK(hipEventCreate(&m->ev_rb0)); LM_CHECK(hipEventCreate(&m->ev_rb1)); }
    }
    if (m->frames_in_flight) { LM_CHECK(hipEventSynchronize(m->ev_frames)); m->frames_in_flight = 0; }      // (the pinned table is rewritten only behind its last upload)
    for (int f = 0; f < n_frames; ++f) {
        LmFrame& d = m->h_frames[f];
        const int k = frame_idx[f];
        const double* ps = poses + 7 * f;                        // t[3], q[4] (w first)
        d.src = v.d_local + (size_t)k * v.cap; d.n = v.h_n[k]; d.pad_ = 0;
        for (int e = 0; e < 4; ++e) d.q[e] = ps[3 + e];
        for (int e = 0; e < 3; ++e) d.t[e] = ps[e];
    }
    // a scan / map sent ahead on the upload stream still writes the ring and the table: behind it (the rebuild supersedes that map; the scan stays for the next slide)
    { const int ra = glio_order_behind_ahead(c); if (ra != GLIO_OK) return ra; }
    // the association's pending frame copies come first -- for the context's stream, not for the host
    LM_CHECK(hipEventRecord(m->ev_dep, v.stream));
    LM_CHECK(hipStreamWaitEvent(c->stream, m->ev_dep, 0));
    LM_CHECK(hipMemcpyAsync(m->d_frames, m->h_frames, (size_t)n_frames * sizeof(LmFrame), hipMemcpyHostToDevice, c->stream));
    LM_CHECK(hipEventRecord(m->ev_frames, c->stream));
    m->frames_in_flight = 1;
    const float inv_leaf = 1.0f / m->leaf;
    if (m->time_rebuild) LM_CHECK(hipEventRecord(m->ev_rb0, c->stream));
    hipLaunchKernelGGL(k_lm_rebuild_clear, dim3((std::max(m->table_cap, 6 * m->width) + 255) / 256), dim3(256), 0, c->stream, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys,
                       m->d_frames, n_frames, m->width, m->d_slot_bbox, m->d_n);
    hipLaunchKernelGGL(k_lm_rebuild_frames, dim3((max_n + LM_RB_THREADS * LM_RB_PER - 1) / (LM_RB_THREADS * LM_RB_PER), n_frames), dim3(LM_RB_THREADS), 0, c->stream, m->d_frames,
                       m->d_ring, m->cap, inv_leaf, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys, m->d_slot_bbox);
    LM_CHECK(hipGetLastError());
    if (m->time_rebuild) { LM_CHECK(hipEventRecord(m->ev_rb1, c->stream)); m->have_rebuild_ms = 1; }
    // ... and the association must not overwrite a cloud before this has read it
    { const int re = glio_bassoc_external_read(frames, c->stream); if (re != GLIO_OK) return re; }
    m->head = 0; m->count = n_frames; m->pushed = n_frames; m->nkeys_seen = 0;          // a fresh ring after n_frames pushes: no tombstones
    for (int f = 0; f < m->width; ++f) m->h_n[f] = f < n_frames ? m->h_frames[f].n : 0;
    return glio_localmap_build(c, out_points);
}

// device time of the last rebuild's own two launches (table clear + the multi-frame kernel), ms -- only in a process started with GLIO_LM_REBUILD_TIMING=1
// (the events are not recorded otherwise: two event records per call are launch-rate money); GLIO_E_STATE without it or before a rebuild
int glio_localmap_last_rebuild_device_ms(glio_ctx* c, float* ms) {
    if (!c || !ms) return GLIO_E_ARG;
    LocalMap* m = c->localmap;
    if (!m || !m->time_rebuild || !m->have_rebuild_ms) { glio_set_error("no timed rebuild (GLIO_LM_REBUILD_TIMING=1, then glio_localmap_rebuild_from_frames)"); return GLIO_E_STATE; }
    LM_CHECK(hipSetDevice(c->device));
    LM_CHECK(hipEventSynchronize(m->ev_rb1));
    LM_CHECK(hipEventElapsedTime(ms, m->ev_rb0, m->ev_rb1));
    return GLIO_OK;
}
// 0 (default): exact fixed-point voxel sums (insert / evict without re-streaming the ring, bit-reproducible whatever the atomic order);
// 1: pcl::VoxelGrid's own arithmetic -- float sums over the voxel's points in the order of the concatenated cloud (the oracle's restatement): the centroids
// then equal the oracle's BIT FOR BIT, at the price of one pass over the ring per build.  For A/B runs of the 1.5e-5 m difference between the two.
int glio_localmap_set_accumulation(glio_ctx* c, int mode) {
    if (!c || !c->localmap || (mode != 0 && mode != 1)) { glio_set_error("glio_localmap_config first; mode 0 or 1"); return GLIO_E_ARG; }
    LocalMap* m = c->localmap;
    LM_CHECK(hipSetDevice(c->device));
    return lm_set_accumulation(m, mode);
}

// test hook (undeclared): which branches the local map has taken -- host fields only, no launch, no synchronisation.
// out[0] table_cap, [1] nkeys_seen, [2] table rebuilds from the ring since glio_localmap_config, [3] ordered-output path of the last build (0 empty,
// 1 bitmap rank, 2 radix sort), [4] its radix passes, [5] its voxels, [6] builds that wiped the whole bitmap after an interrupted one, [7] 0
int glio_debug_localmap_stats(glio_ctx* c, int32_t out[8]) {
    if (!c || !c->localmap || !out) return GLIO_E_ARG;
    const LocalMap* m = c->localmap;
    out[0] = m->table_cap; out[1] = m->nkeys_seen; out[2] = m->n_table_rebuilds; out[3] = m->last_path; out[4] = m->last_passes; out[5] = m->last_nv;
    out[6] = m->n_bm_wipes; out[7] = 0;
    return GLIO_OK;
}

int glio_localmap_read(glio_ctx* c, float* out_xyzi, int capacity, int* out_n) {
    if (!c || !c->localmap || !out_n) return GLIO_E_ARG;
    LM_CHECK(hipSetDevice(c->device));
    const int n = c->map_n;
    *out_n = n;
    if (out_xyzi && n > 0) {
        if (capacity < n) return GLIO_E_ARG;
        LM_CHECK(hipStreamSynchronize(c->stream));
        LM_CHECK(hipMemcpy(out_xyzi, c->localmap->d_out, (size_t)n * 16, hipMemcpyDeviceToHost));
    }
    return GLIO_OK;
}

}  // extern "C"

// ---- the same VoxelGrid for a caller that is not a context: a list of device-resident clouds, each moved by transformCloud (k_lm_transform: cloud_transform), concatenated in
// list order and filtered with the float accumulation (accumulation = 1: pcl::VoxelGrid's arithmetic and output order, the oracle's bit for bit).  The ring is
// used as a plain array of `width` slots, refilled by every build.  For the loop-closure submaps (loop_kernels.hip).
int glio_vg_create(int width, int cap, float leaf, int max_vox, hipStream_t stream, LocalMap** out) {
    LocalMap* m = new LocalMap();
    memset(m, 0, sizeof *m);
    m->width = width; m->cap = cap; m->leaf = leaf; m->max_vox = max_vox > 0 ? max_vox : 1;
    int rc = lm_alloc(m, stream);
    if (rc == GLIO_OK) rc = lm_set_accumulation(m, 1);
    if (rc != GLIO_OK) { lm_free(m); return rc; }
    *out = m;
    return GLIO_OK;
}
void glio_vg_destroy(LocalMap* m) { lm_free(m); }
void glio_vg_set_wave_emit(LocalMap* m, int on) { m->wave_emit = on ? 1 : 0; }
float4* glio_vg_staging(LocalMap* m) { return m->d_ring; }
int* glio_vg_staging_box(LocalMap* m) { return m->d_slot_bbox; }
const float4* glio_vg_output(LocalMap* m) { return m->d_out; }
int glio_vg_staged_begin(LocalMap* m, hipStream_t stream, int n) {
    if (n < 1 || n > m->cap) return GLIO_E_ARG;
    hipLaunchKernelGGL(k_lm_clear, dim3((m->table_cap + 255) / 256), dim3(256), 0, stream, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    if (m->width > 1) LM_CHECK(hipMemsetAsync(m->d_n, 0, (size_t)m->width * 4, stream));
    hipLaunchKernelGGL(k_lm_bbox_init, dim3(1), dim3(64), 0, stream, m->d_slot_bbox, m->d_n, n);
    LM_CHECK(hipGetLastError());
    m->head = 0; m->count = 1; m->nkeys_seen = 0; m->pcl_overflow = 1;
    for (int f = 0; f < m->width; ++f) m->h_n[f] = f == 0 ? n : 0;
    return GLIO_OK;
}
int glio_vg_staged_finish(LocalMap* m, hipStream_t stream, int n, float leaf, int* nv_out, int* passthrough) {
    if (n < 1 || n > m->cap || !(leaf > 0.f)) return GLIO_E_ARG;
    m->leaf = leaf;
    hipLaunchKernelGGL(k_lm_accumulate, dim3((n + 255) / 256), dim3(256), 0, stream, m->d_ring, n, 1.0f / leaf, +1, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    LM_CHECK(hipGetLastError());
    int nv = 0;
    { const int rv = lm_voxelize(m, stream, &nv); if (rv != GLIO_OK) return rv; }
    *passthrough = m->last_passthrough;
    *nv_out = m->last_passthrough ? n : nv;
    return GLIO_OK;
}
int glio_vg_build(LocalMap* m, hipStream_t stream, int n_frames, const float4* const* src, const int* n_src, const double* poses, float4* out, int out_cap, int* nv_out) {
    if (n_frames < 1 || n_frames > m->width) return GLIO_E_ARG;
    const float inv_leaf = 1.0f / m->leaf;
    hipLaunchKernelGGL(k_lm_clear, dim3((m->table_cap + 255) / 256), dim3(256), 0, stream, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
    LM_CHECK(hipMemsetAsync(m->d_n, 0, (size_t)m->width * 4, stream));
    m->head = 0; m->count = n_frames; m->nkeys_seen = 0;
    for (int f = 0; f < m->width; ++f) m->h_n[f] = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int n = n_src[f];
        if (n < 0 || n > m->cap) return GLIO_E_ARG;
        const double* ps = poses + 7 * f;            // t[3], q[4] (w first)
        float4* dst = m->d_ring + (size_t)f * m->cap;
        hipLaunchKernelGGL(k_lm_bbox_init, dim3(1), dim3(64), 0, stream, m->d_slot_bbox + 6 * f, m->d_n + f, n);
        if (n > 0) {
            hipLaunchKernelGGL(k_lm_transform, dim3((n + 255) / 256), dim3(256), 0, stream, src[f], n, ps[3], ps[4], ps[5], ps[6], ps[0], ps[1], ps[2], dst);
            hipLaunchKernelGGL(k_lm_bbox, dim3(std::min(64, (n + 1023) / 1024)), dim3(1024), 0, stream, dst, n, m->d_slot_bbox + 6 * f);
            hipLaunchKernelGGL(k_lm_accumulate, dim3((n + 255) / 256), dim3(256), 0, stream, dst, n, inv_leaf, +1, m->d_keys, m->d_sum, m->d_cnt, m->table_cap, m->d_nkeys);
        }
        m->h_n[f] = n;
    }
    LM_CHECK(hipGetLastError());
    int nv = 0;
    { const int rv = lm_voxelize(m, stream, &nv); if (rv != GLIO_OK) return rv; }
    *nv_out = nv;
    if (nv > out_cap) return GLIO_OK;                 // (the caller reports it)
    if (nv > 0) LM_CHECK(hipMemcpyAsync(out, m->d_out, (size_t)nv * 16, hipMemcpyDeviceToDevice, stream));
    return GLIO_OK;
}

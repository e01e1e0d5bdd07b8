// feature_kernels.hip -- LiDAR feature extraction from the raw scan on the device.
//
// Replaces Preprocessing::cloudHandler (reference GLIO/src/Preprocessing.cpp:353-681) after the ROS message parse: range / NaN filter,
// ring assignment, orientation with the halfPassed state machine, relTime, undistortion by qIMU, the stable bucketing by ring, the 11-point
// curvature, the six sectors of every ring with their greedy edge / flat picks and neighbour suppression, the less-flat points and the
// per-ring pcl::VoxelGrid.  The IMU integration that yields qIMU (processIMU / solveRotation, :202-259) stays on the host.
//
//   k_ft_count / k_ft_scan_tiles / k_ft_compact   the survivors of removeNaNFromPointCloud + removeClosedPointCloud, in order (tiles of 1024)
//   k_ft_project                                  scanID (or reject) and the first-branch orientation per survivor; halfPassed flips at the
//                                                 FIRST valid survivor whose first-branch ori - startOri > pi (an atomicMin of its index)
//   k_ft_deskew                                   the branch per point, relTime, intensity, undistortion, the rank among the tile's points of
//                                                 the same ring (ballots) and the tile's ring histogram
//   k_ft_scan_rings / k_ft_scatter                ring-major exclusive scan over (ring, tile): the stable bucketing, concatenated in ring order
//   k_ft_rings                                    ONE workgroup per ring: curvature, the sectors in order (sector j's marks reach into j + 1), the
//                                                 picks, the less-flat points, the ring's VoxelGrid
//   k_ft_gather                                   the per-ring outputs concatenated in ring order
//
// The greedy picks need no sort: the reference walks a sector sorted by curvature and takes every candidate that is not yet marked and passes
// the threshold; marks only ever get added, so its k-th pick is the extreme (curvature, index) among the candidates unmarked at that moment.
// Every pick is therefore one block-wide arg-max (edges, from the top) or arg-min (flats, from the bottom) over the sector, at most 11 + 4
// of them per sector.  Ties of the reference's unstable std::sort are ordered by (curvature, index) -- the one deviation.
#include <cfloat>
#include <climits>
#include <cstring>

#include "glio_device.h"
#include "cloud_device.h"

// the stencil, the neighbour gates, the voxel sums and the de-skew's double products round like the reference's scalar build
#pragma clang fp contract(off)

#define FT_TILE 1024
#define FT_MAX_RINGS 64
#define FT_SHARP_PER_RING 12        /* 2 per sector */
#define FT_LSHARP_PER_RING 60       /* 10 per sector */
#define FT_FLAT_PER_RING 24         /* 4 per sector (the 4th is kept, :609-613) */
#define FT_VG_LDS_KEYS 4096         /* a voxel-grid segment up to this size is sorted in LDS, a larger one in global memory */
#define FT_PI 3.14159265358979323846

// d_meta layout
enum { M_SURV = 0, M_HALF = 1, M_CUT = 2, M_SHARP = 3, M_LSHARP = 4, M_FLAT = 5, M_SURFN = 6, M_TS = 7,
       M_RSTART = 16, M_RSIZE = M_RSTART + FT_MAX_RINGS, M_RSH = M_RSIZE + FT_MAX_RINGS, M_RLS = M_RSH + FT_MAX_RINGS,
       M_RFL = M_RLS + FT_MAX_RINGS, M_RSU = M_RFL + FT_MAX_RINGS, M_WORDS = M_RSU + FT_MAX_RINGS };

struct FeatWork {
    glio_feat_opts o;
    int cap, nt_max;
    float4 *d_raw, *d_surv, *d_pt, *d_cut, *d_lf, *d_rsurf, *d_ts;
    float4 *d_rsharp, *d_rls, *d_rflat;                   // [64][12], [64][60], [64][24]: per-ring picks in pick order
    float4 *d_o_surf, *d_o_ls, *d_o_sharp, *d_o_flat;     // the outputs, concatenated in ring order
    float* d_ori; float* d_curv;
    int *d_ring, *d_rank, *d_tile, *d_hist, *d_pick, *d_label, *d_meta;
    unsigned long long* d_gkeys;                          // [2 cap] voxel-grid sort keys beyond the LDS path (ring r at 2 start_r: disjoint)
    int* h_meta;                                          // pinned
    hipEvent_t ev0, ev1;
    int have, ts_n;
    glio_feat_counts counts;
};

// ------------------------------------------------------------------------------------------------ block helpers (1024 threads = 16 wavefronts)
// (rank of a flag and exclusive scan of an int over the block: cloud_wg_rank<16>, cloud_wg_excl_scan<16>)
template <bool MAX> __device__ __forceinline__ unsigned long long ft_blk_ext(unsigned long long v, unsigned long long* s_red) {
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = MAX ? (o > v ? o : v) : (o < v ? o : v); }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = s_red[0];
    for (int k = 1; k < 16; ++k) { const unsigned long long o = s_red[k]; m = MAX ? (o > m ? o : m) : (o < m ? o : m); }
    __syncthreads();
    return m;
}
// ascending bitonic sort of N (a power of two) keys by the whole block; a[] in LDS or in global memory (__syncthreads orders both inside a workgroup)
__device__ void ft_bitonic(unsigned long long* a, const int N) {
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = a[i], y = a[l];
                    if ((i & k) == 0 ? x > y : x < y) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
}

// ------------------------------------------------------------------------------------------------ pcl::VoxelGrid of one segment, by one block
// The definition the CPU oracle restates (its voxel-grid routine): bounding box, min_b = floor(min * inv), voxel (int)(floor(x * inv) - min_b) per axis,
// linear index i + j div0 + k div0 div1, centroid of x y z intensity summed in FLOAT in input order, output ordered by voxel index.  PCL's overflow
// rule: (int64)((max - min) * inv) + 1 per axis, a product above INT32_MAX passes the segment through unfiltered.  Returns the output count.
__device__ int ft_voxel_grid(const float4* __restrict__ in, const int n, const float leaf, float4* __restrict__ out, unsigned long long* s_keys,
                             unsigned long long* g_keys, float* s_f, int* s_w) {
    if (n <= 0) return 0;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = tid; i < n; i += blockDim.x) {
        const float4 p = in[i];
        mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
        mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
    }
    for (int c = 0; c < 3; ++c)
        for (int off = 32; off > 0; off >>= 1) { mn[c] = fminf(mn[c], __shfl_xor(mn[c], off, 64)); mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off, 64)); }
    if (lane == 0) for (int c = 0; c < 3; ++c) { s_f[c * 16 + w] = mn[c]; s_f[48 + c * 16 + w] = mx[c]; }
    __syncthreads();
    for (int c = 0; c < 3; ++c) for (int k = 0; k < 16; ++k) { mn[c] = fminf(mn[c], s_f[c * 16 + k]); mx[c] = fmaxf(mx[c], s_f[48 + c * 16 + k]); }
    __syncthreads();
    const float inv = 1.0f / leaf;
    const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
    if (dx * dy * dz > (long long)INT_MAX) {
        for (int i = tid; i < n; i += blockDim.x) out[i] = in[i];
        return n;
    }
    int min_b[3], div_b[3];
    for (int c = 0; c < 3; ++c) { min_b[c] = (int)floorf(mn[c] * inv); div_b[c] = (int)floorf(mx[c] * inv) - min_b[c] + 1; }
    int N = 1;
    while (N < n) N <<= 1;
    unsigned long long* keys = N <= FT_VG_LDS_KEYS ? s_keys : g_keys;
    for (int i = tid; i < N; i += blockDim.x) {
        unsigned long long key = ~0ull;
        if (i < n) {
            const float4 p = in[i];
            const int i0 = (int)(floorf(p.x * inv) - (float)min_b[0]);
            const int i1 = (int)(floorf(p.y * inv) - (float)min_b[1]);
            const int i2 = (int)(floorf(p.z * inv) - (float)min_b[2]);
            const long long idx = (long long)i0 + (long long)i1 * div_b[0] + (long long)i2 * div_b[0] * (long long)div_b[1];
            key = ((unsigned long long)idx << 20) | (unsigned long long)i;          // (voxel, input position): unique keys, a stable order
        }
        keys[i] = key;
    }
    __syncthreads();
    ft_bitonic(keys, N);
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += blockDim.x) {
        const int s = c0 + tid;
        const bool head = s < n && (s == 0 || (keys[s] >> 20) != (keys[s - 1] >> 20));
        int tot;
        const int rk = cloud_wg_rank<16>(head, s_w, tot);
        if (head) {
            const unsigned long long v = keys[s] >> 20;
            float ax = 0.f, ay = 0.f, az = 0.f, ai = 0.f;
            int j = s;
            for (; j < n && (keys[j] >> 20) == v; ++j) {
                const float4 p = in[(int)(keys[j] & 0xFFFFFull)];
                ax += p.x; ay += p.y; az += p.z; ai += p.w;
            }
            const float cnt = (float)(j - s);
            out[base + rk] = make_float4(ax / cnt, ay / cnt, az / cnt, ai / cnt);
        }
        base += tot;
    }
    return base;
}

// ------------------------------------------------------------------------------------------------ survivors
__device__ __forceinline__ bool ft_keep(const float4 p, const float thr2) {
    // removeNaNFromPointCloud (x, y, z finite), then removeClosedPointCloud: x*x + y*y + z*z < thres*thres in float drops the point (:154-157)
    return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && !(p.x * p.x + p.y * p.y + p.z * p.z < thr2);
}
__global__ __launch_bounds__(1024) void k_ft_count(const float4* __restrict__ raw, const int n, const float thr2, int* __restrict__ tile_cnt) {
    __shared__ int s_w[16];
    const int i = blockIdx.x * FT_TILE + threadIdx.x;
    const bool keep = i < n && ft_keep(raw[i], thr2);
    int tot;
    cloud_wg_rank<16>(keep, s_w, tot);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_ft_scan_tiles(int* __restrict__ tile, const int nt, int* __restrict__ meta) {
    __shared__ int s_w[16];
    const int t = threadIdx.x;                         // nt <= 1024 (max_raw_points <= 400000)
    const int v = t < nt ? tile[t] : 0;
    int tot;
    const int ex = cloud_wg_excl_scan<16>(v, s_w, tot);
    if (t < nt) tile[t] = ex;
    if (t == 0) { meta[M_SURV] = tot; meta[M_HALF] = INT_MAX; }
}
__global__ __launch_bounds__(1024) void k_ft_compact(const float4* __restrict__ raw, const int n, const float thr2, const int* __restrict__ tile_off,
                                                     float4* __restrict__ surv) {
    __shared__ int s_w[16];
    const int i = blockIdx.x * FT_TILE + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = false;
    if (i < n) { p = raw[i]; keep = ft_keep(p, thr2); }
    int tot;
    const int rk = cloud_wg_rank<16>(keep, s_w, tot);
    if (keep) surv[tile_off[blockIdx.x] + rk] = p;
}

// ------------------------------------------------------------------------------------------------ projection
struct FtOri { float start, end; };
__device__ __forceinline__ FtOri ft_start_end(const float4* __restrict__ surv, const int ns) {
    // :401-410 from the first and the last survivor (atan2 of two floats is atan2f; the 2 pi terms are doubles)
    const float4 a = surv[0], b = surv[ns - 1];
    FtOri o;
    o.start = -atan2f(a.y, a.x);
    o.end = (float)((double)(-atan2f(b.y, b.x)) + 2 * FT_PI);
    if ((double)(o.end - o.start) > 3 * FT_PI) o.end = (float)((double)o.end - 2 * FT_PI);
    else if ((double)(o.end - o.start) < FT_PI) o.end = (float)((double)o.end + 2 * FT_PI);
    return o;
}
__device__ __forceinline__ float ft_first_branch(float ori, const float start_ori) {
    if ((double)ori < (double)start_ori - FT_PI / 2) ori = (float)((double)ori + 2 * FT_PI);
    else if ((double)ori > (double)start_ori + FT_PI * 3 / 2) ori = (float)((double)ori - 2 * FT_PI);
    return ori;
}
// scanID of :430-488 or -1 (angle = atan(z / sqrt(x*x + y*y)) * 180 / M_PI: atanf, sqrtf, a float product, a double quotient stored as float)
__device__ __forceinline__ int ft_scan_id(const float4 p, const int n_scans) {
    const float angle = (float)((double)(atanf(p.z / sqrtf(p.x * p.x + p.y * p.y)) * 180.0f) / FT_PI);
    int id;
    if (n_scans == 16) {
        id = (int)((double)((angle + 15.0f) / 2.0f) + 0.5);
        if (id > 15 || id < 0) return -1;
    } else if (n_scans == 32) {
        id = (int)(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
        if (id > 31 || id < 0) return -1;
    } else {
        if ((double)angle >= -8.83) id = (int)((double)(2.0f - angle) * 3.0 + 0.5);
        else id = 32 + (int)((-8.83 - (double)angle) * 2.0 + 0.5);
        if ((double)angle > 2 || (double)angle < -24.33 || id > 50 || id < 0) return -1;
    }
    return id;
}
__global__ __launch_bounds__(1024) void k_ft_project(const float4* __restrict__ surv, int* __restrict__ meta, const int n_scans,
                                                     int* __restrict__ ring, float* __restrict__ ori_raw) {
    const int ns = meta[M_SURV];
    const int i = blockIdx.x * FT_TILE + threadIdx.x;
    if (i >= ns) return;
    const float4 p = surv[i];
    const int id = ft_scan_id(p, n_scans);
    ring[i] = id;
    if (id < 0) return;
    const FtOri so = ft_start_end(surv, ns);
    const float o = -atan2f(p.y, p.x);
    ori_raw[i] = o;
    if ((double)(ft_first_branch(o, so.start) - so.start) > FT_PI) atomicMin(&meta[M_HALF], i);
}
__global__ __launch_bounds__(1024) void k_ft_deskew(const float4* __restrict__ surv, const int* __restrict__ meta, const int* __restrict__ ring,
                                                    const float* __restrict__ ori_raw, const double qw, const double qx, const double qy, const double qz,
                                                    const double lw, const double lx, const double ly, const double lz,
                                                    float4* __restrict__ pt, int* __restrict__ rank, int* __restrict__ hist) {
    __shared__ int s_cnt[16][FT_MAX_RINGS];
    const int ns = meta[M_SURV], half = meta[M_HALF];
    const int i = blockIdx.x * FT_TILE + threadIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < 16 * FT_MAX_RINGS; k += blockDim.x) s_cnt[k / FT_MAX_RINGS][k % FT_MAX_RINGS] = 0;
    const int r = i < ns ? ring[i] : -1;
    if (r >= 0) {
        const FtOri so = ft_start_end(surv, ns);
        float ori = ori_raw[i];
        if (i <= half) ori = ft_first_branch(ori, so.start);          // halfPassed is still false at the point that sets it (:500-507)
        else {
            ori = (float)((double)ori + 2 * FT_PI);
            if ((double)ori < (double)so.end - FT_PI * 3 / 2) ori = (float)((double)ori + 2 * FT_PI);
            else if ((double)ori > (double)so.end + FT_PI / 2) ori = (float)((double)ori - 2 * FT_PI);
        }
        const float rel = (ori - so.start) / (so.end - so.start);
        const float inten = (float)((double)r + 0.1 * (double)rel);                // :512
        // undistortion (:176-200): dt_i = intensity - int(intensity) in float, ratio capped at 1, Eigen's slerp from the identity, q_lb * q_si * q_lb^-1, q * v
        // (cloud_deskew_ratio, cloud_slerp_identity: cloud_device.h, shared with the keyframe cloud's de-skew)
        const double qimu[4] = {qw, qx, qy, qz};
        double qs[4];
        cloud_slerp_identity(qimu, cloud_deskew_ratio(inten), qs);
        const double ql[4] = {lw, lx, ly, lz};
        double qa[4], qi[4], qf[4];
        d_qmul(ql, qs, qa);
        d_qinv(ql, qi);
        d_qmul(qa, qi, qf);
        const float4 p = surv[i];
        const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
        double o[3];
        d_qrot(qf, v, o);
        pt[i] = make_float4((float)o[0], (float)o[1], (float)o[2], inten);
    }
    __syncthreads();
    // rank among the earlier points of the tile with the same ring: ballots on the ring's six bits inside the wavefront, wavefront counts in LDS
    unsigned long long same = __ballot(r >= 0);
    for (int b = 0; b < 6; ++b) {
        const unsigned long long bal = __ballot(r >= 0 && ((r >> b) & 1));
        same &= (r >= 0 && ((r >> b) & 1)) ? bal : ~bal;
    }
    const int rw = __popcll(same & ((1ull << lane) - 1ull));
    if (r >= 0 && rw == 0) s_cnt[w][r] = __popcll(same);
    __syncthreads();
    if (r >= 0) {
        int before = rw;
        for (int k = 0; k < w; ++k) before += s_cnt[k][r];
        rank[i] = before;
    }
    if (threadIdx.x < FT_MAX_RINGS) {
        int s = 0;
        for (int k = 0; k < 16; ++k) s += s_cnt[k][threadIdx.x];
        hist[blockIdx.x * FT_MAX_RINGS + threadIdx.x] = s;
    }
}
// ring-major exclusive scan of hist[tile][ring]: where tile t's points of ring r go; ring starts / sizes (:517-526) into meta
__global__ __launch_bounds__(1024) void k_ft_scan_rings(int* __restrict__ hist, const int nt, int* __restrict__ meta) {
    __shared__ int part[16][FT_MAX_RINGS], rbase[FT_MAX_RINGS];
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int per = (nt + 15) / 16, ta = min(nt, q * per), tb = min(nt, ta + per);
    int s = 0;
    for (int t = ta; t < tb; ++t) s += hist[t * FT_MAX_RINGS + r];
    part[q][r] = s;
    __syncthreads();
    if (threadIdx.x < 64) {
        int tot = 0;
        for (int k = 0; k < 16; ++k) tot += part[k][r];
        int incl = tot;
        for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (r >= off) incl += o; }
        rbase[r] = incl - tot;
        meta[M_RSTART + r] = incl - tot; meta[M_RSIZE + r] = tot;
        if (r == 63) meta[M_CUT] = incl;
    }
    __syncthreads();
    int run = rbase[r];
    for (int k = 0; k < q; ++k) run += part[k][r];
    for (int t = ta; t < tb; ++t) { const int x = hist[t * FT_MAX_RINGS + r]; hist[t * FT_MAX_RINGS + r] = run; run += x; }
}
__global__ __launch_bounds__(1024) void k_ft_scatter(const float4* __restrict__ pt, const int* __restrict__ meta, const int* __restrict__ ring,
                                                     const int* __restrict__ rank, const int* __restrict__ hist, float4* __restrict__ cut) {
    const int i = blockIdx.x * FT_TILE + threadIdx.x;
    if (i >= meta[M_SURV]) return;
    const int r = ring[i];
    if (r < 0) return;
    cut[hist[blockIdx.x * FT_MAX_RINGS + r] + rank[i]] = pt[i];
}

// ------------------------------------------------------------------------------------------------ one workgroup per ring
// neighbour suppression (:579-596, :618-635): +-5 while the float squared step stays <= 0.05 (a double comparison).  ind -+ 5 stays in the ring.
__device__ __forceinline__ void ft_mark(const float4* __restrict__ cut, int* __restrict__ pick, const int ind) {
    float4 q[11];
#pragma unroll
    for (int l = 0; l < 11; ++l) q[l] = cut[ind - 5 + l];
    for (int l = 1; l <= 5; ++l) {
        const float dx = q[5 + l].x - q[4 + l].x, dy = q[5 + l].y - q[4 + l].y, dz = q[5 + l].z - q[4 + l].z;
        if ((double)(dx * dx + dy * dy + dz * dz) > 0.05) break;
        pick[ind + l] = 1;
    }
    for (int l = -1; l >= -5; --l) {
        const float dx = q[5 + l].x - q[6 + l].x, dy = q[5 + l].y - q[6 + l].y, dz = q[5 + l].z - q[6 + l].z;
        if ((double)(dx * dx + dy * dy + dz * dz) > 0.05) break;
        pick[ind + l] = 1;
    }
}
__device__ __forceinline__ bool ft_near(const float4 p) { return (double)(p.x * p.x + p.y * p.y + p.z * p.z) < 0.25; }     // :603, :641
__global__ __launch_bounds__(1024) void k_ft_rings(const float4* __restrict__ cut, int* __restrict__ meta, const int ds_rate, const double edge_thr,
                                                   const double surf_thr, const float leaf, float* __restrict__ curv, int* __restrict__ pick,
                                                   int* __restrict__ label, float4* __restrict__ lf, float4* __restrict__ rsurf,
                                                   float4* __restrict__ rsharp, float4* __restrict__ rls, float4* __restrict__ rflat,
                                                   unsigned long long* __restrict__ gkeys) {
    __shared__ unsigned long long s_keys[FT_VG_LDS_KEYS];
    __shared__ unsigned long long s_red[16];
    __shared__ float s_f[96];
    __shared__ int s_w[16];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int start = meta[M_RSTART + r], size = meta[M_RSIZE + r];
    const int S = start + 5, E = start + size - 6;                      // scanStartInd / scanEndInd (:522-526)
    int n_sh = 0, n_ls = 0, n_fl = 0, n_lf = 0;                         // (the pick counts live in thread 0)
    if (E - S < 6 || r % ds_rate != 0) {                                // :542
        if (tid == 0) { meta[M_RSH + r] = 0; meta[M_RLS + r] = 0; meta[M_RFL + r] = 0; meta[M_RSU + r] = 0; }
        return;
    }
    // the curvature (:529-538) of the points the sectors cover: the stencil reads start .. start + size - 2, never another ring
    for (int i = S + tid; i < E; i += blockDim.x) {
        float dx = cut[i - 5].x, dy = cut[i - 5].y, dz = cut[i - 5].z;
        for (int l = -4; l <= -1; ++l) { dx += cut[i + l].x; dy += cut[i + l].y; dz += cut[i + l].z; }
        dx -= 10.0f * cut[i].x; dy -= 10.0f * cut[i].y; dz -= 10.0f * cut[i].z;
        for (int l = 1; l <= 5; ++l) { dx += cut[i + l].x; dy += cut[i + l].y; dz += cut[i + l].z; }
        curv[i] = dx * dx + dy * dy + dz * dz;
        pick[i] = 0; label[i] = 0;
    }
    __syncthreads();
    for (int j = 0; j < 6; ++j) {
        const int sp = S + (E - S) * j / 6, ep = S + (E - S) * (j + 1) / 6 - 1;          // :550-551
        // edges from the top (:557-598): 2 sharp, then less sharp up to the 10th, break on the 11th
        for (int picked = 1;; ++picked) {
            unsigned long long best = 0;                               // (keys are >= 5: index >= 5)
            for (int k = sp + tid; k <= ep; k += blockDim.x) {
                const float cv = curv[k];
                if (pick[k] == 0 && (double)cv > edge_thr) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(cv) << 32) | (unsigned)k;     // curvature >= 0: bits order = value order
                    best = key > best ? key : best;
                }
            }
            best = ft_blk_ext<true>(best, s_red);
            if (best == 0 || picked > 10) break;
            const int ind = (int)(unsigned)best;
            if (tid == 0) {
                label[ind] = picked <= 2 ? 2 : 1;
                if (picked <= 2) rsharp[r * FT_SHARP_PER_RING + n_sh++] = cut[ind];
                rls[r * FT_LSHARP_PER_RING + n_ls++] = cut[ind];
                pick[ind] = 1;
                ft_mark(cut, pick, ind);
            }
            __syncthreads();
        }
        // flats from the bottom (:600-637): points with norm^2 < 0.25 skipped, the 4th pick breaks before it marks anything
        for (int picked = 1; picked <= 4; ++picked) {
            unsigned long long best = ~0ull;
            for (int k = sp + tid; k <= ep; k += blockDim.x) {
                const float cv = curv[k];
                if (pick[k] == 0 && (double)cv < surf_thr && !ft_near(cut[k])) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(cv) << 32) | (unsigned)k;
                    best = key < best ? key : best;
                }
            }
            best = ft_blk_ext<false>(best, s_red);
            if (best == ~0ull) break;
            const int ind = (int)(unsigned)best;
            if (tid == 0) {
                label[ind] = -1;
                rflat[r * FT_FLAT_PER_RING + n_fl++] = cut[ind];
                if (picked < 4) { pick[ind] = 1; ft_mark(cut, pick, ind); }
            }
            __syncthreads();
        }
        // less-flat points of the sector in index order (:639-645)
        for (int c0 = sp; c0 <= ep; c0 += blockDim.x) {
            const int k = c0 + tid;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
            bool f = false;
            if (k <= ep) { p = cut[k]; f = !ft_near(p) && label[k] <= 0; }
            int tot;
            const int rk = cloud_wg_rank<16>(f, s_w, tot);
            if (f) lf[start + n_lf + rk] = p;
            n_lf += tot;
        }
    }
    __syncthreads();
    // pcl::VoxelGrid over the ring's less-flat cloud with its own bounding box (:648-652)
    const int nsu = ft_voxel_grid(lf + start, n_lf, leaf, rsurf + start, s_keys, gkeys + 2 * (size_t)start, s_f, s_w);
    if (tid == 0) { meta[M_RSH + r] = n_sh; meta[M_RLS + r] = n_ls; meta[M_RFL + r] = n_fl; meta[M_RSU + r] = nsu; }
}
// the per-ring outputs concatenated in ring order (:654 and the push_backs into the whole-scan clouds)
__global__ __launch_bounds__(256) void k_ft_gather(int* __restrict__ meta, const int n_rings, const float4* __restrict__ rsharp, const float4* __restrict__ rls,
                                                   const float4* __restrict__ rflat, const float4* __restrict__ rsurf, float4* __restrict__ o_sharp,
                                                   float4* __restrict__ o_ls, float4* __restrict__ o_flat, float4* __restrict__ o_surf) {
    const int r = blockIdx.x;
    int osh = 0, ols = 0, ofl = 0, osu = 0;
    for (int k = 0; k < r; ++k) { osh += meta[M_RSH + k]; ols += meta[M_RLS + k]; ofl += meta[M_RFL + k]; osu += meta[M_RSU + k]; }
    const int nsh = meta[M_RSH + r], nls = meta[M_RLS + r], nfl = meta[M_RFL + r], nsu = meta[M_RSU + r];
    for (int i = threadIdx.x; i < nsh; i += blockDim.x) o_sharp[osh + i] = rsharp[r * FT_SHARP_PER_RING + i];
    for (int i = threadIdx.x; i < nls; i += blockDim.x) o_ls[ols + i] = rls[r * FT_LSHARP_PER_RING + i];
    for (int i = threadIdx.x; i < nfl; i += blockDim.x) o_flat[ofl + i] = rflat[r * FT_FLAT_PER_RING + i];
    const int rs = meta[M_RSTART + r];
    for (int i = threadIdx.x; i < nsu; i += blockDim.x) o_surf[osu + i] = rsurf[rs + i];
    if (r == n_rings - 1 && threadIdx.x == 0) { meta[M_SHARP] = osh + nsh; meta[M_LSHARP] = ols + nls; meta[M_FLAT] = ofl + nfl; meta[M_SURFN] = osu + nsu; }
}
// LidarOdometry's downSampleCloud: the same voxel grid over one segment (the whole surf cloud)
__global__ __launch_bounds__(1024) void k_ft_voxel_one(const float4* __restrict__ in, const int n, const float leaf, float4* __restrict__ out,
                                                       int* __restrict__ meta, unsigned long long* __restrict__ gkeys) {
    __shared__ unsigned long long s_keys[FT_VG_LDS_KEYS];
    __shared__ float s_f[96];
    __shared__ int s_w[16];
    const int nv = ft_voxel_grid(in, n, leaf, out, s_keys, gkeys, s_f, s_w);
    if (threadIdx.x == 0) meta[M_TS] = nv;
}

// ------------------------------------------------------------------------------------------------ host side
static void ft_free(FeatWork* f) {
    void* p[] = {f->d_raw, f->d_surv, f->d_pt, f->d_cut, f->d_lf, f->d_rsurf, f->d_ts, f->d_rsharp, f->d_rls, f->d_rflat, f->d_o_surf, f->d_o_ls, f->d_o_sharp,
                 f->d_o_flat, f->d_ori, f->d_curv, f->d_ring, f->d_rank, f->d_tile, f->d_hist, f->d_pick, f->d_label, f->d_meta, f->d_gkeys};
    for (void* q : p) if (q) hipFree(q);
    if (f->h_meta) hipHostFree(f->h_meta);
    if (f->ev0) hipEventDestroy(f->ev0);
    if (f->ev1) hipEventDestroy(f->ev1);
    delete f;
}
void glio_features_destroy(glio_ctx* c) {
    // (another context's keyframe cloud stage may still be reading the surf features: glio_set_scan_from_features)
    if (c->feat_read_pending) { hipEventSynchronize(c->ev_feat_read); c->feat_read_pending = 0; }
    if (c->cut_read_pending) { hipEventSynchronize(c->ev_cut_read); c->cut_read_pending = 0; }      // (... or a dense store the cut cloud)
    if (c->features) { ft_free(c->features); c->features = nullptr; }
}
int glio_features_surf_view(glio_ctx* c, const float4** d_surf, int* n) {
    FeatWork* f = c->features;
    if (!f || !f->have) { glio_set_error("glio_features_extract first"); return GLIO_E_STATE; }
    *d_surf = f->d_o_surf; *n = f->counts.surf;
    return GLIO_OK;
}

int glio_features_cut_view(glio_ctx* c, const float4** d_cut, int* n) {
    FeatWork* f = c->features;
    if (!f || !f->have) { glio_set_error("glio_features_extract first"); return GLIO_E_STATE; }
    *d_cut = f->d_cut; *n = f->counts.cut;
    return GLIO_OK;
}
int glio_features_cut_external_read(glio_ctx* c, hipStream_t reader) {
    if (!c->ev_cut_read) GLIO_HIP_CHECK(hipEventCreateWithFlags(&c->ev_cut_read, hipEventDisableTiming));
    if (c->cut_read_pending) GLIO_HIP_CHECK(hipStreamWaitEvent(reader, c->ev_cut_read, 0));       // (another store's read: the new record covers it)
    GLIO_HIP_CHECK(hipEventRecord(c->ev_cut_read, reader));
    c->cut_read_pending = 1;
    return GLIO_OK;
}

#define FT_ALLOC(ptr, bytes) GLIO_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes)))

extern "C" {

void glio_feat_opts_default(glio_feat_opts* o) {
    memset(o, 0, sizeof *o);
    o->n_scans = 32;                    // config_urban_hk.yaml: line_num
    o->ds_rate = 1;                     // ds_rate
    o->edge_threshold = 1.0;            // edgeThreshold
    o->surf_threshold = 0.1;            // surfThreshold
    o->ds_leaf = 0.4f;                  // Preprocessing::ds_v (:14)
    o->min_range = 3.0f;                // removeClosedPointCloud(.., 3.0) (:397)
    o->q_lb[0] = 1.0;                   // ql2b_w/x/y/z: identity
    o->max_raw_points = GLIO_FEAT_MAX_RAW_POINTS;
}

int glio_feat_struct_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(glio_feat_opts), (int32_t)sizeof(glio_feat_counts)};
    for (int i = 0; i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

static int ft_config_body(glio_ctx* c, FeatWork* f) {
    const size_t cap = (size_t)f->cap, f4 = sizeof(float4);
    FT_ALLOC(f->d_raw, cap * f4); FT_ALLOC(f->d_surv, cap * f4); FT_ALLOC(f->d_pt, cap * f4); FT_ALLOC(f->d_cut, cap * f4);
    FT_ALLOC(f->d_lf, cap * f4); FT_ALLOC(f->d_rsurf, cap * f4); FT_ALLOC(f->d_ts, cap * f4); FT_ALLOC(f->d_o_surf, cap * f4);
    FT_ALLOC(f->d_rsharp, FT_MAX_RINGS * FT_SHARP_PER_RING * f4); FT_ALLOC(f->d_rls, FT_MAX_RINGS * FT_LSHARP_PER_RING * f4);
    FT_ALLOC(f->d_rflat, FT_MAX_RINGS * FT_FLAT_PER_RING * f4); FT_ALLOC(f->d_o_sharp, FT_MAX_RINGS * FT_SHARP_PER_RING * f4);
    FT_ALLOC(f->d_o_ls, FT_MAX_RINGS * FT_LSHARP_PER_RING * f4); FT_ALLOC(f->d_o_flat, FT_MAX_RINGS * FT_FLAT_PER_RING * f4);
    FT_ALLOC(f->d_ori, cap * 4); FT_ALLOC(f->d_curv, cap * 4); FT_ALLOC(f->d_ring, cap * 4); FT_ALLOC(f->d_rank, cap * 4);
    FT_ALLOC(f->d_pick, cap * 4); FT_ALLOC(f->d_label, cap * 4);
    FT_ALLOC(f->d_tile, (size_t)f->nt_max * 4); FT_ALLOC(f->d_hist, (size_t)f->nt_max * FT_MAX_RINGS * 4);
    FT_ALLOC(f->d_meta, M_WORDS * 4); FT_ALLOC(f->d_gkeys, 2 * cap * sizeof(unsigned long long));
    GLIO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&f->h_meta), M_WORDS * 4, hipHostMallocDefault));
    GLIO_HIP_CHECK(hipEventCreate(&f->ev0)); GLIO_HIP_CHECK(hipEventCreate(&f->ev1));
    GLIO_HIP_CHECK(hipMemsetAsync(f->d_meta, 0, M_WORDS * 4, c->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GLIO_OK;
}

int glio_features_config(glio_ctx* c, const glio_feat_opts* o) {
    if (!c || !o) return GLIO_E_ARG;
    if ((o->n_scans != 16 && o->n_scans != 32 && o->n_scans != 64) || o->ds_rate < 1 || !(o->ds_leaf > 0.f) ||
        o->max_raw_points < 1 || o->max_raw_points > GLIO_FEAT_MAX_RAW_POINTS) {
        glio_set_error("bad glio_feat_opts (n_scans %d, ds_rate %d, ds_leaf %g, max_raw_points %d)", o->n_scans, o->ds_rate, (double)o->ds_leaf, o->max_raw_points);
        return GLIO_E_ARG;
    }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    GLIO_HIP_CHECK(hipStreamSynchronize(c->stream));
    glio_features_destroy(c);
    FeatWork* f = new FeatWork();
    memset(f, 0, sizeof *f);
    f->o = *o;
    f->cap = o->max_raw_points;
    f->nt_max = (f->cap + FT_TILE - 1) / FT_TILE;
    const int rc = ft_config_body(c, f);
    if (rc != GLIO_OK) { ft_free(f); return rc; }
    c->features = f;
    return GLIO_OK;
}

int glio_features_extract_strided(glio_ctx* c, const void* raw, int n, int stride_bytes, int intensity_offset, const double q_imu[4], glio_feat_counts* counts) {
    GLIO_TRACE("glio_features_extract");
    if (!c) return GLIO_E_ARG;
    FeatWork* f = c->features;
    if (!f) { glio_set_error("glio_features_config first"); return GLIO_E_STATE; }
    if (n < 0 || n > f->cap || (n > 0 && !raw) || !q_imu) { glio_set_error("bad raw scan (n %d, capacity %d)", n, f->cap); return GLIO_E_ARG; }
    if (!glio_point_layout_ok(stride_bytes, intensity_offset)) { glio_set_error("bad point layout (stride %d, intensity at %d)", stride_bytes, intensity_offset); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // (a keyframe cloud stage on another stream may still be reading the last extraction's surf features: this one overwrites them behind that read)
    if (c->feat_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, c->ev_feat_read, 0)); c->feat_read_pending = 0; }
    // (... and a dense store the cut cloud: its own event, so that neither read hides the other)
    if (c->cut_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, c->ev_cut_read, 0)); c->cut_read_pending = 0; }
    { const int ru = glio_upload_points(s, &c->raw_stage, raw, n, stride_bytes, intensity_offset, f->d_raw); if (ru != GLIO_OK) return ru; }
    GLIO_HIP_CHECK(hipEventRecord(f->ev0, s));
    const int nt = (n + FT_TILE - 1) / FT_TILE, ntl = nt > 0 ? nt : 1;
    const float thr = f->o.min_range, thr2 = thr * thr;
    const int R = f->o.n_scans;
    if (n > 0) hipLaunchKernelGGL(k_ft_count, dim3(nt), dim3(FT_TILE), 0, s, f->d_raw, n, thr2, f->d_tile);
    else GLIO_HIP_CHECK(hipMemsetAsync(f->d_tile, 0, 4, s));
    hipLaunchKernelGGL(k_ft_scan_tiles, dim3(1), dim3(1024), 0, s, f->d_tile, ntl, f->d_meta);
    if (n > 0) {
        hipLaunchKernelGGL(k_ft_compact, dim3(nt), dim3(FT_TILE), 0, s, f->d_raw, n, thr2, f->d_tile, f->d_surv);
        hipLaunchKernelGGL(k_ft_project, dim3(nt), dim3(FT_TILE), 0, s, f->d_surv, f->d_meta, R, f->d_ring, f->d_ori);
        hipLaunchKernelGGL(k_ft_deskew, dim3(nt), dim3(FT_TILE), 0, s, f->d_surv, f->d_meta, f->d_ring, f->d_ori, q_imu[0], q_imu[1], q_imu[2], q_imu[3],
                           f->o.q_lb[0], f->o.q_lb[1], f->o.q_lb[2], f->o.q_lb[3], f->d_pt, f->d_rank, f->d_hist);
    } else GLIO_HIP_CHECK(hipMemsetAsync(f->d_hist, 0, FT_MAX_RINGS * 4, s));
    hipLaunchKernelGGL(k_ft_scan_rings, dim3(1), dim3(1024), 0, s, f->d_hist, ntl, f->d_meta);
    if (n > 0) hipLaunchKernelGGL(k_ft_scatter, dim3(nt), dim3(FT_TILE), 0, s, f->d_pt, f->d_meta, f->d_ring, f->d_rank, f->d_hist, f->d_cut);
    hipLaunchKernelGGL(k_ft_rings, dim3(R), dim3(1024), 0, s, f->d_cut, f->d_meta, f->o.ds_rate, f->o.edge_threshold, f->o.surf_threshold, f->o.ds_leaf,
                       f->d_curv, f->d_pick, f->d_label, f->d_lf, f->d_rsurf, f->d_rsharp, f->d_rls, f->d_rflat, f->d_gkeys);
    hipLaunchKernelGGL(k_ft_gather, dim3(R), dim3(256), 0, s, f->d_meta, R, f->d_rsharp, f->d_rls, f->d_rflat, f->d_rsurf, f->d_o_sharp, f->d_o_ls,
                       f->d_o_flat, f->d_o_surf);
    GLIO_HIP_CHECK(hipGetLastError());
    GLIO_HIP_CHECK(hipEventRecord(f->ev1, s));
    GLIO_HIP_CHECK(hipMemcpyAsync(f->h_meta, f->d_meta, 8 * 4, hipMemcpyDeviceToHost, s));
    GLIO_HIP_CHECK(hipStreamSynchronize(s));
    glio_feat_counts k;
    memset(&k, 0, sizeof k);
    k.in = n; k.kept = f->h_meta[M_SURV]; k.cut = f->h_meta[M_CUT]; k.sharp = f->h_meta[M_SHARP]; k.less_sharp = f->h_meta[M_LSHARP];
    k.flat = f->h_meta[M_FLAT]; k.surf = f->h_meta[M_SURFN];
    f->counts = k;
    f->have = 1;
    if (counts) *counts = k;
    return GLIO_OK;
}
int glio_features_extract(glio_ctx* c, const float* xyzi, int n, const double q_imu[4], glio_feat_counts* counts) {
    return glio_features_extract_strided(c, xyzi, n, 16, 12, q_imu, counts);
}

int glio_features_read(glio_ctx* c, int which, float* out, int capacity, int* n_out) {
    if (!c) return GLIO_E_ARG;
    FeatWork* f = c->features;
    if (!f) { glio_set_error("glio_features_config first"); return GLIO_E_STATE; }
    const float4* src = nullptr;
    int n = 0;
    switch (which) {
        case GLIO_FEAT_SURF: src = f->d_o_surf; n = f->counts.surf; break;
        case GLIO_FEAT_EDGE_LESS_SHARP: src = f->d_o_ls; n = f->counts.less_sharp; break;
        case GLIO_FEAT_SHARP: src = f->d_o_sharp; n = f->counts.sharp; break;
        case GLIO_FEAT_FLAT: src = f->d_o_flat; n = f->counts.flat; break;
        case GLIO_FEAT_CUT_CLOUD: src = f->d_cut; n = f->counts.cut; break;
        case GLIO_FEAT_LAST_SCAN: src = f->d_ts; n = f->ts_n; break;
        default: glio_set_error("unknown feature output %d", which); return GLIO_E_ARG;
    }
    if (!f->have) n = 0;
    if (n_out) *n_out = n;
    if (!out) return GLIO_OK;
    if (n > capacity) { glio_set_error("capacity %d < count %d", capacity, n); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    if (n > 0) GLIO_HIP_CHECK(hipMemcpyAsync(out, src, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GLIO_OK;
}

int glio_features_to_scan(glio_ctx* c, int slot, float leaf, int* n_out) {
    GLIO_TRACE("glio_features_to_scan");
    if (!c || slot < 0 || slot >= c->W) { glio_set_error("bad slot"); return GLIO_E_ARG; }
    FeatWork* f = c->features;
    if (!f || !f->have) { glio_set_error("glio_features_extract first"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int ns = f->counts.surf;
    int nv = ns;
    if (leaf > 0.f && ns > 0) {
        hipLaunchKernelGGL(k_ft_voxel_one, dim3(1), dim3(1024), 0, s, f->d_o_surf, ns, leaf, f->d_ts, f->d_meta, f->d_gkeys);
        GLIO_HIP_CHECK(hipGetLastError());
        GLIO_HIP_CHECK(hipMemcpyAsync(f->h_meta + M_TS, f->d_meta + M_TS, 4, hipMemcpyDeviceToHost, s));
        GLIO_HIP_CHECK(hipStreamSynchronize(s));
        nv = f->h_meta[M_TS];
    } else if (ns > 0) GLIO_HIP_CHECK(hipMemcpyAsync(f->d_ts, f->d_o_surf, (size_t)ns * 16, hipMemcpyDeviceToDevice, s));
    f->ts_n = nv;
    if (n_out) *n_out = nv;
    if (nv > c->cap) { glio_set_error("%d points exceed max_points_per_scan %d", nv, c->cap); return GLIO_E_ARG; }
    if (c->ext_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, c->ev_ext_read, 0)); c->ext_read_pending = 0; }
    if (nv > 0) GLIO_HIP_CHECK(hipMemcpyAsync(c->d_scan + (size_t)glio_scan_row(c, slot) * c->cap, f->d_ts, (size_t)nv * 16, hipMemcpyDeviceToDevice, s));
    glio_assoc_scan_uploaded(c, slot, nv);
    GLIO_HIP_CHECK(hipGetLastError());
    c->h_scan_count[slot] = nv;
    return GLIO_OK;
}

int glio_features_last_device_ms(glio_ctx* c, float* ms) {
    if (!c || !ms) return GLIO_E_ARG;
    FeatWork* f = c->features;
    if (!f || !f->have) { glio_set_error("glio_features_extract first"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipEventElapsedTime(ms, f->ev0, f->ev1));
    return GLIO_OK;
}

}  // extern "C"

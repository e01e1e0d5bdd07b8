// cloud_device.h -- the device routines that the point-cloud stages share (localmap_kernels.hip, globalmap_kernels.hip, loop_kernels.hip,
// feature_kernels.hip, keyframe_cloud_kernels.hip, assoc_kernels.hip): transformCloud of one point, the cell key of the voxel tables, the de-skew's ratio
// and slerp, the bounding box of a workgroup, the wavefront and workgroup scan and ballot rank, one pass of the stable radix sort.  Each has ONE definition here: the stages are held to the reference, the oracle or
// each other bit for bit, so a rounding or an ordering is changed in one place or not at all.  The integer routines are exact whatever the order of their
// additions; cloud_transform, cloud_deskew_ratio and cloud_slerp_identity are the only arithmetic.
#pragma once
#include <cfloat>

#include "glio_device.h"

// transformCloud of one point (reference Estimator.cpp:1517-1546): double q * v + t, float store.  Eigen's q * v is v + w * (2 u x v) + u x (2 u x v) with
// the products kept separate (d_qrot_nc); the translation is added last, (v + q0 uv + uuv) + t.  No contraction whatever the including file says.
// cloud_transform_d: the sums before the float store (k_qbin_tile carries them on into a second frame).
__device__ __forceinline__ void cloud_transform_d(const double q[4], const double t[3], const float4 p, double o[3]) {
#pragma clang fp contract(off)
    const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
    double r[3];
    d_qrot_nc(q, v, r);
    o[0] = r[0] + t[0]; o[1] = r[1] + t[1]; o[2] = r[2] + t[2];
}
__device__ __forceinline__ float4 cloud_transform(const double q[4], const double t[3], const float4 p) {
    double o[3];
    cloud_transform_d(q, t, p, o);
    return make_float4((float)o[0], (float)o[1], (float)o[2], p.w);
}

// ---- the cell key of the open-addressing voxel tables (assoc_kernels.hip: the map's and the keyframes' hashes and the query grouping; localmap_kernels.hip:
// the ring's voxel table): 21 bits per axis, biased by 2^20, x in the HIGH bits; the all-ones word is no key (the tables' EMPTY).  globalmap_kernels.hip packs
// x into the LOW bits -- its sort order depends on that -- and keeps its own packing.
__device__ __forceinline__ unsigned long long cloud_cell_key(const int ix, const int iy, const int iz) {
    return ((unsigned long long)(unsigned)(ix + (1 << 20)) << 42) | ((unsigned long long)(unsigned)(iy + (1 << 20)) << 21) |
           (unsigned long long)(unsigned)(iz + (1 << 20));
}
__device__ __forceinline__ void cloud_cell_of_key(const unsigned long long key, int& ix, int& iy, int& iz) {
    ix = (int)((key >> 42) & 0x1fffffu) - (1 << 20); iy = (int)((key >> 21) & 0x1fffffu) - (1 << 20); iz = (int)(key & 0x1fffffu) - (1 << 20);
}
// a key as the two ints (lo, hi) a 16 B table entry or unit record carries, and back
__device__ __forceinline__ int cloud_key_lo(const unsigned long long key) { return (int)(unsigned)(key & 0xffffffffull); }
__device__ __forceinline__ int cloud_key_hi(const unsigned long long key) { return (int)(unsigned)(key >> 32); }
__device__ __forceinline__ unsigned long long cloud_key_join(const int lo, const int hi) { return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo; }
// the tables' hash of a key (the 64-bit finaliser of MurmurHash3)
__device__ __forceinline__ unsigned cloud_key_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned)k;
}

// ---- the de-skew of one point by its intensity (reference Preprocessing.cpp:176-200, LidarOdometry.cpp:180-201: the same body twice)
// ratio = (intensity - (float)(int)intensity) / 0.1: the difference in FLOAT, the quotient in double, capped at 1 and NOT clamped below (a negative intensity
// truncates toward zero and gives a negative ratio)
__device__ __forceinline__ double cloud_deskew_ratio(const float inten) {
#pragma clang fp contract(off)
    const int line = (int)inten;
    const double dt_i = (double)(inten - (float)line);
    double t = dt_i / 0.1;
    if (t >= 1.0) t = 1.0;
    return t;
}
// Eigen's Quaterniond::Identity().slerp(t, q): the linear branch at |d| >= 1 - DBL_EPSILON, the sign flipped for d < 0; every product rounded before it is
// added (the zero products of the identity's coefficients are written out: they are what the reference's dot() and coeffs() sums hold)
__device__ __forceinline__ void cloud_slerp_identity(const double q[4], const double t, double qs[4]) {
#pragma clang fp contract(off)
    const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
    const double d = 0.0 * qx + 0.0 * qy + 0.0 * qz + 1.0 * qw;               // dot of the identity's and q's coefficients
    const double ad = fabs(d);
    double s0, s1;
    if (ad >= 1.0 - DBL_EPSILON) { s0 = 1.0 - t; s1 = t; }
    else {
        const double th = acos(ad), sth = sin(th);
        s0 = sin((1.0 - t) * th) / sth;
        s1 = sin(t * th) / sth;
    }
    if (d < 0.0) s1 = -s1;
    qs[0] = s0 * 1.0 + s1 * qw; qs[1] = s0 * 0.0 + s1 * qx; qs[2] = s0 * 0.0 + s1 * qy; qs[3] = s0 * 0.0 + s1 * qz;
}

// ---- bounding box of three ints (ordered floats, f2ord, or voxel coordinates): per thread, then per wavefront, then six atomics per workgroup
struct CloudBox {
    int mn[3], mx[3];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = 0x7fffffff; mx[a] = (int)0x80000000; }
    }
    __device__ __forceinline__ void add(const int a, const int v) { mn[a] = min(mn[a], v); mx[a] = max(mx[a], v); }
    __device__ __forceinline__ void add(const int x, const int y, const int z) { add(0, x); add(1, y); add(2, z); }
    __device__ __forceinline__ void wave_reduce() {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { mn[a] = min(mn[a], __shfl_xor(mn[a], off, 64)); mx[a] = max(mx[a], __shfl_xor(mx[a], off, 64)); }
        }
    }
    // the whole workgroup of NW wavefronts calls this once: box6[0..3) takes the minima, box6[3..6) the maxima -- one set of six atomics per workgroup
    // (they all hit the same six words).  s_box: NW * 6 ints of LDS.
    template <int NW> __device__ __forceinline__ void commit(int* s_box, int* box6) {
        wave_reduce();
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { s_box[6 * (threadIdx.x >> 6) + a] = mn[a]; s_box[6 * (threadIdx.x >> 6) + 3 + a] = mx[a]; }
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            int v = s_box[threadIdx.x];
            if (threadIdx.x < 3) { for (int w = 1; w < NW; ++w) v = min(v, s_box[6 * w + threadIdx.x]); atomicMin(box6 + threadIdx.x, v); }
            else { for (int w = 1; w < NW; ++w) v = max(v, s_box[6 * w + threadIdx.x]); atomicMax(box6 + threadIdx.x, v); }
        }
    }
};

// ---- workgroup scan and rank (NW wavefronts, every thread of the workgroup calls; s_w: NW ints of LDS, free again on return)
// inclusive scan inside every aligned group of W lanes of a wavefront (W a power of two; 64 = the whole wavefront)
template <int W = 64> __device__ __forceinline__ int cloud_wave_incl_scan(const int v) {
    const int lane = threadIdx.x & (W - 1);
    int incl = v;
#pragma unroll
    for (int off = 1; off < W; off <<= 1) { const int o = __shfl_up(incl, off, W); if (lane >= off) incl += o; }
    return incl;
}
// the sum of the wavefronts' totals before this thread's wavefront; total = all of them
template <int NW> __device__ __forceinline__ int cloud_wg_before(const int wave_total, const bool writer, int* s_w, int& total) {
    const int w = threadIdx.x >> 6;
    if (writer) s_w[w] = wave_total;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) { const int x = s_w[k]; before += k < w ? x : 0; tot += x; }
    __syncthreads();
    total = tot;
    return before;
}
// exclusive scan of v in thread order; total = the sum over the workgroup
template <int NW> __device__ __forceinline__ int cloud_wg_excl_scan(const int v, int* s_w, int& total) {
    const int incl = cloud_wave_incl_scan(v);
    return cloud_wg_before<NW>(incl, (threadIdx.x & 63) == 63, s_w, total) + incl - v;
}
// exclusive rank of a flag among the workgroup's threads in thread order; total = flags set
template <int NW> __device__ __forceinline__ int cloud_wg_rank(const bool f, int* s_w, int& total) {
    const int lane = threadIdx.x & 63;
    const unsigned long long b = __ballot(f);
    return cloud_wg_before<NW>(__popcll(b), lane == 0, s_w, total) + __popcll(b & ((1ull << lane) - 1ull));
}

// ---- one pass of a stable least-significant-digit radix sort on 8-bit digits: ONE wavefront per tile of TILE (key, value) pairs.  digit(key) is the
// pass's digit of a key, 0..255.  Between the two, the caller scans hist[tile][digit] exclusively over (digit, tile) in that order.
// the tile's 256-bin histogram (LDS atomics) -> hist_row = hist[tile][.]; h: 256 ints of LDS
template <int TILE, class Digit> __device__ __forceinline__ void cloud_radix_hist(const unsigned long long* __restrict__ key, const int n, const int tile, const Digit digit,
                                                                                  int* h, int* __restrict__ hist_row) {
    const int lane = threadIdx.x, t0 = tile * TILE;
    for (int d = lane; d < 256; d += 64) h[d] = 0;
    GLIO_WAVE_LDS_SYNC();
    unsigned long long kk[TILE / 64];
#pragma unroll
    for (int q = 0; q < TILE / 64; ++q) { const int e = t0 + 64 * q + lane; kk[q] = e < n ? key[e] : 0ull; }
#pragma unroll
    for (int q = 0; q < TILE / 64; ++q) if (t0 + 64 * q + lane < n) atomicAdd(&h[digit(kk[q])], 1);
    GLIO_WAVE_LDS_SYNC();
    for (int d = lane; d < 256; d += 64) hist_row[d] = h[d];           // [tile][digit]: coalesced here, in the scan and in the scatter
}
// the tile's pairs to where the scanned hist_row says its run of each digit starts.  The wavefront walks the tile's chunks of 64 in order; inside a chunk
// a pair's rank among the lanes with the same digit comes from eight ballots (one per digit bit): stable, no LDS traffic for the ranking.  base: 256 ints
// of LDS.  (pos < n: the offsets are the scan of this very digit's counts)
template <int TILE, class Digit, class V> __device__ __forceinline__ void cloud_radix_scatter(const unsigned long long* __restrict__ key, const V* __restrict__ val, const int n,
                                                                                              const int tile, const Digit digit, int* base, const int* __restrict__ hist_row,
                                                                                              unsigned long long* __restrict__ okey, V* __restrict__ oval) {
    const int lane = threadIdx.x, t0 = tile * TILE;
    for (int d = lane; d < 256; d += 64) base[d] = hist_row[d];
    GLIO_WAVE_LDS_SYNC();
    // all chunks of the tile are fetched first (TILE / 64 independent loads per lane in flight), then ranked chunk by chunk
    unsigned long long kk[TILE / 64]; V vv[TILE / 64];
#pragma unroll
    for (int q = 0; q < TILE / 64; ++q) {
        const int e = t0 + 64 * q + lane;
        kk[q] = e < n ? key[e] : 0ull;
        vv[q] = e < n ? val[e] : (V)0;
    }
#pragma unroll
    for (int q = 0; q < TILE / 64; ++q) {
        const int e = t0 + 64 * q + lane;
        const bool live = e < n;
        const unsigned long long k = kk[q];
        const int dg = live ? digit(k) : 0;
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((dg >> b) & 1);
            same &= ((dg >> b) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        const int pos = live ? base[dg] + rank : 0;
        GLIO_WAVE_LDS_SYNC();
        if (live && rank == 0) base[dg] += __popcll(same);           // the first lane of every digit group advances its run
        GLIO_WAVE_LDS_SYNC();
        if (live) { okey[pos] = k; oval[pos] = vv[q]; }
    }
}

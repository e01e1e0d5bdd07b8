// keyframe_cloud_kernels.hip -- the hand-over of a keyframe's surf cloud from the front end to the sliding window, on the device.
//
// Replaces LidarOdometry::publishCloudLast's undistortion(surf_features, rel_pose's translation, identity) (reference GLIO/src/LidarOdometry.cpp:180-201,
// :619-627, only with if_to_deskew) and Estimator::downSampleCloud's ds_filter_surf (Estimator.cpp:3628-3630: pcl::VoxelGrid at surfDSRange) together with the
// glio_set_scan that followed them: the unfiltered cloud -- a host buffer, or the surf features where the front end's extraction left them -- is de-skewed,
// voxel-filtered and written into the window's scan row, presorted, without leaving the device.
//
//   k_kfc_deskew        ONE pass over the source (records of any stride: a caller's pcl::PointXYZI records as uploaded, a packed float4 array, the front end's
//                       surf features): the point moved by the slerp of its intensity's fraction (cloud_deskew_ratio, cloud_slerp_identity, cloud_transform:
//                       cloud_device.h) -- or copied, without a motion -- stored into the VoxelGrid's staging slot and added to its bounding box
//   glio_vg_staged_*    the multi-workgroup pcl::VoxelGrid of localmap_kernels.hip (float sums in input order, PCL's output order and overflow rule)
//   glio_assoc_*        the presort of the row, as glio_set_scan does
//
// One host wait per call: the VoxelGrid's count (published by a kernel behind the upload, so it also tells that a host source has been read).  With
// leaf <= 0 the count is n and the only wait is for the upload of a host source.
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "glio_device.h"
#include "cloud_device.h"

#pragma clang fp contract(off)

#define KFC_THREADS 256
#define KFC_PER 4             /* points per thread: a workgroup covers 1024 points */

struct KfCloud {
    int max_in;
    LocalMap* vg;                       // width 1, cap max_in; voxel table for max(max_in, max_points_per_scan) voxels: it can never fill, the count is always exact
    GlioRawStage raw;                   // the raw records of a host source
    hipEvent_t ev_src;                  // resident source: the front end's stream at the time of the call
    hipEvent_t ev_done; hipStream_t last_stream; int busy;      // the end of the last call's launches: a call on the OTHER stream (slot / ahead forms) reuses the buffers behind it
    hipEvent_t ev_read;                 // leaf <= 0, host source: the end of the upload
    int timed, have_ms; hipEvent_t ev_t[4];                      // GLIO_KFCLOUD_TIMING=1: around de-skew + box, VoxelGrid (+ the copy into the row), presort
};

// (KfcMotion, the motion of the sweep: glio_device.h -- the dense store runs the same pass)
__global__ __launch_bounds__(KFC_THREADS) void k_kfc_deskew(const unsigned char* __restrict__ src, const int n, const int stride, const int ioff, const KfcMotion m,
                                                            float4* __restrict__ out, int* __restrict__ box6) {
    __shared__ int s_box[KFC_THREADS / 64 * 6];
    const int base = blockIdx.x * (KFC_THREADS * KFC_PER);
    CloudBox b;
    b.init();
    float4 p[KFC_PER];
    // the source is read once: all of a thread's loads in flight together
#pragma unroll
    for (int k = 0; k < KFC_PER; ++k) {
        const int i = base + k * KFC_THREADS + (int)threadIdx.x;
        if (i < n) {
            const unsigned char* r = src + (size_t)i * stride;
            const float* f = reinterpret_cast<const float*>(r);
            p[k] = make_float4(f[0], f[1], f[2], *reinterpret_cast<const float*>(r + ioff));
        }
    }
#pragma unroll
    for (int k = 0; k < KFC_PER; ++k) {
        const int i = base + k * KFC_THREADS + (int)threadIdx.x;
        if (i >= n) continue;
        float4 g = p[k];
        if (m.on) {
            const double ratio = cloud_deskew_ratio(g.w);
            double qs[4];
            cloud_slerp_identity(m.q, ratio, qs);
            const double ts[3] = {ratio * m.t[0], ratio * m.t[1], ratio * m.t[2]};
            g = cloud_transform(qs, ts, g);
        }
        out[i] = g;
        b.add(f2ord(g.x), f2ord(g.y), f2ord(g.z));
    }
    b.commit<KFC_THREADS / 64>(s_box, box6);          // (every thread of the workgroup arrives: no early return above)
}

void glio_kfcloud_destroy(glio_ctx* c) {
    KfCloud* k = c->kfcloud;
    if (!k) return;
    if (k->busy) hipEventSynchronize(k->ev_done);
    if (k->vg) glio_vg_destroy(k->vg);
    if (k->raw.d) hipFree(k->raw.d);
    if (k->ev_src) hipEventDestroy(k->ev_src);
    if (k->ev_done) hipEventDestroy(k->ev_done);
    if (k->ev_read) hipEventDestroy(k->ev_read);
    for (hipEvent_t e : k->ev_t) if (e) hipEventDestroy(e);
    delete k;
    c->kfcloud = nullptr;
}

bool glio_kfc_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i) if (!(fabs(v[i]) <= DBL_MAX)) return false;
    return true;
}
void glio_kfc_motion(const double* trans, const double* quat, KfcMotion* m) {
    memset(m, 0, sizeof *m);
    m->q[0] = 1.0;
    if (trans) {
        m->on = 1;
        for (int e = 0; e < 3; ++e) m->t[e] = trans[e];
        if (quat) for (int e = 0; e < 4; ++e) m->q[e] = quat[e];
    }
}
void glio_kfc_launch_deskew(hipStream_t s, const unsigned char* src, int n, int stride, int ioff, const KfcMotion& m, float4* out, int* box6) {
    const dim3 grid((n + KFC_THREADS * KFC_PER - 1) / (KFC_THREADS * KFC_PER));
    hipLaunchKernelGGL(k_kfc_deskew, grid, dim3(KFC_THREADS), 0, s, src, n, stride, ioff, m, out, box6);
}

// slot >= 0: into window slot `slot` on the context's stream; slot < 0: ahead, into the row of the current slot 0 on the upload stream.
// fe == null: n records of `stride` bytes in host memory at `host`; else the surf features of `fe`.
static int kfc_run(glio_ctx* c, const int slot, const void* host, glio_ctx* fe, int n, int stride, int ioff, const float leaf, const double* trans, const double* quat,
                   int* n_out) {
    const bool ahead = slot < 0;
    if (ahead && c->W < 2) { glio_set_error("a scan is sent ahead into a window of two keyframes or more"); return GLIO_E_ARG; }
    if (!ahead && slot >= c->W) { glio_set_error("bad slot %d", slot); return GLIO_E_ARG; }
    if (!fe && !glio_point_layout_ok(stride, ioff)) { glio_set_error("bad point layout (stride %d, intensity at %d)", stride, ioff); return GLIO_E_ARG; }
    if (fe && fe->device != c->device) { glio_set_error("the front end is on device %d, the context on %d", fe->device, c->device); return GLIO_E_ARG; }
    if ((trans && !glio_kfc_finite(trans, 3)) || (quat && !glio_kfc_finite(quat, 4))) { glio_set_error("the de-skew motion is not finite"); return GLIO_E_ARG; }
    KfCloud* k = c->kfcloud;
    if (!k) { glio_set_error("glio_scan_filter_config first"); return GLIO_E_STATE; }
    const float4* d_feat = nullptr;
    if (fe) {
        const int rv = glio_features_surf_view(fe, &d_feat, &n);
        if (rv != GLIO_OK) return rv;
        stride = 16; ioff = 12;
    } else if (n < 0 || (n > 0 && !host)) { glio_set_error("bad cloud (n %d)", n); return GLIO_E_ARG; }
    if (n > k->max_in) { glio_set_error("%d input points exceed max_input_points %d", n, k->max_in); return GLIO_E_ARG; }
    if (!(leaf > 0.f) && n > c->cap) { if (n_out) *n_out = n; glio_set_error("%d points exceed max_points_per_scan %d", n, c->cap); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (ahead) { const int rb = glio_ahead_begin(c, &s); if (rb != GLIO_OK) return rb; }
    const size_t row = (size_t)glio_scan_row(c, ahead ? 0 : slot) * c->cap;
    int nv = 0;
    if (n > 0) {
        // the staging, the voxel table and the raw records are one set: a call on the other stream comes behind the last call's launches (on the device)
        if (k->busy && k->last_stream != s) GLIO_HIP_CHECK(hipStreamWaitEvent(s, k->ev_done, 0));
        const unsigned char* src;
        if (fe) {
            // behind the extraction that wrote the features -- for this stream, not for the host
            if (fe->stream != s) { GLIO_HIP_CHECK(hipEventRecord(k->ev_src, fe->stream)); GLIO_HIP_CHECK(hipStreamWaitEvent(s, k->ev_src, 0)); }
            src = reinterpret_cast<const unsigned char*>(d_feat);
        } else {
            const size_t bytes = (size_t)n * stride;
            if (bytes > k->raw.cap) {           // (records wider than pcl::PointXYZI's 32 bytes: grown once)
                if (k->busy) GLIO_HIP_CHECK(hipEventSynchronize(k->ev_done));
                if (k->raw.d) hipFree(k->raw.d);
                k->raw.d = nullptr; k->raw.cap = 0;
                GLIO_HIP_CHECK(hipMalloc(&k->raw.d, (size_t)k->max_in * stride));
                k->raw.cap = (size_t)k->max_in * stride;
            }
            GLIO_HIP_CHECK(hipMemcpyAsync(k->raw.d, host, bytes, hipMemcpyHostToDevice, s));
            src = static_cast<const unsigned char*>(k->raw.d);
        }
        KfcMotion m;
        glio_kfc_motion(trans, quat, &m);
        const bool filter = leaf > 0.f;
        if (filter) { const int rb = glio_vg_staged_begin(k->vg, s, n); if (rb != GLIO_OK) return rb; }
        else if (c->ext_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, c->ev_ext_read, 0)); if (!ahead) c->ext_read_pending = 0; }
        if (k->timed) GLIO_HIP_CHECK(hipEventRecord(k->ev_t[0], s));
        // leaf <= 0: the count is n, the moved points go straight into the row (the box is computed and not used)
        glio_kfc_launch_deskew(s, src, n, stride, ioff, m, filter ? glio_vg_staging(k->vg) : c->d_scan + row, glio_vg_staging_box(k->vg));
        GLIO_HIP_CHECK(hipGetLastError());
        if (k->timed) GLIO_HIP_CHECK(hipEventRecord(k->ev_t[1], s));
        if (fe && fe->stream != s) {            // the front end's next extraction (and its destruction) come behind this read
            if (!fe->ev_feat_read) GLIO_HIP_CHECK(hipEventCreateWithFlags(&fe->ev_feat_read, hipEventDisableTiming));
            GLIO_HIP_CHECK(hipEventRecord(fe->ev_feat_read, s));
            fe->feat_read_pending = 1;
        }
        k->busy = 1; k->last_stream = s;
        if (filter) {
            int pass = 0;
            const int rf = glio_vg_staged_finish(k->vg, s, n, leaf, &nv, &pass);          // (the one host wait)
            if (rf != GLIO_OK) { hipEventRecord(k->ev_done, s); return rf; }
            if (n_out) *n_out = nv;
            if (nv > c->cap) {
                GLIO_HIP_CHECK(hipEventRecord(k->ev_done, s));
                glio_set_error("%d points exceed max_points_per_scan %d", nv, c->cap);
                return GLIO_E_ARG;
            }
            // (a copy of a resident scan on another stream may still be reading the row this call overwrites)
            if (c->ext_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, c->ev_ext_read, 0)); if (!ahead) c->ext_read_pending = 0; }
            GLIO_HIP_CHECK(hipMemcpyAsync(c->d_scan + row, pass ? glio_vg_staging(k->vg) : glio_vg_output(k->vg), (size_t)nv * 16, hipMemcpyDeviceToDevice, s));
        } else {
            nv = n;
            if (!fe) GLIO_HIP_CHECK(hipEventRecord(k->ev_read, s));
        }
        if (k->timed) GLIO_HIP_CHECK(hipEventRecord(k->ev_t[2], s));
    }
    if (n_out) *n_out = nv;
    if (ahead) {
        glio_assoc_presort_row(c, s, row, nv);
        if (n > 0 && k->timed) GLIO_HIP_CHECK(hipEventRecord(k->ev_t[3], s));
        const int rk = glio_ahead_commit(c, nv);
        if (rk != GLIO_OK) return rk;
    } else {
        glio_assoc_scan_uploaded(c, slot, nv);
        GLIO_HIP_CHECK(hipGetLastError());
        if (n > 0 && k->timed) GLIO_HIP_CHECK(hipEventRecord(k->ev_t[3], s));
        c->h_scan_count[slot] = nv;
    }
    if (n > 0) {
        GLIO_HIP_CHECK(hipEventRecord(k->ev_done, s));
        if (k->timed) k->have_ms = 1;
        if (!(leaf > 0.f) && !fe) GLIO_HIP_CHECK(hipEventSynchronize(k->ev_read));      // the caller's buffer has been read
    }
    return GLIO_OK;
}

extern "C" {

int glio_scan_filter_config(glio_ctx* c, int max_input_points) {
    if (!c || max_input_points < 1 || max_input_points > GLIO_FEAT_MAX_RAW_POINTS) {
        glio_set_error("max_input_points %d outside [1, %d]", max_input_points, GLIO_FEAT_MAX_RAW_POINTS);
        return GLIO_E_ARG;
    }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    GLIO_HIP_CHECK(hipStreamSynchronize(c->stream));
    glio_kfcloud_destroy(c);
    KfCloud* k = new KfCloud();
    memset(k, 0, sizeof *k);
    k->max_in = max_input_points;
    c->kfcloud = k;
    const int max_vox = max_input_points > c->cap ? max_input_points : c->cap;
    int rc = glio_vg_create(1, max_input_points, 1.0f, max_vox, c->stream, &k->vg);
    if (rc != GLIO_OK) { glio_kfcloud_destroy(c); return rc; }
    k->timed = glio_switch_at_create<GLIO_SW_KFCLOUD_TIMING>();
    hipError_t he = hipMalloc(&k->raw.d, (size_t)max_input_points * 32);
    if (he == hipSuccess) { k->raw.cap = (size_t)max_input_points * 32; he = hipEventCreateWithFlags(&k->ev_src, hipEventDisableTiming); }
    if (he == hipSuccess) he = hipEventCreateWithFlags(&k->ev_done, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&k->ev_read, hipEventDisableTiming);
    for (int i = 0; i < 4 && k->timed && he == hipSuccess; ++i) he = hipEventCreate(&k->ev_t[i]);
    if (he != hipSuccess) { glio_set_error("glio_scan_filter_config: %s", hipGetErrorString(he)); glio_kfcloud_destroy(c); return GLIO_E_HIP; }
    return GLIO_OK;
}

int glio_set_scan_filtered_strided(glio_ctx* c, int slot, const void* points, int n, int stride_bytes, int intensity_offset, float leaf, const double* deskew_trans,
                                   const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_set_scan_filtered");
    if (!c || slot < 0) { glio_set_error("bad slot"); return GLIO_E_ARG; }
    return kfc_run(c, slot, points, nullptr, n, stride_bytes, intensity_offset, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_set_scan_filtered(glio_ctx* c, int slot, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    return glio_set_scan_filtered_strided(c, slot, xyzi, n, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_set_scan_filtered_ahead_strided(glio_ctx* c, const void* points, int n, int stride_bytes, int intensity_offset, float leaf, const double* deskew_trans,
                                         const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_set_scan_filtered_ahead");
    if (!c) { glio_set_error("null context"); return GLIO_E_ARG; }
    return kfc_run(c, -1, points, nullptr, n, stride_bytes, intensity_offset, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_set_scan_filtered_ahead(glio_ctx* c, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    return glio_set_scan_filtered_ahead_strided(c, xyzi, n, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_set_scan_from_features(glio_ctx* c, int slot, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_set_scan_from_features");
    if (!c || !frontend || slot < 0) { glio_set_error("bad slot / null context"); return GLIO_E_ARG; }
    return kfc_run(c, slot, nullptr, frontend, 0, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_set_scan_from_features_ahead(glio_ctx* c, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_set_scan_from_features_ahead");
    if (!c || !frontend) { glio_set_error("null context"); return GLIO_E_ARG; }
    return kfc_run(c, -1, nullptr, frontend, 0, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}

int glio_get_scan(glio_ctx* c, int slot, float* out_xyzi, int capacity, int* n) {
    if (!c || slot < 0 || slot >= c->W) { glio_set_error("bad slot"); return GLIO_E_ARG; }
    const int ns = c->h_scan_count[slot];
    if (n) *n = ns;
    if (!out_xyzi) return GLIO_OK;
    if (ns > capacity) { glio_set_error("capacity %d < count %d", capacity, ns); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    if (ns > 0) GLIO_HIP_CHECK(hipMemcpyAsync(out_xyzi, c->d_scan + (size_t)glio_scan_row(c, slot) * c->cap, (size_t)ns * 16, hipMemcpyDeviceToHost, c->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return GLIO_OK;
}

int glio_scan_filter_last_device_ms(glio_ctx* c, float ms[3]) {
    if (!c || !ms) return GLIO_E_ARG;
    KfCloud* k = c->kfcloud;
    if (!k || !k->timed || !k->have_ms) { glio_set_error("no timed call (GLIO_KFCLOUD_TIMING=1 at glio_scan_filter_config, then a non-empty cloud)"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(c->device));
    GLIO_HIP_CHECK(hipEventSynchronize(k->ev_t[3]));
    for (int i = 0; i < 3; ++i) GLIO_HIP_CHECK(hipEventElapsedTime(ms + i, k->ev_t[i], k->ev_t[i + 1]));
    return GLIO_OK;
}

}  // extern "C"

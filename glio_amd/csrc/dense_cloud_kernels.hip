// dense_cloud_kernels.hip -- the store of full_clouds_ds on the device (glio_dense_*, include/glio_dense.h): per keyframe the FULL cloud, de-skewed and
// voxel-filtered as Estimator::downSampleCloud's fullDS would leave it (reference GLIO/src/LidarOdometry.cpp:626, Estimator.cpp:3623-3626), kept resident for the
// global map (globalmap_kernels.hip reads the store through the view it reads a batch association through).
//
//   k_kfc_deskew        the keyframe cloud's pass (keyframe_cloud_kernels.hip, glio_kfc_launch_deskew): undistortion of one point, stored into the VoxelGrid's
//                       staging slot and added to its bounding box
//   glio_vg_staged_*    the multi-workgroup pcl::VoxelGrid of localmap_kernels.hip with the wavefront-per-long-list emit (glio_vg_set_wave_emit): a full cloud
//                       has voxels of hundreds of points next to the sensor
//   k_dn_world          pub_full_cloud_map (LidarOdometry.cpp:645-658): cloud_transform of the staged, unfiltered cloud
//
// Everything runs on the store's own stream.  One host wait per call: the VoxelGrid's count (it also tells that a host source has been read).
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "glio_device.h"
#include "cloud_device.h"
#include "../../include/glio_dense.h"

#pragma clang fp contract(off)

struct glio_dense {
    int device, K, cap, max_in;
    hipStream_t stream;
    float4* d_store;                    // [K][cap]
    int* h_n;                           // [K]
    LocalMap* vg;                       // width 1, cap max_in, a voxel table for max_in voxels: it can never fill
    GlioRawStage raw;                   // the raw records of a host source
    float4* d_world;                    // [max_in] glio_dense_world_cloud's output (allocated at its first call)
    int staged_n;                       // points of the last call's de-skewed cloud in the VoxelGrid's staging slot (-1: none yet)
    hipEvent_t ev_src;                  // resident source: the front end's stream at the time of the call
    hipEvent_t ev_read;                 // leaf <= 0, host source: the end of the upload
    hipEvent_t ev_ext_read; int ext_read_pending;      // a global map's stream is still READING the store: the next write to a frame comes behind this event
    int timed, have_ms; hipEvent_t ev_t[4];            // GLIO_DENSE_TIMING=1: around de-skew + box, VoxelGrid, the copy into the store
};

__global__ void k_dn_world(const float4* __restrict__ in, const int n, const double q0, const double q1, const double q2, const double q3, const double t0,
                           const double t1, const double t2, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double q[4] = {q0, q1, q2, q3}, t[3] = {t0, t1, t2};
    out[i] = cloud_transform(q, t, in[i]);
}

int glio_dense_view(glio_dense* d, GlioBassocView* out) {
    if (!d || !out) return GLIO_E_ARG;
    out->device = d->device; out->K = d->K; out->cap = d->cap; out->d_local = d->d_store; out->h_n = d->h_n; out->stream = d->stream;
    return GLIO_OK;
}
int glio_dense_external_read(glio_dense* d, hipStream_t reader) {
    if (d->ext_read_pending) GLIO_HIP_CHECK(hipStreamWaitEvent(reader, d->ev_ext_read, 0));       // (another object's read: the new record covers it)
    GLIO_HIP_CHECK(hipEventRecord(d->ev_ext_read, reader));
    d->ext_read_pending = 1;
    return GLIO_OK;
}

// fe == null: n records of `stride` bytes in host memory at `host`; else the cut cloud of `fe`
static int dn_run(glio_dense* d, const int k, const void* host, glio_ctx* fe, int n, int stride, int ioff, const float leaf, const double* trans, const double* quat,
                  int* n_out) {
    if (k < 0 || k >= d->K) { glio_set_error("frame %d outside [0, %d)", k, d->K); return GLIO_E_ARG; }
    if (!fe && !glio_point_layout_ok(stride, ioff)) { glio_set_error("bad point layout (stride %d, intensity at %d)", stride, ioff); return GLIO_E_ARG; }
    if (fe && fe->device != d->device) { glio_set_error("the front end is on device %d, the dense store on %d", fe->device, d->device); return GLIO_E_ARG; }
    if ((trans && !glio_kfc_finite(trans, 3)) || (quat && !glio_kfc_finite(quat, 4))) { glio_set_error("the de-skew motion is not finite"); return GLIO_E_ARG; }
    const float4* d_cut = nullptr;
    if (fe) {
        const int rv = glio_features_cut_view(fe, &d_cut, &n);
        if (rv != GLIO_OK) return rv;
        stride = 16; ioff = 12;
    } else if (n < 0 || (n > 0 && !host)) { glio_set_error("bad cloud (n %d)", n); return GLIO_E_ARG; }
    if (n > d->max_in) { glio_set_error("%d input points exceed max_input_points %d", n, d->max_in); return GLIO_E_ARG; }
    const bool filter = leaf > 0.f;
    if (!filter && n > d->cap) { if (n_out) *n_out = n; glio_set_error("%d points exceed max_points_per_frame %d", n, d->cap); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(d->device));
    hipStream_t s = d->stream;
    int nv = 0;
    if (n > 0) {
        const unsigned char* src;
        if (fe) {
            // behind the extraction that wrote the cut cloud -- for this stream, not for the host
            GLIO_HIP_CHECK(hipEventRecord(d->ev_src, fe->stream));
            GLIO_HIP_CHECK(hipStreamWaitEvent(s, d->ev_src, 0));
            src = reinterpret_cast<const unsigned char*>(d_cut);
        } else {
            const size_t bytes = (size_t)n * stride;
            if (bytes > d->raw.cap) {           // (records wider than pcl::PointXYZI's 32 bytes: grown once)
                GLIO_HIP_CHECK(hipStreamSynchronize(s));
                if (d->raw.d) hipFree(d->raw.d);
                d->raw.d = nullptr; d->raw.cap = 0;
                GLIO_HIP_CHECK(hipMalloc(&d->raw.d, (size_t)d->max_in * stride));
                d->raw.cap = (size_t)d->max_in * stride;
            }
            GLIO_HIP_CHECK(hipMemcpyAsync(d->raw.d, host, bytes, hipMemcpyHostToDevice, s));
            src = static_cast<const unsigned char*>(d->raw.d);
        }
        KfcMotion m;
        glio_kfc_motion(trans, quat, &m);
        if (filter) { const int rb = glio_vg_staged_begin(d->vg, s, n); if (rb != GLIO_OK) return rb; }
        if (d->timed) GLIO_HIP_CHECK(hipEventRecord(d->ev_t[0], s));
        // (leaf <= 0: the staged cloud is the frame; the box is computed and not used)
        glio_kfc_launch_deskew(s, src, n, stride, ioff, m, glio_vg_staging(d->vg), glio_vg_staging_box(d->vg));
        GLIO_HIP_CHECK(hipGetLastError());
        d->staged_n = n;
        if (d->timed) GLIO_HIP_CHECK(hipEventRecord(d->ev_t[1], s));
        // the front end's next extraction (and its destruction) come behind this read
        if (fe) { const int re = glio_features_cut_external_read(fe, s); if (re != GLIO_OK) return re; }
        const float4* from = glio_vg_staging(d->vg);
        if (filter) {
            int pass = 0;
            const int rf = glio_vg_staged_finish(d->vg, s, n, leaf, &nv, &pass);          // (the one host wait)
            if (rf != GLIO_OK) return rf;
            if (n_out) *n_out = nv;
            if (nv > d->cap) { glio_set_error("%d points exceed max_points_per_frame %d", nv, d->cap); return GLIO_E_ARG; }
            if (!pass) from = glio_vg_output(d->vg);
        } else {
            nv = n;
            if (!fe) GLIO_HIP_CHECK(hipEventRecord(d->ev_read, s));
        }
        if (d->timed) GLIO_HIP_CHECK(hipEventRecord(d->ev_t[2], s));
        // (a global map on another stream may still be reading the frame this call overwrites)
        if (d->ext_read_pending) { GLIO_HIP_CHECK(hipStreamWaitEvent(s, d->ev_ext_read, 0)); d->ext_read_pending = 0; }
        GLIO_HIP_CHECK(hipMemcpyAsync(d->d_store + (size_t)k * d->cap, from, (size_t)nv * 16, hipMemcpyDeviceToDevice, s));
        if (d->timed) { GLIO_HIP_CHECK(hipEventRecord(d->ev_t[3], s)); d->have_ms = 1; }
        if (!filter && !fe) GLIO_HIP_CHECK(hipEventSynchronize(d->ev_read));      // the caller's buffer has been read
    } else d->staged_n = 0;
    d->h_n[k] = nv;
    if (n_out) *n_out = nv;
    return GLIO_OK;
}

extern "C" {

void glio_dense_destroy(glio_dense* d) {
    if (!d) return;
    hipSetDevice(d->device);
    if (d->stream) hipStreamSynchronize(d->stream);
    if (d->ev_ext_read) { if (d->ext_read_pending) hipEventSynchronize(d->ev_ext_read); hipEventDestroy(d->ev_ext_read); }
    if (d->vg) glio_vg_destroy(d->vg);
    void* p[] = {d->d_store, d->raw.d, d->d_world};
    for (void* q : p) if (q) hipFree(q);
    if (d->ev_src) hipEventDestroy(d->ev_src);
    if (d->ev_read) hipEventDestroy(d->ev_read);
    for (hipEvent_t e : d->ev_t) if (e) hipEventDestroy(e);
    if (d->stream) hipStreamDestroy(d->stream);
    delete[] d->h_n;
    delete d;
}

static int dn_create_body(glio_dense* d) {
    GLIO_HIP_CHECK(hipSetDevice(d->device));
    GLIO_HIP_CHECK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    GLIO_HIP_CHECK(hipMalloc((void**)&d->d_store, (size_t)d->K * d->cap * 16));
    GLIO_HIP_CHECK(hipMalloc(&d->raw.d, (size_t)d->max_in * 32));
    d->raw.cap = (size_t)d->max_in * 32;
    { const int rv = glio_vg_create(1, d->max_in, 1.0f, d->max_in, d->stream, &d->vg); if (rv != GLIO_OK) return rv; }
    glio_vg_set_wave_emit(d->vg, 1);
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&d->ev_src, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&d->ev_read, hipEventDisableTiming));
    GLIO_HIP_CHECK(hipEventCreateWithFlags(&d->ev_ext_read, hipEventDisableTiming));
    d->timed = glio_switch_at_create<GLIO_SW_DENSE_TIMING>();
    for (int i = 0; i < 4 && d->timed; ++i) GLIO_HIP_CHECK(hipEventCreate(&d->ev_t[i]));
    return GLIO_OK;
}
int glio_dense_create(int device, int K, int max_points_per_frame, int max_input_points, glio_dense** out) {
    if (!out || K < 1 || max_points_per_frame < 1 || max_input_points < 1 || max_input_points > GLIO_FEAT_MAX_RAW_POINTS) {
        glio_set_error("bad dense store (K %d, max_points_per_frame %d, max_input_points %d outside [1, %d])", K, max_points_per_frame, max_input_points, GLIO_FEAT_MAX_RAW_POINTS);
        return GLIO_E_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { glio_set_error("no HIP device %d", device); return GLIO_E_HIP; }
    glio_dense* d = new glio_dense();
    memset(d, 0, sizeof *d);
    d->device = device; d->K = K; d->cap = max_points_per_frame; d->max_in = max_input_points; d->staged_n = -1;
    d->h_n = new int[K]();
    const int rc = dn_create_body(d);
    if (rc != GLIO_OK) { glio_dense_destroy(d); return rc; }
    *out = d;
    return GLIO_OK;
}

int glio_dense_set_frame_strided(glio_dense* d, int k, const void* points, int n, int stride_bytes, int intensity_offset, float leaf, const double* deskew_trans,
                                 const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_dense_set_frame");
    if (!d) { glio_set_error("null dense store"); return GLIO_E_ARG; }
    return dn_run(d, k, points, nullptr, n, stride_bytes, intensity_offset, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_dense_set_frame(glio_dense* d, int k, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    return glio_dense_set_frame_strided(d, k, xyzi, n, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}
int glio_dense_set_frame_from_features(glio_dense* d, int k, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out) {
    GLIO_TRACE("glio_dense_set_frame_from_features");
    if (!d || !frontend) { glio_set_error("null dense store / front end"); return GLIO_E_ARG; }
    return dn_run(d, k, nullptr, frontend, 0, 16, 12, leaf, deskew_trans, deskew_quat, n_out);
}

int glio_dense_frame_count(glio_dense* d, int k, int* n) {
    if (!d || !n || k < 0 || k >= d->K) { glio_set_error("bad frame"); return GLIO_E_ARG; }
    *n = d->h_n[k];
    return GLIO_OK;
}
int glio_dense_read_frame(glio_dense* d, int k, float* out_xyzi, int capacity, int* n) {
    if (!d || k < 0 || k >= d->K) { glio_set_error("bad frame"); return GLIO_E_ARG; }
    const int nk = d->h_n[k];
    if (n) *n = nk;
    if (!out_xyzi) return GLIO_OK;
    if (nk > capacity) { glio_set_error("capacity %d < count %d", capacity, nk); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(d->device));
    if (nk > 0) GLIO_HIP_CHECK(hipMemcpyAsync(out_xyzi, d->d_store + (size_t)k * d->cap, (size_t)nk * 16, hipMemcpyDeviceToHost, d->stream));
    GLIO_HIP_CHECK(hipStreamSynchronize(d->stream));
    return GLIO_OK;
}

int glio_dense_last_device_ms(glio_dense* d, float ms[3]) {
    if (!d || !ms) return GLIO_E_ARG;
    if (!d->timed || !d->have_ms) { glio_set_error("no timed call (GLIO_DENSE_TIMING=1 at glio_dense_create, then a non-empty cloud)"); return GLIO_E_STATE; }
    GLIO_HIP_CHECK(hipSetDevice(d->device));
    GLIO_HIP_CHECK(hipEventSynchronize(d->ev_t[3]));
    for (int i = 0; i < 3; ++i) GLIO_HIP_CHECK(hipEventElapsedTime(ms + i, d->ev_t[i], d->ev_t[i + 1]));
    return GLIO_OK;
}

int glio_dense_world_cloud(glio_dense* d, const double* pose_qt, float* out_xyzi, int capacity, int* n) {
    if (!d || !pose_qt) { glio_set_error("null dense store / pose"); return GLIO_E_ARG; }
    if (d->staged_n < 0) { glio_set_error("glio_dense_set_frame first"); return GLIO_E_STATE; }
    if (!glio_kfc_finite(pose_qt, 7)) { glio_set_error("the pose is not finite"); return GLIO_E_ARG; }
    const int ns = d->staged_n;
    if (n) *n = ns;
    if (!out_xyzi) return GLIO_OK;
    if (ns > capacity) { glio_set_error("capacity %d < count %d", capacity, ns); return GLIO_E_ARG; }
    GLIO_HIP_CHECK(hipSetDevice(d->device));
    if (!d->d_world) GLIO_HIP_CHECK(hipMalloc((void**)&d->d_world, (size_t)d->max_in * 16));
    if (ns > 0) {
        hipLaunchKernelGGL(k_dn_world, dim3((ns + 255) / 256), dim3(256), 0, d->stream, glio_vg_staging(d->vg), ns, pose_qt[3], pose_qt[4], pose_qt[5], pose_qt[6],
                           pose_qt[0], pose_qt[1], pose_qt[2], d->d_world);
        GLIO_HIP_CHECK(hipGetLastError());
        GLIO_HIP_CHECK(hipMemcpyAsync(out_xyzi, d->d_world, (size_t)ns * 16, hipMemcpyDeviceToHost, d->stream));
    }
    GLIO_HIP_CHECK(hipStreamSynchronize(d->stream));
    return GLIO_OK;
}

}  // extern "C"

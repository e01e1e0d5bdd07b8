// glio_map_backend.hpp -- the global map of Estimator (GLIO/src/Estimator.cpp:5315-5350, mapVisualizationThread's save_pcd part; :5275-5313, publishCompleteMap)
// on the C-ABI of include/glio_hip.h.  C-ABI only, C++14, no HIP headers.
//
//   glio::GlobalMap          the device object (glio_gmap_*): the listed resident keyframe clouds of a glio_bassoc moved to the world at their final poses, the
//                            concatenation through one pcl::VoxelGrid (leaf 0.2, :856); added to call by call, bit for bit what one call would give
//   glio::globalMapFrames    :5339   which keyframes enter the map
//   glio::DenseClouds        the store of full_clouds_ds (glio_dense_*, include/glio_dense.h): per keyframe the FULL cloud, de-skewed and filtered on the device
//                            (LidarOdometry.cpp:626, Estimator.cpp:3623-3626); a GlobalMap constructed on it is publishCompleteMap -- the dense map
// The poses are glio::loopFramePoses (glio_loop_backend.hpp, :5287-5288).  Writing the .pcd stays with the caller.
// The Python twin is glio_amd/mapping.py.
#ifndef GLIO_MAP_BACKEND_HPP_
#define GLIO_MAP_BACKEND_HPP_
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_hip.h"
#include "glio_dense.h"
#include "glio_static.h"

namespace glio {

// Estimator.cpp:5339: for (i = 0; i < n; i += mapping_interval)
inline std::vector<int32_t> globalMapFrames(int n_keyframes, int mapping_interval) {
    std::vector<int32_t> out;
    if (mapping_interval < 1) throw std::invalid_argument("globalMapFrames: mapping_interval < 1");
    for (int i = 0; i < n_keyframes; i += mapping_interval) out.push_back(i);
    return out;
}

// One glio_dense: K frames of up to max_points_per_frame points, each pcl::VoxelGrid(leaf) of undistortion(cloud, trans, quat), on a stream of its own.
class DenseClouds {
public:
    DenseClouds(int K, int max_points_per_frame, int max_input_points, int device = 0) {
        check(glio_dense_create(device, K, max_points_per_frame, max_input_points, &h_), "glio_dense_create");
    }
    ~DenseClouds() { glio_dense_destroy(h_); }
    DenseClouds(const DenseClouds&) = delete;
    DenseClouds& operator=(const DenseClouds&) = delete;
    glio_dense* handle() const { return h_; }
    // records of stride_bytes with the intensity float at intensity_offset (a packed [n][4] array: 16, 12); trans / quat null: no de-skew / the identity.
    // Returns the frame's point count; throws on a refusal, which leaves the frame as it was.
    int setFrame(int k, const void* points, int n, int stride_bytes, int intensity_offset, float leaf, const double* trans = nullptr, const double* quat = nullptr) {
        int out = 0;
        check(glio_dense_set_frame_strided(h_, k, points, n, stride_bytes, intensity_offset, leaf, trans, quat, &out), "glio_dense_set_frame_strided");
        return out;
    }
    // the CUT cloud of `frontend`'s last glio_features_extract* (ScanToMapOdometry::ctx() after runRaw), read where it lies; the reference's call has
    // trans = rel_pose's translation (&rel_pose[4]) and no quat
    int setFrameFromFeatures(int k, glio_ctx* frontend, float leaf, const double* trans = nullptr, const double* quat = nullptr) {
        int out = 0;
        check(glio_dense_set_frame_from_features(h_, k, frontend, leaf, trans, quat, &out), "glio_dense_set_frame_from_features");
        return out;
    }
    int frameCount(int k) { int n = 0; check(glio_dense_frame_count(h_, k, &n), "glio_dense_frame_count"); return n; }
    std::vector<float> readFrame(int k) {
        const int n = frameCount(k);
        std::vector<float> out((size_t)n * 4);
        int got = 0;
        check(glio_dense_read_frame(h_, k, out.data(), n, &got), "glio_dense_read_frame");
        return out;
    }
    // pub_full_cloud_map: the last setFrame*'s de-skewed, unfiltered cloud moved to pose = t[3], q[4] (w first)
    std::vector<float> worldCloud(const double pose[7]) {
        int n = 0;
        check(glio_dense_world_cloud(h_, pose, nullptr, 0, &n), "glio_dense_world_cloud");
        std::vector<float> out((size_t)n * 4);
        check(glio_dense_world_cloud(h_, pose, out.data(), n, &n), "glio_dense_world_cloud");
        return out;
    }
    // de-skew + box, VoxelGrid, copy into the store (GLIO_DENSE_TIMING=1 at construction)
    void lastDeviceMs(float ms[3]) { check(glio_dense_last_device_ms(h_, ms), "glio_dense_last_device_ms"); }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_dense* h_ = nullptr;
};

class GlobalMap {
public:
    // `assoc` owns the resident keyframe clouds and must outlive this object
    explicit GlobalMap(glio_bassoc* assoc, const glio_gmap_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_gmap_opts_default(&o_);
        check(glio_gmap_create(assoc, &o_, &h_), "glio_gmap_create");
    }
    // ... or `dense`, whose frames add() then reads: the dense map
    explicit GlobalMap(DenseClouds& dense, const glio_gmap_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_gmap_opts_default(&o_);
        check(glio_gmap_create_on_dense(dense.handle(), &o_, &h_), "glio_gmap_create_on_dense");
    }
    // ... or a static store (glio::StaticClouds::handle(), glio_static_backend.hpp): its frames without the points that were seen through -- the static map
    explicit GlobalMap(glio_static* st, const glio_gmap_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_gmap_opts_default(&o_);
        check(glio_gmap_create_on_static(st, &o_, &h_), "glio_gmap_create_on_static");
    }
    ~GlobalMap() { glio_gmap_destroy(h_); }
    GlobalMap(const GlobalMap&) = delete;
    GlobalMap& operator=(const GlobalMap&) = delete;
    glio_gmap* handle() const { return h_; }
    const glio_gmap_opts& opts() const { return o_; }
    // frames in list order (repeats allowed), poses [n][7] = t, q (loopFramePoses); behind everything added since the last clear.  Throws on a refusal, which
    // leaves the map exactly as it was.
    glio_gmap_info add(const std::vector<int32_t>& frames, const std::vector<double>& poses) {
        glio_gmap_info info;
        check(glio_gmap_add_frames(h_, (int)frames.size(), frames.data(), poses.data(), &info), "glio_gmap_add_frames");
        return info;
    }
    void clear() { check(glio_gmap_clear(h_), "glio_gmap_clear"); }
    int size() { int n = 0; check(glio_gmap_size(h_, &n), "glio_gmap_size"); return n; }
    // voxels [first, first + n) as xyzi
    std::vector<float> read(int first, int n) {
        std::vector<float> out((size_t)(n > 0 ? n : 0) * 4);
        check(glio_gmap_read(h_, first, n, out.data()), "glio_gmap_read");
        return out;
    }
    std::vector<float> read() { return read(0, size()); }
    // the map on the device ([size()] x 4 floats), valid until the next successful add
    const void* pointsDev(int* n = nullptr) { const void* p = nullptr; check(glio_gmap_points_dev(h_, &p, n), "glio_gmap_points_dev"); return p; }
    float lastDeviceMs() { float ms = 0; check(glio_gmap_last_device_ms(h_, &ms), "glio_gmap_last_device_ms"); return ms; }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_gmap_opts o_;
    glio_gmap* h_ = nullptr;
};

}  // namespace glio
#endif  // GLIO_MAP_BACKEND_HPP_

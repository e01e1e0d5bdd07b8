// glio_static_backend.hpp -- the static map on the C-ABI of include/glio_static.h: every point of every resident frame tested against the range images of
// other frames, the points that were seen through dropped, the rest kept per frame for glio::GlobalMap.  The library's own addition (the reference maps
// full_clouds_ds as it comes).  C-ABI only, C++14, no HIP headers.
//
//   glio::StaticClouds      the device object (glio_static_*) on a glio_bassoc or a glio::DenseClouds
//   glio::staticViews       the usual choice of views: the nearest frames in list order on both sides that are at least min_baseline away
//   glio::GlobalMap(st.handle())   the map of the static store (glio_map_backend.hpp)
// The Python twin is glio_amd/static_map.py: the same scalar arithmetic in the same order.
#ifndef GLIO_STATIC_BACKEND_HPP_
#define GLIO_STATIC_BACKEND_HPP_
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_map_backend.hpp"
#include "glio_static.h"

namespace glio {

// poses [n][7] (t, q): for frame f up to half_window earlier frames (nearest first), then up to half_window later ones (nearest first), each with a position at
// least min_baseline from f's (squared distances compared in double; a stationary vehicle gives no parallax).  -> view_offsets [n + 1], views
inline void staticViews(const std::vector<double>& poses, int half_window, double min_baseline, std::vector<int32_t>* view_offsets, std::vector<int32_t>* views) {
    const int n = (int)(poses.size() / 7);
    const double b2 = min_baseline * min_baseline;
    view_offsets->assign(1, 0);
    views->clear();
    for (int f = 0; f < n; ++f) {
        for (int step = -1; step <= 1; step += 2) {
            int taken = 0;
            for (int j = f + step; j >= 0 && j < n && taken < half_window; j += step) {
                const double dx = poses[7 * j] - poses[7 * f], dy = poses[7 * j + 1] - poses[7 * f + 1], dz = poses[7 * j + 2] - poses[7 * f + 2];
                if ((dx * dx + dy * dy) + dz * dz >= b2) { views->push_back(j); ++taken; }
            }
        }
        view_offsets->push_back((int32_t)views->size());
    }
}

class StaticClouds {
public:
    // `assoc` / `dense` owns the resident clouds and must outlive this object.  Static frame k is the owner's frame k without its dynamic points.
    explicit StaticClouds(glio_bassoc* assoc, const glio_static_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_static_opts_default(&o_);
        check(glio_static_create(assoc, &o_, &h_), "glio_static_create");
    }
    explicit StaticClouds(DenseClouds& dense, const glio_static_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_static_opts_default(&o_);
        check(glio_static_create_on_dense(dense.handle(), &o_, &h_), "glio_static_create_on_dense");
    }
    ~StaticClouds() { glio_static_destroy(h_); }
    StaticClouds(const StaticClouds&) = delete;
    StaticClouds& operator=(const StaticClouds&) = delete;
    glio_static* handle() const { return h_; }
    const glio_static_opts& opts() const { return o_; }
    int rows() const { return o_.rows; }
    int cols() const { return 4 * o_.cols_per_quadrant; }
    // rules 1 - 6 of glio_static.h; poses [n][7] = t, q.  Throws on a refusal, which leaves the store, the counts and the votes exactly as they were.
    glio_static_info classify(const std::vector<int32_t>& frames, const std::vector<double>& poses, const std::vector<int32_t>& view_offsets,
                              const std::vector<int32_t>& views) {
        if (poses.size() != 7 * frames.size() || view_offsets.size() != frames.size() + 1) throw std::invalid_argument("StaticClouds::classify: list lengths differ");
        glio_static_info info;
        check(glio_static_classify(h_, (int)frames.size(), frames.data(), poses.data(), view_offsets.data(), views.empty() ? nullptr : views.data(), &info),
              "glio_static_classify");
        return info;
    }
    int frameCount(int k) { int n = 0; check(glio_static_frame_count(h_, k, &n), "glio_static_frame_count"); return n; }
    // static frame k as xyzi
    std::vector<float> readFrame(int k) {
        const int n = frameCount(k);
        std::vector<float> out((size_t)n * 4);
        int got = 0;
        check(glio_static_read_frame(h_, k, out.data(), n, &got), "glio_static_read_frame");
        return out;
    }
    void readVotes(int k, std::vector<uint8_t>* through, std::vector<uint8_t>* tested) {
        int n = 0;
        check(glio_static_read_votes(h_, k, nullptr, nullptr, 0, &n), "glio_static_read_votes");
        through->assign((size_t)n, 0); tested->assign((size_t)n, 0);
        check(glio_static_read_votes(h_, k, through->data(), tested->data(), n, &n), "glio_static_read_votes");
    }
    // the last call's images of its call-local frame `view`: [rows][cols] each
    void readImage(int view, std::vector<float>* raw, std::vector<float>* floor) {
        raw->assign((size_t)rows() * cols(), 0.f); floor->assign((size_t)rows() * cols(), 0.f);
        check(glio_static_read_image(h_, view, raw->data(), floor->data()), "glio_static_read_image");
    }
    void lastDeviceMs(float ms[4]) { check(glio_static_last_device_ms(h_, ms), "glio_static_last_device_ms"); }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_static_opts o_;
    glio_static* h_ = nullptr;
};

}  // namespace glio
#endif  // GLIO_STATIC_BACKEND_HPP_

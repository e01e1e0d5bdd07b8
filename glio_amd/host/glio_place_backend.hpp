// glio_place_backend.hpp -- place recognition on the C-ABI of include/glio_place.h: a Scan Context descriptor of every resident keyframe cloud and the exact
// scan-context distance of a query place to every stored one.  The library's own addition (the reference proposes loops by position only,
// Estimator.cpp:5113-5123).  C-ABI only, C++14, no HIP headers.
//
//   glio::PlaceRecognition             the device object (glio_place_*) on a glio_bassoc or a glio_dense
//   glio::levelingQuaternion           a keyframe's attitude with its yaw removed: the level_q of addFrames
//   glio::detectCandidateByAppearance  the appearance rule beside glio::detectLoopCandidate: closest keyframe, heading, distance
//   glio::placeInitialGuess            the pose the source submap is built at, so that the ICP starts from the heading the match found
// The Python twin is glio_amd/place.py: the same scalar arithmetic in the same order.
#ifndef GLIO_PLACE_BACKEND_HPP_
#define GLIO_PLACE_BACKEND_HPP_
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_place.h"

namespace glio {

class PlaceRecognition {
public:
    // `assoc` / `dense` owns the resident clouds and must outlive this object.  The caller keeps keyframe i at place i.
    explicit PlaceRecognition(glio_bassoc* assoc, const glio_place_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_place_opts_default(&o_);
        check(glio_place_create(assoc, &o_, &h_), "glio_place_create");
    }
    explicit PlaceRecognition(glio_dense* dense, const glio_place_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_place_opts_default(&o_);
        check(glio_place_create_on_dense(dense, &o_, &h_), "glio_place_create_on_dense");
    }
    ~PlaceRecognition() { glio_place_destroy(h_); }
    PlaceRecognition(const PlaceRecognition&) = delete;
    PlaceRecognition& operator=(const PlaceRecognition&) = delete;
    glio_place* handle() const { return h_; }
    const glio_place_opts& opts() const { return o_; }
    // one launch for all frames; level_q [n][4] (w first) or empty.  Throws on a refusal, which leaves the store exactly as it was.
    void addFrames(const std::vector<int32_t>& frames, const std::vector<int32_t>& places, const std::vector<double>& times, const std::vector<double>& level_q = {}) {
        if (places.size() != frames.size() || times.size() != frames.size() || (!level_q.empty() && level_q.size() != 4 * frames.size()))
            throw std::invalid_argument("PlaceRecognition::addFrames: list lengths differ");
        check(glio_place_add_frames(h_, (int)frames.size(), frames.data(), places.data(), level_q.empty() ? nullptr : level_q.data(), times.data()), "glio_place_add_frames");
    }
    struct Descriptor { std::vector<float> heights; uint64_t mask; double time; bool valid; };
    Descriptor readDescriptor(int place) {
        Descriptor d;
        d.heights.assign((size_t)GLIO_PLACE_RINGS * GLIO_PLACE_SECTORS, 0.f);
        int32_t valid = 0;
        check(glio_place_read_descriptor(h_, place, d.heights.data(), &d.mask, &d.time, &valid), "glio_place_read_descriptor");
        d.valid = valid != 0;
        return d;
    }
    void setDescriptor(int place, const float* heights, uint64_t mask, double time) { check(glio_place_set_descriptor(h_, place, heights, mask, time), "glio_place_set_descriptor"); }
    void clear() { check(glio_place_clear(h_), "glio_place_clear"); }
    // the top_k candidates of `place` by ascending (distance, place)
    std::vector<glio_place_match> query(int place, double min_time_gap, int top_k = 1) {
        std::vector<glio_place_match> m((size_t)(top_k > 0 ? top_k : 0));
        int32_t n = 0;
        check(glio_place_query(h_, place, min_time_gap, top_k, m.data(), &n), "glio_place_query");
        m.resize((size_t)n);
        return m;
    }
    // places first .. first + n - 1 in one call: matches [n][top_k], n_found [n]
    void queryMany(int first, int n, double min_time_gap, bool earlier_only, int top_k, std::vector<glio_place_match>* matches, std::vector<int32_t>* n_found) {
        matches->assign((size_t)(n > 0 ? n : 0) * (size_t)(top_k > 0 ? top_k : 0), glio_place_match());
        n_found->assign((size_t)(n > 0 ? n : 0), 0);
        check(glio_place_query_many(h_, first, n, min_time_gap, earlier_only ? 1 : 0, top_k, matches->data(), n_found->data()), "glio_place_query_many");
    }
    float lastDeviceMs() { float ms = 0; check(glio_place_last_device_ms(h_, &ms), "glio_place_last_device_ms"); return ms; }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_place_opts o_;
    glio_place* h_ = nullptr;
};

namespace place_detail {
// Eigen's quaternion product, (w, x, y, z)
inline void qmul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3]; o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3]; o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
// the yaw of the ZYX Euler angles of q
inline double yawOf(const double q[4]) { return std::atan2(2.0 * (q[0] * q[3] + q[1] * q[2]), 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3])); }
inline void qz(double yaw, double o[4]) { o[0] = std::cos(0.5 * yaw); o[1] = 0.0; o[2] = 0.0; o[3] = std::sin(0.5 * yaw); }
}  // namespace place_detail

// the attitude q (w, x, y, z) with its yaw removed, qz(-yaw(q)) * q
inline void levelingQuaternion(const double q[4], double out[4]) {
    double z[4];
    place_detail::qz(-place_detail::yawOf(q), z);
    place_detail::qmul(z, q, out);
}

struct PlaceCandidate { int closest; double yaw; double distance; };
// The stored place closest to query_place among those more than time_thres away in time, taken when its distance is below dist_thres; closest = -1 (yaw 0) when
// there is none or |time_last_loop - time_new_odom| < 0.2 (Estimator.cpp:5127).
inline PlaceCandidate detectCandidateByAppearance(PlaceRecognition& pr, int query_place, double time_thres, double time_new_odom, double time_last_loop, double dist_thres = 0.2) {
    const std::vector<glio_place_match> m = pr.query(query_place, time_thres, 1);
    PlaceCandidate c;
    c.closest = -1; c.yaw = 0.0; c.distance = m.empty() ? INFINITY : (double)m[0].distance;
    if (m.empty() || !((double)m[0].distance < dist_thres)) return c;
    if (std::fabs(time_last_loop - time_new_odom) < 0.2) return c;
    c.closest = m[0].place; c.yaw = (double)m[0].yaw;
    return c;
}

// pose = t[3], q[4] (w first).  q_query null: both attitudes level, q = q_closest * qz(yaw); otherwise q = qz(yaw(q_closest) + yaw) * levelingQuaternion(q_query)
inline void placeInitialGuess(const double pose_closest[7], double yaw, const double* q_query, double out[7]) {
    for (int k = 0; k < 3; ++k) out[k] = pose_closest[k];
    double z[4];
    if (!q_query) {
        place_detail::qz(yaw, z);
        place_detail::qmul(pose_closest + 3, z, out + 3);
    } else {
        double lq[4];
        levelingQuaternion(q_query, lq);
        place_detail::qz(place_detail::yawOf(pose_closest + 3) + yaw, z);
        place_detail::qmul(z, lq, out + 3);
    }
}

}  // namespace glio
#endif  // GLIO_PLACE_BACKEND_HPP_

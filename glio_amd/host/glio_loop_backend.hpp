// glio_loop_backend.hpp -- the loop-closure thread of Estimator (GLIO/src/Estimator.cpp:5090-5273) on the C-ABI of include/glio_hip.h.  C-ABI only, C++14.
//
//   glio::LoopClosure          the device object (glio_loop_*): detectLoopClosure's submaps from the resident keyframe clouds of a glio_bassoc and
//                              performLoopClosure's pcl::IterativeClosestPoint (restated from PCL 1.8.1, UNPINNED: see glio_hip.h)
//   glio::detectLoopCandidate  :5113-5128   which keyframe closes the loop
//   glio::loopSubmapFrames     :5133-5175   which keyframes make the two submaps
//   glio::loopFramePoses       :5147-5148   their poses, as glio_loop_build_submap takes them
//   glio::loopConstraint       :5210-5247   the gate on the ICP result and the relative pose for the BetweenFactor
// The pose graph that takes the constraint and returns the corrected poses (:5249-5262) is glio::GlobalGraph / glio::PoseGraph (glio_posegraph_backend.hpp,
// glio_pgraph_*); a caller may keep GTSAM instead.  correctPoses' bookkeeping and the reset of the marginalization prior (:5264-5269) stay with the caller.
// The Python twin is glio_amd/loop.py: the same scalar arithmetic in the same order (tests/test_loop_host_cpu.py holds the two to each other bit for bit).
#ifndef GLIO_LOOP_BACKEND_HPP_
#define GLIO_LOOP_BACKEND_HPP_
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "glio_hip.h"

namespace glio {

class LoopClosure {
public:
    // `assoc` owns the resident keyframe clouds and must outlive this object
    explicit LoopClosure(glio_bassoc* assoc, const glio_loop_opts* opts = nullptr) {
        if (opts) o_ = *opts; else glio_loop_opts_default(&o_);
        check(glio_loop_create(assoc, &o_, &h_), "glio_loop_create");
    }
    ~LoopClosure() { glio_loop_destroy(h_); }
    LoopClosure(const LoopClosure&) = delete;
    LoopClosure& operator=(const LoopClosure&) = delete;
    glio_loop* handle() const { return h_; }
    const glio_loop_opts& opts() const { return o_; }
    // frames in list order, poses [n][7] = t, q (loopFramePoses); returns the filtered submap's size
    int buildSubmap(int which, const std::vector<int32_t>& frames, const std::vector<double>& poses) {
        int n = 0;
        check(glio_loop_build_submap(h_, which, (int)frames.size(), frames.data(), poses.data(), &n), "glio_loop_build_submap");
        return n;
    }
    void setSubmap(int which, const float* xyzi, int n) { check(glio_loop_set_submap(h_, which, xyzi, n), "glio_loop_set_submap"); }
    std::vector<float> readSubmap(int which) {
        int n = 0;
        check(glio_loop_read_submap(h_, which, nullptr, 0, &n), "glio_loop_read_submap");
        std::vector<float> out((size_t)n * 4);
        if (n > 0) check(glio_loop_read_submap(h_, which, out.data(), n, &n), "glio_loop_read_submap");
        return out;
    }
    glio_loop_result align() { glio_loop_result r; check(glio_loop_align(h_, &r), "glio_loop_align"); return r; }
    void resetCurrent() { check(glio_loop_reset_current(h_), "glio_loop_reset_current"); }
    glio_loop_step_result step() { glio_loop_step_result r; check(glio_loop_step(h_, &r), "glio_loop_step"); return r; }
    float lastDeviceMs() { float ms = 0; check(glio_loop_last_device_ms(h_, &ms), "glio_loop_last_device_ms"); return ms; }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_loop_opts o_;
    glio_loop* h_ = nullptr;
};

namespace loop_detail {
// Eigen's quaternion product, (w, x, y, z)
inline void qmul(const double a[4], const double b[4], double o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
// Eigen's quaternion * vector: v + w (2 u x v) + u x (2 u x v)
inline void qrot(const double q[4], const double v[3], double o[3]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    double uv[3] = {y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]};
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    const double uuv[3] = {y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]};
    o[0] = v[0] + w * uv[0] + uuv[0]; o[1] = v[1] + w * uv[1] + uuv[1]; o[2] = v[2] + w * uv[2] + uuv[2];
}
// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>): no flip to w >= 0, no normalisation
inline void eigenR2q(const double m[3][3], double q[4]) {
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[2][1] - m[1][2]) * t;
        q[2] = (m[0][2] - m[2][0]) * t;
        q[3] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[k][j] - m[j][k]) * t;
        q[1 + j] = (m[j][i] + m[i][j]) * t;
        q[1 + k] = (m[k][i] + m[i][k]) * t;
    }
}
}  // namespace loop_detail

// Estimator.cpp:5113-5128.  positions [n][3] float (pose_keyframe), times [n].  The keyframes within `radius` of select_pose (float squared distance
// (dx dx + dy dy) + dz dz, counted when (double) d2 < radius^2) by ascending squared distance, ties by index (PCL's radius search sorts; the tie rule is
// unpinned); the first whose |time - time_new_odom| > time_thres.  -1: no such keyframe, or |time_last_loop - time_new_odom| < 0.2.
inline int detectLoopCandidate(const float* positions, const double* times, int n, const float select_pose[3], double time_new_odom, double time_last_loop,
                               double radius, double time_thres) {
    std::vector<std::pair<float, int>> cand;
    const double r2 = radius * radius;
    for (int i = 0; i < n; ++i) {
        const float dx = positions[3 * i] - select_pose[0], dy = positions[3 * i + 1] - select_pose[1], dz = positions[3 * i + 2] - select_pose[2];
        const float a = dx * dx, b = dy * dy, c = dz * dz;
        const float ab = a + b;
        const float d2 = ab + c;
        if ((double)d2 < r2) cand.push_back(std::make_pair(d2, i));
    }
    std::sort(cand.begin(), cand.end());
    int closest = -1;
    for (size_t k = 0; k < cand.size(); ++k)
        if (std::fabs(times[cand[k].second] - time_new_odom) > time_thres) { closest = cand[k].second; break; }
    if (closest == -1) return -1;
    if (std::fabs(time_last_loop - time_new_odom) < 0.2) return -1;
    return closest;
}

// Estimator.cpp:5133-5175.  latest = n - W; source: latest - j for j = 0..5 where >= 0, in that order; target: closest + j for j = -w..w where
// 0 <= closest + j <= latest, ascending.
inline void loopSubmapFrames(int n_keyframes, int slide_window_width, int closest, int lc_map_width, int* latest_out, std::vector<int32_t>& source,
                             std::vector<int32_t>& target) {
    const int latest = n_keyframes - slide_window_width;
    source.clear(); target.clear();
    for (int j = 0; j < 6; ++j) if (latest - j >= 0) source.push_back(latest - j);
    for (int j = -lc_map_width; j <= lc_map_width; ++j) if (closest + j >= 0 && closest + j <= latest) target.push_back(closest + j);
    if (latest_out) *latest_out = latest;
}

// Estimator.cpp:5147-5148 for every row of pose_info [n][7] = t_po, q_po (w first): out [n][7] = t, q with q = q_po * q_bl, t = q_po * t_bl + t_po
inline void loopFramePoses(const double* pose_info, int n, const double q_bl[4], const double t_bl[3], double* out) {
    for (int k = 0; k < n; ++k) {
        const double* p = pose_info + 7 * k;
        double r[3];
        loop_detail::qmul(p + 3, q_bl, out + 7 * k + 3);
        loop_detail::qrot(p + 3, t_bl, r);
        for (int c = 0; c < 3; ++c) out[7 * k + c] = r[c] + p[c];
    }
}

// Estimator.cpp:5210-5247.  false when !converged or fitness > icp_thres (:5210).  Otherwise qIncre = Eigen::Quaterniond(rotation block cast to double),
// poseFrom = (qIncre * q, qIncre * t + tIncre) of pose_latest, poseTo = pose_closest (poses = t[3], q[4]); relative [7] = t, q of poseFrom^-1 * poseTo,
// variances [6] all = fitness.  The two rotations enter the relative pose as UNIT quaternions (gtsam::Rot3::Quaternion builds a rotation from them).
inline bool loopConstraint(const glio_loop_result& res, const double pose_latest[7], const double pose_closest[7], double icp_thres, double relative[7],
                           double variances[6]) {
    if (!res.converged || res.fitness > icp_thres) return false;
    double R[3][3], ti[3], qi[4], qf[4], r[3], tf[3];
    for (int a = 0; a < 3; ++a) { for (int c = 0; c < 3; ++c) R[a][c] = (double)res.transform[4 * a + c]; ti[a] = (double)res.transform[4 * a + 3]; }
    loop_detail::eigenR2q(R, qi);
    loop_detail::qmul(qi, pose_latest + 3, qf);
    loop_detail::qrot(qi, pose_latest, r);
    for (int c = 0; c < 3; ++c) tf[c] = r[c] + ti[c];
    const double nf = std::sqrt(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3]);
    for (int c = 0; c < 4; ++c) qf[c] = qf[c] / nf;
    double qt[4] = {pose_closest[3], pose_closest[4], pose_closest[5], pose_closest[6]};
    const double nt = std::sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
    for (int c = 0; c < 4; ++c) qt[c] = qt[c] / nt;
    const double qfi[4] = {qf[0], -qf[1], -qf[2], -qf[3]};
    const double d[3] = {pose_closest[0] - tf[0], pose_closest[1] - tf[1], pose_closest[2] - tf[2]};
    loop_detail::qmul(qfi, qt, relative + 3);
    loop_detail::qrot(qfi, d, relative);
    for (int c = 0; c < 6; ++c) variances[c] = res.fitness;
    return true;
}

// The sliding window's share of correctPoses (Estimator.cpp:4664-4686, :4702-4773).  abs_poses [N][7] = q (w first), t, in/out -- the estimator's abs_poses, where
// row i + 1 belongs to keyframe i; W = slide_window_width; corrected [N - W][7], same layout: the pose-graph poses of keyframes 0 .. N - 1 - W
// (pose_each_frame[keyframe_id_in_frame[i]], :4702-4713).  (1) the W - 1 relative poses between rows N - W .. N - 1 are taken BEFORE anything is corrected,
// q_rel = q_from.inverse() * q_to, t_rel = q_from.inverse() * (t_to - t_from), Eigen's inverse() = conjugate / squaredNorm; (2) rows 1 .. N - W take the
// corrected poses; (3) rows N - W + 1 .. N - 1 are chained back on: t = t_prev + q_prev * t_rel, q = q_prev * q_rel.  Rs [N][9] (row-major toRotationMatrix(),
// not normalised) and Ps [N][3] receive every rewritten row (row 0 is not written; either may be null).  pose_keyframe / pose_info_keyframe[i] are row i + 1.
// The corrected poses come from glio::GlobalGraph::keyframePoses (glio_posegraph_backend.hpp; or from the caller's GTSAM / iSAM2).  What stays with the caller:
// pose_each_frame, recent_surf_keyframes.clear() (SlidingWindowBackend::loopClosed), marg = false
// (glio_set_prior(NULL)).  The Python twin is loop.correct_window_poses (tests/test_map_schedule_host_cpu.py: bit for bit).  false: bad sizes.
inline bool correctWindowPoses(double* abs_poses, int N, const double* corrected, int n_corrected, int W, double* Rs, double* Ps) {
    if (W < 1 || W > N || n_corrected != N - W) return false;
    auto q2R = [](const double q[4], double R[9]) {
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
        const double twx = tx * w, twy = ty * w, twz = tz * w;
        const double txx = tx * x, txy = ty * x, txz = tz * x;
        const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
        R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
        R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
        R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
    };
    auto book = [&](int row) {
        if (Rs) q2R(abs_poses + 7 * row, Rs + 9 * row);
        if (Ps) for (int c = 0; c < 3; ++c) Ps[3 * row + c] = abs_poses[7 * row + 4 + c];
    };
    std::vector<double> rel((size_t)(W > 1 ? W - 1 : 0) * 7);
    for (int i = N - W, k = 0; i < N - 1; ++i, ++k) {
        const double* from = abs_poses + 7 * i; const double* to = abs_poses + 7 * (i + 1);
        const double n2 = from[0] * from[0] + from[1] * from[1] + from[2] * from[2] + from[3] * from[3];
        double qi[4] = {0.0, 0.0, 0.0, 0.0};
        if (n2 > 0.0) { qi[0] = from[0] / n2; qi[1] = -from[1] / n2; qi[2] = -from[2] / n2; qi[3] = -from[3] / n2; }
        const double d[3] = {to[4] - from[4], to[5] - from[5], to[6] - from[6]};
        loop_detail::qmul(qi, to, &rel[7 * (size_t)k]);
        loop_detail::qrot(qi, d, &rel[7 * (size_t)k + 4]);
    }
    for (int i = 0; i < N - W; ++i) {
        for (int c = 0; c < 7; ++c) abs_poses[7 * (i + 1) + c] = corrected[7 * i + c];
        book(i + 1);
    }
    for (int i = N - W, k = 0; i < N - 1; ++i, ++k) {
        const double* prev = abs_poses + 7 * i;
        double r[3], q[4];
        loop_detail::qrot(prev, &rel[7 * (size_t)k + 4], r);
        loop_detail::qmul(prev, &rel[7 * (size_t)k], q);
        double* out = abs_poses + 7 * (i + 1);
        for (int c = 0; c < 3; ++c) out[4 + c] = prev[4 + c] + r[c];
        for (int c = 0; c < 4; ++c) out[c] = q[c];
        book(i + 1);
    }
    return true;
}

}  // namespace glio
#endif  // GLIO_LOOP_BACKEND_HPP_

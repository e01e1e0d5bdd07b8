// glio_posegraph_backend.hpp -- the pose graphs of Estimator (GLIO/src/Estimator.cpp: the global graph :4586-4652, :5251-5256; the local graph :4561-4581,
// addLIOFactor :1999-2043, addGNSSFactor :1915-1997) on the C-ABI of include/glio_hip.h.  C-ABI only, C++14, no HIP headers.
//
//   glio::PoseGraph           the device object (glio_pgraph_*): poses t[3], q[4] (w first), factors and retraction as stated in glio_hip.h, every solve the
//                             batch Gauss-Newton estimate (the two stated deviations from GTSAM / iSAM2 are in the header)
//   glio::globalGraphFrames   :4589-4611   the frame ids that enter the global graph at a keyframe call
//   glio::loopEdgeFrames      :5251-5252   the loop's edge joins frame ids
//   glio::GlobalGraph         the global graph fed per keyframe call, the loop edge, the corrected keyframe poses (correctPoses :4702-4713)
//   glio::GnssGate            :1915-1997   every gate of addGNSSFactor, without GTSAM
//   glio::LocalGraph          addLIOFactor's node per keyframe that left the window, the gate, the solve and poseCovariance (:4563-4578)
// What PoseGraph::readPoses returns is what glio::correctWindowPoses (after its q, t reordering), glio_localmap_rebuild_from_frames, glio_loop_build_submap and
// glio_gmap_add_frames take (through glio::loopFramePoses where the LiDAR offset applies).  The Python twin is glio_amd/posegraph.py: the same scalar
// arithmetic in the same order (tests/test_pose_graph_host_cpu.py).
#ifndef GLIO_POSEGRAPH_BACKEND_HPP_
#define GLIO_POSEGRAPH_BACKEND_HPP_
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_hip.h"
#include "glio_pgraph_cov.h"

namespace glio {

// Estimator.cpp:4589-4611.  n_keyframes < W: none; == W: frame 0 (with the prior); > W: keyframe_id_in_frame[n - W - 1] + 1 .. keyframe_id_in_frame[n - W]
inline std::vector<int32_t> globalGraphFrames(const std::vector<int32_t>& keyframe_id_in_frame, int n_keyframes, int W) {
    std::vector<int32_t> out;
    if (n_keyframes < W) return out;
    if (n_keyframes == W) { out.push_back(0); return out; }
    for (int32_t i = keyframe_id_in_frame[n_keyframes - W - 1] + 1; i <= keyframe_id_in_frame[n_keyframes - W]; ++i) out.push_back(i);
    return out;
}
// Estimator.cpp:5251-5252
inline void loopEdgeFrames(const std::vector<int32_t>& keyframe_id_in_frame, int latest_keyframe, int closest_keyframe, int* i, int* j) {
    *i = keyframe_id_in_frame[latest_keyframe]; *j = keyframe_id_in_frame[closest_keyframe];
}

class PoseGraph {
public:
    explicit PoseGraph(const glio_pgraph_opts* opts = nullptr, int device = 0) {
        if (opts) o_ = *opts; else glio_pgraph_opts_default(&o_);
        check(glio_pgraph_create(device, &o_, &h_), "glio_pgraph_create");
    }
    ~PoseGraph() { glio_pgraph_destroy(h_); }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;
    glio_pgraph* handle() const { return h_; }
    const glio_pgraph_opts& opts() const { return o_; }
    void clear() { check(glio_pgraph_clear(h_), "glio_pgraph_clear"); }
    void setPrior(const double pose[7], const double* var = nullptr) { check(glio_pgraph_set_prior(h_, pose, var), "glio_pgraph_set_prior"); }
    // n nodes with poses [n][7] as initial estimates and one between factor each; prev_pose: the caller's pose of the current last node (null: its estimate)
    void append(int n, const double* poses, const double* prev_pose = nullptr, const double* var = nullptr) {
        check(glio_pgraph_append(h_, n, poses, prev_pose, var), "glio_pgraph_append");
    }
    void addBetween(int i, int j, const double rel[7], const double var[6]) { check(glio_pgraph_add_between(h_, i, j, rel, var), "glio_pgraph_add_between"); }
    void addGps(int i, const double xyz[3], const double var[3]) { check(glio_pgraph_add_gps(h_, i, xyz, var), "glio_pgraph_add_gps"); }
    glio_pgraph_info solve() { glio_pgraph_info info; check(glio_pgraph_solve(h_, &info), "glio_pgraph_solve"); return info; }
    // glio_pgraph_solve_damped: the solve that never leaves a worse estimate (lm_opts null: the defaults); lm (may be null): its counters and final radius;
    // history (may be null): per trial E tried, the radius used, the model decrease, 1 accepted / 0 rejected / -1 invalid
    glio_pgraph_info solveDamped(const glio_pgraph_lm_opts* lm_opts = nullptr, glio_pgraph_lm_info* lm = nullptr, std::vector<double>* history = nullptr) {
        glio_pgraph_info info;
        glio_pgraph_lm_info li;
        check(glio_pgraph_solve_damped(h_, lm_opts, &info, &li), "glio_pgraph_solve_damped");
        if (lm) *lm = li;
        if (history) {
            history->assign((size_t)4 * li.trials, 0.0);
            check(glio_pgraph_lm_history(h_, 0, li.trials, history->data()), "glio_pgraph_lm_history");
        }
        return info;
    }
    int size() { int n = 0; check(glio_pgraph_size(h_, &n), "glio_pgraph_size"); return n; }
    std::vector<double> readPoses(int first, int n) {
        std::vector<double> out((size_t)(n > 0 ? n : 0) * 7);
        check(glio_pgraph_read_poses(h_, first, n, out.data()), "glio_pgraph_read_poses");
        return out;
    }
    std::vector<double> readPoses() { return readPoses(0, size()); }
    // row major 6x6, rotation first
    std::vector<double> marginalCovariance(int node) {
        std::vector<double> out(36);
        check(glio_pgraph_marginal_covariance(h_, node, out.data()), "glio_pgraph_marginal_covariance");
        return out;
    }
    // glio_pgraph_covariance_all (glio_pgraph_cov.h): block (i, i) of (J^T J)^-1 of EVERY node from one factorisation, [N][36] row major, rotation first;
    // next (may be null): the blocks (i, i + 1), [N - 1][36]; info (may be null): the plan used, the factor's squared diagonal, the node of a failed pivot
    std::vector<double> marginalCovariances(std::vector<double>* next = nullptr, glio_pgraph_cov_info* info = nullptr) {
        const int n = size();
        std::vector<double> diag((size_t)36 * (n > 0 ? n : 1));
        if (next) next->assign((size_t)36 * (n > 1 ? n - 1 : 1), 0.0);
        check(glio_pgraph_covariance_all(h_, diag.data(), next ? next->data() : nullptr, info), "glio_pgraph_covariance_all");
        diag.resize((size_t)36 * n);
        if (next) next->resize((size_t)36 * (n > 1 ? n - 1 : 0));
        return diag;
    }
    double error() { double e = 0; check(glio_pgraph_error(h_, &e), "glio_pgraph_error"); return e; }
    const double* posesDev(int* n = nullptr) { const double* p = nullptr; check(glio_pgraph_poses_dev(h_, &p, n), "glio_pgraph_poses_dev"); return p; }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_pgraph* h_ = nullptr;
    glio_pgraph_opts o_;
};

// The global graph's bookkeeping: one node per frame, fed per keyframe call (:4586-4652)
class GlobalGraph {
public:
    GlobalGraph(PoseGraph* graph, int W) : g_(graph), W_(W) {}
    // pose_each_frame [F][7] = t, q of every frame so far; returns the frame ids added
    std::vector<int32_t> keyframeCall(const std::vector<double>& pose_each_frame, const std::vector<int32_t>& keyframe_id_in_frame, int n_keyframes) {
        std::vector<int32_t> ids = globalGraphFrames(keyframe_id_in_frame, n_keyframes, W_);
        if (ids.empty()) return ids;
        const double* P = pose_each_frame.data();
        if (ids.size() == 1 && ids[0] == 0 && g_->size() == 0) {
            g_->setPrior(P);
            g_->append(1, P);
            return ids;
        }
        if (ids[0] != g_->size()) throw std::logic_error("GlobalGraph::keyframeCall: frames are not contiguous with the graph");
        g_->append((int)ids.size(), P + (size_t)7 * ids[0], P + (size_t)7 * (ids[0] - 1));
        return ids;
    }
    // rel [7], var [6] = glio::loopConstraint's; adds the edge (:5251-5254) and solves (:5255-5261).  damped: PoseGraph::solveDamped instead -- the call for a
    // loop over a long drive, where the undamped step can raise the error; lm (may be null): its counters
    glio_pgraph_info loopClosed(const std::vector<int32_t>& keyframe_id_in_frame, int latest_keyframe, int closest_keyframe, const double rel[7], const double var[6],
                                bool damped = false, glio_pgraph_lm_info* lm = nullptr) {
        int i, j;
        loopEdgeFrames(keyframe_id_in_frame, latest_keyframe, closest_keyframe, &i, &j);
        g_->addBetween(i, j, rel, var);
        return damped ? g_->solveDamped(nullptr, lm) : g_->solve();
    }
    // pose_each_frame[keyframe_id_in_frame[i]] of the corrected estimate, keyframes 0 .. n - 1 (:4702-4713): rows t, q
    std::vector<double> keyframePoses(const std::vector<int32_t>& keyframe_id_in_frame, int n) {
        const std::vector<double> all = g_->readPoses();
        std::vector<double> out((size_t)7 * n);
        for (int k = 0; k < n; ++k) std::copy(all.begin() + (size_t)7 * keyframe_id_in_frame[k], all.begin() + (size_t)7 * keyframe_id_in_frame[k] + 7, out.begin() + (size_t)7 * k);
        return out;
    }
private:
    PoseGraph* g_;
    int W_;
};

// pointDistance(PointType, PointType) (:1570-1573): float differences, products and sum, the square root in double
inline double pointDistanceF32(const float a[3], const float b[3]) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;       // separate statements: no contraction across them
    const float s1 = xx + yy;
    const float s = s1 + zz;
    return std::sqrt((double)s);
}
// pointDistance(PointPoseInfo, PointPoseInfo) (:1575-1578)
inline double pointDistanceF64(const double a[3], const double b[3]) {
    const double xx = (a[0] - b[0]) * (a[0] - b[0]), yy = (a[1] - b[1]) * (a[1] - b[1]), zz = (a[2] - b[2]) * (a[2] - b[2]);
    const double s1 = xx + yy;
    const double s = s1 + zz;
    return std::sqrt(s);
}

struct GnssFix { double stamp; double xyz[3]; double cov[3]; };       // nav_msgs::Odometry: header.stamp, pose.pose.position, pose.covariance[0..2]
struct GnssFactor { int node; double xyz[3]; double var[3]; };

// addGNSSFactor (:1915-1997) without GTSAM
class GnssGate {
public:
    explicit GnssGate(double timeshift = 0.0, double gnss_cov_threshold = 200.0, double pose_cov_threshold = 1.0)
        : timeshift_(timeshift), gnss_thr_(gnss_cov_threshold), pose_thr_(pose_cov_threshold) {}
    void push(const GnssFix& f) { queue_.push_back(f); }
    size_t queued() const { return queue_.size(); }
    // keyframe_xyz / keyframe_time: pose_info_keyframe[n_keyframes - W]; cov33 / cov44: poseCovariance(3,3), (4,4).  true: *out is the factor to add
    bool select(int n_keyframes, int W, const double keyframe_xyz[3], double keyframe_time, double cov33, double cov44, GnssFactor* out) {
        if (n_keyframes <= W) return false;                                             // :1918
        const int idx = n_keyframes - W;
        if (queue_.empty()) return false;                                               // :1922
        if (pointDistanceF64(last_add_pos_, keyframe_xyz) < 5) return false;            // :1932
        if (cov33 < pose_thr_ && cov44 < pose_thr_) return false;                       // :1938
        const double t = keyframe_time + timeshift_;                                    // :1946
        while (!queue_.empty()) {
            const GnssFix f = queue_.front();
            if (f.stamp < t - 0.2) queue_.pop_front();                                  // :1950
            else if (f.stamp > t + 0.2) break;                                          // :1954
            else {
                queue_.pop_front();
                const float nx = (float)f.cov[0], ny = (float)f.cov[1], nz = (float)f.cov[2];      // :1964-1966
                if (nx > gnss_thr_ || ny > gnss_thr_) continue;                         // :1967
                const float g[3] = {(float)f.xyz[0], (float)f.xyz[1], (float)f.xyz[2]}; // :1971-1973
                if (pointDistanceF32(g, last_gps_) < 5) continue;                       // :1980
                for (int k = 0; k < 3; ++k) last_gps_[k] = g[k];
                out->node = idx;
                const float n3[3] = {nx, ny, nz};
                for (int k = 0; k < 3; ++k) { out->xyz[k] = g[k]; out->var[k] = std::max(n3[k], 1.0f); last_add_pos_[k] = keyframe_xyz[k]; }      // :1986, :1992
                return true;
            }
        }
        return false;
    }
private:
    double timeshift_, gnss_thr_, pose_thr_;
    double last_add_pos_[3] = {0, 0, 0};        // last_GNSS_add_pos (:499-501)
    float last_gps_[3] = {0, 0, 0};             // static PointType lastGPSPoint (:1943)
    std::deque<GnssFix> queue_;
};

// The local graph's bookkeeping (:4563-4578)
class LocalGraph {
public:
    LocalGraph(PoseGraph* graph, int W, GnssGate* gate) : g_(graph), W_(W), gate_(gate), cov_(36, 0.0) {}
    // pose_info_keyframe [n][7] = t, q; keyframe_time [n].  Returns false when the call adds nothing (n_keyframes < W); *gps_added, *info may be null
    bool keyframeCall(const std::vector<double>& pose_info_keyframe, const std::vector<double>& keyframe_time, int n_keyframes, bool* gps_added, glio_pgraph_info* info) {
        if (n_keyframes < W_) return false;                                             // :4563
        const double* P = pose_info_keyframe.data();
        const int idx = n_keyframes - W_;
        if (n_keyframes == W_) { g_->setPrior(P); g_->append(1, P); }                   // :2003-2015
        else {                                                                          // :2018-2041
            if (idx != g_->size()) throw std::logic_error("LocalGraph::keyframeCall: keyframes are not contiguous with the graph");
            g_->append(1, P + (size_t)7 * idx, P + (size_t)7 * (idx - 1));
        }
        GnssFactor f;
        const bool add = gate_->select(n_keyframes, W_, P + (size_t)7 * idx, keyframe_time[idx], cov_[6 * 3 + 3], cov_[6 * 4 + 4], &f);
        if (add) g_->addGps(f.node, f.xyz, f.var);
        const glio_pgraph_info r = g_->solve();                                         // :4566-4577
        cov_ = g_->marginalCovariance(g_->size() - 1);                                  // :4578
        if (gps_added) *gps_added = add;
        if (info) *info = r;
        return true;
    }
    const std::vector<double>& poseCovariance() const { return cov_; }
private:
    PoseGraph* g_;
    int W_;
    GnssGate* gate_;
    std::vector<double> cov_;
};

}  // namespace glio
#endif

// glio_trajectory_backend.hpp -- the every-frame trajectory of Estimator::saveKeyFramesAndFactors (GLIO/src/Estimator.cpp:4273-4557, optimizeLocalGraph
// :3452-3527) on the C-ABI of include/glio_traj.h.  C-ABI only, C++14, no HIP headers.
//
//   glio::frameImuSamples     :4287-4375, :4399-4481   which IMU samples make the segments of a gap (the host's share, as glio::keyframeImuSamples is)
//   glio::TrajectoryStore     the device object (glio_traj_*): push a gap, read it, solve every stored gap again between new keyframe poses
//   glio::Trajectory          pose_each_frame and keyframe_id_in_frame for the caller: keyframeCall per keyframe, poses() for GlobalGraph::keyframeCall,
//                             resolveAll after optimizeBatch / correctPoses
// The Python twin is glio_amd/trajectory.py: the same scalar arithmetic in the same order (tests/test_trajectory_host_cpu.py).
#ifndef GLIO_TRAJECTORY_BACKEND_HPP_
#define GLIO_TRAJECTORY_BACKEND_HPP_
#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "glio_traj.h"

namespace glio {

struct FrameSegments {
    std::vector<int32_t> seg_offset;          // [n_segments + 1]
    std::vector<glio_imu_sample> samples;
    size_t imu_idx;                           // the running index as the reference leaves it
};

namespace traj_detail {
inline double clampAcc(double v, double lim) {
    if (v > lim) v = lim;
    if (v < -lim) v = -lim;
    return v;
}
}  // namespace traj_detail

// frame_stamps: the stamps of frames keyframe_id_in_frame[a] .. keyframe_id_in_frame[b]; imu_idx = imu_idx_in_kf[a].  Per segment the start row (dt 0: the
// sample interpolated at the segment's first stamp, NOT clamped for an in-between segment :4295-4301, clamped for the last one :4413-4419), the whole
// samples strictly before the next stamp (clamped), the closing row with dt1 interpolated from the values of the last row taken -- the CLAMPED acc of the
// last whole sample (:4348) -- and clamped.  The index steps back after an in-between frame (:4375).
inline FrameSegments frameImuSamples(const std::vector<double>& stamps, const std::vector<std::array<double, 3>>& acc, const std::vector<std::array<double, 3>>& gyr,
                                     const std::vector<double>& frame_stamps, size_t imu_idx) {
    static const double LIM[3] = {15.0, 15.0, 18.0};
    FrameSegments out;
    out.seg_offset.push_back(0);
    size_t ii = imu_idx;
    const size_t M = frame_stamps.empty() ? 0 : frame_stamps.size() - 1;
    for (size_t i = 1; i <= M; ++i) {
        const bool last = i == M;
        const double t0 = frame_stamps[i - 1], t1 = frame_stamps[i];
        double dt1 = t0 - stamps[ii];
        double dt2 = stamps[ii + 1] - t0;
        double w1 = dt2 / (dt1 + dt2);
        double w2 = dt1 / (dt1 + dt2);
        double d[3], r[3];
        for (int k = 0; k < 3; ++k) {
            const double da = w1 * acc[ii][k], db = w2 * acc[ii + 1][k];          // separate statements: no contraction across them
            d[k] = da + db;
            const double ra = w1 * gyr[ii][k], rb = w2 * gyr[ii + 1][k];
            r[k] = ra + rb;
        }
        if (last) for (int k = 0; k < 3; ++k) d[k] = traj_detail::clampAcc(d[k], LIM[k]);
        glio_imu_sample s;
        s.dt = 0.0;
        for (int k = 0; k < 3; ++k) { s.acc[k] = d[k]; s.gyr[k] = r[k]; }
        out.samples.push_back(s);
        ++ii;
        double start = t0;
        while (stamps[ii] < t1) {
            const double t = stamps[ii];
            s.dt = t - start;
            start = t;
            for (int k = 0; k < 3; ++k) { d[k] = traj_detail::clampAcc(acc[ii][k], LIM[k]); r[k] = gyr[ii][k]; s.acc[k] = d[k]; s.gyr[k] = r[k]; }
            out.samples.push_back(s);
            ++ii;
        }
        dt1 = t1 - stamps[ii - 1];
        dt2 = stamps[ii] - t1;
        w1 = dt2 / (dt1 + dt2);
        w2 = dt1 / (dt1 + dt2);
        for (int k = 0; k < 3; ++k) {
            const double da = w1 * d[k], db = w2 * acc[ii][k];
            d[k] = traj_detail::clampAcc(da + db, LIM[k]);
            const double ra = w1 * r[k], rb = w2 * gyr[ii][k];
            r[k] = ra + rb;
        }
        s.dt = dt1;
        for (int k = 0; k < 3; ++k) { s.acc[k] = d[k]; s.gyr[k] = r[k]; }
        out.samples.push_back(s);
        if (!last) --ii;
        out.seg_offset.push_back((int32_t)out.samples.size());
    }
    out.imu_idx = ii;
    return out;
}

class TrajectoryStore {
public:
    explicit TrajectoryStore(const glio_traj_opts* opts = nullptr, int device = 0) {
        if (opts) o_ = *opts; else glio_traj_opts_default(&o_);
        check(glio_traj_create(device, &o_, &h_), "glio_traj_create");
        n_.assign((size_t)o_.max_gaps, -1);
    }
    ~TrajectoryStore() { glio_traj_destroy(h_); }
    TrajectoryStore(const TrajectoryStore&) = delete;
    TrajectoryStore& operator=(const TrajectoryStore&) = delete;
    glio_traj* handle() const { return h_; }
    const glio_traj_opts& opts() const { return o_; }
    // asynchronous: returns once the inputs are copied.  start_state [15] = P, V, R (row major)
    void pushGap(int gap, int n_frames, const FrameSegments& seg, const double* start_state, const double gravity[3], const double prev_row[7],
                 const double anchor_left[7], const double anchor_right[7]) {
        check(glio_traj_push_gap(h_, gap, n_frames, seg.seg_offset.data(), seg.samples.data(), start_state, gravity, prev_row, anchor_left, anchor_right), "glio_traj_push_gap");
        n_[(size_t)gap] = n_frames;
    }
    // keyframe_poses [n_gaps + 1][7]; summaries (may be null): waits
    void resolve(int first_gap, int n_gaps, const double* keyframe_poses, std::vector<glio_traj_summary>* summaries = nullptr) {
        if (summaries) summaries->assign((size_t)(n_gaps > 0 ? n_gaps : 0), glio_traj_summary());
        check(glio_traj_resolve(h_, first_gap, n_gaps, keyframe_poses, summaries && n_gaps > 0 ? summaries->data() : nullptr), "glio_traj_resolve");
    }
    int frames(int gap) const { return n_[(size_t)gap]; }
    // the solved rows [N][7] of a gap (waits for that gap only); summary may be null
    std::vector<double> readSolved(int gap, glio_traj_summary* summary = nullptr) {
        const int N = n_[(size_t)gap] > 0 ? n_[(size_t)gap] : 0;
        std::vector<double> out((size_t)7 * N);
        check(glio_traj_read(h_, gap, summary, nullptr, nullptr, N ? out.data() : nullptr), "glio_traj_read");
        return out;
    }
    void read(int gap, glio_traj_summary* summary, std::vector<double>* dead_reckoned, std::vector<double>* measurements, std::vector<double>* solved) {
        const int N = n_[(size_t)gap] > 0 ? n_[(size_t)gap] : 0;
        if (dead_reckoned) dead_reckoned->assign((size_t)7 * (N + 1), 0.0);
        if (measurements) measurements->assign((size_t)7 * (N + 1), 0.0);
        if (solved) solved->assign((size_t)7 * N, 0.0);
        check(glio_traj_read(h_, gap, summary, dead_reckoned ? dead_reckoned->data() : nullptr, measurements ? measurements->data() : nullptr,
                             solved && N ? solved->data() : nullptr), "glio_traj_read");
    }
private:
    static void check(int rc, const char* what) {
        if (rc != GLIO_OK) throw std::runtime_error(std::string(what) + ": " + glio_last_error());
    }
    glio_traj* h_ = nullptr;
    glio_traj_opts o_;
    std::vector<int> n_;
};

// pose_each_frame (rows t, q) and keyframe_id_in_frame, fed once per keyframe call.  Gap k lies between keyframes k and k + 1.
class Trajectory {
public:
    Trajectory(TrajectoryStore* store, int W, const double gravity[3] = nullptr) : s_(store), W_(W) {
        g_[0] = gravity ? gravity[0] : 0.0; g_[1] = gravity ? gravity[1] : 0.0; g_[2] = gravity ? gravity[2] : 9.805;
    }
    // keyframe_frame_id: the frame the new keyframe is; keyframe_poses [n][7]: pose_info_keyframe after this call's window solve; frame_stamps: every frame
    // so far; start_state [15] = Ps, Vs, Rs at Ps.size() - W -- the keyframe AFTER the one the IMU index and the first frame belong to (:4281-4283 against
    // :4279, :4287; glio_traj.h names the quirk).  Returns the gap pushed or -1.  Asynchronous: the in-between rows arrive with poses().
    int keyframeCall(int32_t keyframe_frame_id, const std::vector<double>& keyframe_poses, const std::vector<double>& frame_stamps, const std::vector<double>& imu_stamps,
                     const std::vector<std::array<double, 3>>& imu_acc, const std::vector<std::array<double, 3>>& imu_gyr, const std::vector<size_t>& imu_idx_in_kf,
                     const double* start_state) {
        kf_id_.push_back(keyframe_frame_id);
        const int n = (int)kf_id_.size();
        const double* kp = keyframe_poses.data();
        if (n == W_) { rows_.insert(rows_.end(), kp, kp + 7); return -1; }          // :4274-4277
        if (n < W_) return -1;
        const int a = n - W_ - 1, b = n - W_;
        const int32_t fa = kf_id_[a], fb = kf_id_[b];
        const int N = fb - fa - 1;
        const std::vector<double> fs(frame_stamps.begin() + fa, frame_stamps.begin() + fb + 1);
        const FrameSegments seg = frameImuSamples(imu_stamps, imu_acc, imu_gyr, fs, imu_idx_in_kf[a]);
        if ((int)(rows_.size() / 7) != fa + 1) throw std::logic_error("Trajectory::keyframeCall: keyframe calls are not contiguous with the trajectory");
        s_->pushGap(a, N, seg, start_state, g_, rows_.data() + (size_t)7 * fa, kp + (size_t)7 * a, kp + (size_t)7 * b);
        pending_.push_back({a, fa + 1, N});
        rows_.resize(rows_.size() + (size_t)7 * N, 0.0);                             // the solved rows, read on demand
        rows_.insert(rows_.end(), kp + (size_t)7 * b, kp + (size_t)7 * b + 7);       // :4397-4398
        return a;
    }
    // pose_each_frame [F][7]: what GlobalGraph::keyframeCall takes (waits for the gaps pushed since the last call)
    const std::vector<double>& poses() { flush(); return rows_; }
    const std::vector<int32_t>& keyframeIdInFrame() const { return kf_id_; }
    // every in-between row solved again between the rows of keyframe_poses [>= n_gaps + 1][7]: one launch
    std::vector<glio_traj_summary> resolveAll(const std::vector<double>& keyframe_poses) {
        flush();
        std::vector<glio_traj_summary> summ;
        const int G = (int)kf_id_.size() - W_;
        if (G < 1) return summ;
        s_->resolve(0, G, keyframe_poses.data(), &summ);
        for (int k = 0; k <= G; ++k) std::copy(keyframe_poses.begin() + (size_t)7 * k, keyframe_poses.begin() + (size_t)7 * k + 7, rows_.begin() + (size_t)7 * kf_id_[k]);
        for (int k = 0; k < G; ++k) {
            const int N = kf_id_[k + 1] - kf_id_[k] - 1;
            if (N <= 0) continue;
            const std::vector<double> sol = s_->readSolved(k);
            std::copy(sol.begin(), sol.end(), rows_.begin() + (size_t)7 * (kf_id_[k] + 1));
        }
        return summ;
    }
private:
    struct Pending { int gap, first, n; };
    void flush() {
        for (const Pending& p : pending_) {
            const std::vector<double> sol = s_->readSolved(p.gap);
            std::copy(sol.begin(), sol.end(), rows_.begin() + (size_t)7 * p.first);
        }
        pending_.clear();
    }
    TrajectoryStore* s_;
    int W_;
    double g_[3];
    std::vector<int32_t> kf_id_;
    std::vector<double> rows_;
    std::vector<Pending> pending_;
};

}  // namespace glio
#endif

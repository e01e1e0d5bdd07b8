// glio_backend.hpp -- host-side C++ mirror of the reference interface for the sliding-window hot path.
//
// Plain C++14, no HIP / torch / Ceres / Eigen headers: this is what a GLIO maintainer compiles into
// GLIO/src/Estimator.cpp and links against libglio_hip.so.  Two layers:
//   (1) factor shims with the exact ceres::CostFunction::Evaluate() signature (reference
//       GLIO/include/factors/LidarKeyframeFactor.h:73-122, ImuFactor.h:12-175) -- derive them from
//       ceres::SizedCostFunction<...> when Ceres is present;
//   (2) SlidingWindowBackend: the buffers optimizeSlidingWindowWithLandMark() works on (tmpTrans/tmpQuat/
//       tmpSpeedBias, Ps/Rs/Vs/Bas/Bgs, Estimator.cpp:345-348) and its call sequence (:2046-2736).
#pragma once

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/glio_cov.h"
#include "../../include/glio_hip.h"

namespace glio {

struct Error : std::runtime_error {
    explicit Error(const std::string& what) : std::runtime_error(what + ": " + glio_last_error()) {}
};
inline void check(int rc, const char* what) { if (rc != GLIO_OK) throw Error(what); }

// The 6 x 6 pose block of SlidingWindowBackend::covariance (columns 15 s .. 15 s + 5 of slot s: translation, then the quaternion's tangent) at the slot's
// quaternion q = (w, x, y, z), in GTSAM's Pose3 order and chart: rotation first, body-frame rotation vector in radians, translation increment R v -- the
// order glio_pgraph_* variances and the reference's poseCovariance(3,3), (4,4) gate are written in.  Row major in and out.
//   The window moves a pose by  t' = t + dt,  q' = (cos |d|, sin |d| d / |d|) * q  (Ceres' QuaternionParameterization: d multiplies on the LEFT and is HALF a
//   rotation vector), i.e. R' = Exp(2 d) R with R = R(q).  Pose3's chart moves it by  R' = R Exp(omega),  t' = t + R v.
//   Exp(2 d) R = R Exp(R^T 2 d) exactly, so omega = 2 R^T d; and t + dt = t + R v gives v = R^T dt.  Both are linear in (dt, d): to first order (and for the
//   rotation at any size) (omega, v) = A (dt, d) with the constant
//       A = [ 0     2 R^T ]
//           [ R^T   0     ]
//   and the covariance maps as A Sigma A^T.  sliding.pose3_covariance is the Python twin.
inline std::array<double, 36> pose3Covariance(const double* cov6, const double q_in[4]) {
    const double nq = std::sqrt(q_in[0] * q_in[0] + q_in[1] * q_in[1] + q_in[2] * q_in[2] + q_in[3] * q_in[3]);
    const double w = q_in[0] / nq, x = q_in[1] / nq, y = q_in[2] / nq, z = q_in[3] / nq;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    double A[36] = {0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[6 * i + 3 + j] = 2.0 * R[3 * j + i]; A[6 * (3 + i) + j] = R[3 * j + i]; }
    double AS[36];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { double s = 0; for (int k = 0; k < 6; ++k) s += A[6 * i + k] * cov6[6 * k + j]; AS[6 * i + j] = s; }
    std::array<double, 36> P{};
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { double s = 0; for (int k = 0; k < 6; ++k) s += AS[6 * i + k] * A[6 * j + k]; P[6 * i + j] = s; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < i; ++j) { const double m = 0.5 * (P[6 * i + j] + P[6 * j + i]); P[6 * i + j] = m; P[6 * j + i] = m; }
    return P;
}

// The marginalization result: last_marginalization_info (linearized_jacobians / residuals, keep_block_*) and
// last_marginalization_parameter_blocks (MarginalizationFactor.h, Estimator.cpp:2584-2606) with blocks named by
// (slot, kind) -- already shifted to the NEXT window's slots.
struct MarginalizationPrior {
    int n = 0;
    std::vector<double> linearized_jacobians, linearized_residuals, keep_block_data;
    std::vector<int32_t> keep_block_slot, keep_block_kind, keep_block_idx;
    glio_prior view() const {
        glio_prior p;
        p.n = n; p.n_blocks = (int32_t)keep_block_slot.size();
        p.lin_jac = linearized_jacobians.data(); p.lin_res = linearized_residuals.data();
        p.blk_slot = keep_block_slot.data(); p.blk_kind = keep_block_kind.data(); p.blk_idx = keep_block_idx.data();
        p.blk_x0 = keep_block_data.data();
        return p;
    }
};

// ---- (1) factor shims ------------------------------------------------------------------------------
// LidarPlaneNormFactor: residual 1, blocks {t[3], q[4]} (LidarKeyframeFactor.h:112-114)
class LidarPlaneNormFactorHip {
public:
    LidarPlaneNormFactorHip(glio_ctx* ctx, const float cp[4], const float plane[4], double score) : ctx_(ctx), score_(score) {
        for (int k = 0; k < 4; ++k) { cp_[k] = cp[k]; plane_[k] = plane[k]; }
    }
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_lidar_plane(ctx_, cp_, plane_, score_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; float cp_[4], plane_[4]; double score_;
};
// ImuFactor: residual 15, blocks {Pi3,Qi4,SBi9,Pj3,Qj4,SBj9} (ImuFactor.h:12)
class ImuFactorHip {
public:
    ImuFactorHip(glio_ctx* ctx, const glio_preint& pre) : ctx_(ctx), pre_(pre) {}
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_imu(ctx_, &pre_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; glio_preint pre_;
};

// ---- (2) the window ----------------------------------------------------------------------------------
// dd_psr_factor_20 (dd_psr_factor.hpp:15-171): 19 residuals, blocks {Pi3, Pj3, yaw1, anc3}
class DdPsrFactorHip {
public:
    DdPsrFactorHip(glio_ctx* ctx, const glio_dd_psr& f) : ctx_(ctx), f_(f) {}
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_dd_psr(ctx_, &f_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; glio_dd_psr f_;
};
// tcdopplerFactor (dopp_factor.hpp:19-85): 1 residual, blocks {Pi3, SBi9, Pj3, SBj9, rcv_ddt[EPOCH_SIZE], yaw1, anc3};
// jacobians[4], when requested, must point to EPOCH_SIZE doubles in Ceres: the shim a maintainer writes zero-fills it and
// stores the single value glio_eval_doppler returns at [epoch]
class DopplerFactorHip {
public:
    DopplerFactorHip(glio_ctx* ctx, const glio_doppler& f) : ctx_(ctx), f_(f) {}
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_doppler(ctx_, &f_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; glio_doppler f_;
};
// MarginalizationFactor (MarginalizationFactor.cpp:223-287): prior->n residuals, one block per kept parameter block
class MarginalizationFactorHip {
public:
    MarginalizationFactorHip(glio_ctx* ctx, const glio_prior* prior) : ctx_(ctx), prior_(prior) {}
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_marginalization(ctx_, prior_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; const glio_prior* prior_;
};
// BinaryLidarPlaneNormFactor (LidarKeyframeFactor.h:124-164): 1 residual, blocks {t1 3, q1 4, t2 3, q2 4}
class BinaryLidarPlaneNormFactorHip {
public:
    BinaryLidarPlaneNormFactorHip(glio_ctx* ctx, const float cp[4], const double norm_cent[6], double score) : ctx_(ctx), score_(score) {
        for (int k = 0; k < 4; ++k) cp_[k] = cp[k];
        for (int k = 0; k < 6; ++k) nc_[k] = norm_cent[k];
    }
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const {
        return glio_eval_binary_plane(ctx_, cp_, nc_, score_, parameters, residuals, jacobians) == GLIO_OK;
    }
private:
    glio_ctx* ctx_; float cp_[4]; double nc_[6]; double score_;
};

// Estimator.cpp:2611-2726: copy the solution back into the estimator's members with the reference's sanity gates.
//   tmpTrans [W][3], tmpQuat [W][4] (w,x,y,z), tmpSpeedBias [W][9], tmp_rcv_dt [W][3] (may be null): the solved blocks
//   Ps / Vs [W][3], Qs [W][4] (the reference keeps Rs as matrices), para_speed_bias [W][9]                : in/out
//   Bas / Bgs [W][3], abs_poses [W][7] (q w,x,y,z then t, :2651-2666), rcv_dt [W][3]                       : out, any may be null
// A component failing its gate keeps its old value (Q14: |dp| < 100, |dq.vec| < 10, |dv| < 100, |db| < 22).  abs_poses takes the
// RAW solved quaternion, Rs the normalised one (:2661-2669).  The six bias gates are chained by dangling `else`s (the
// ROS_WARNs between them are commented out, :2689-2722), so only the FIRST bias component that passes is written (Q16).
// rcv_dt is copied unconditionally (:2645-2647; the blocks carry no residuals, Q6) -- and the reference writes it ONE KEYFRAME EARLIER than
// the other arrays: rcv_dt[i-1] <- tmp_rcv_dt[slot of i] while Ps[i], Vs[i] ... take slot i.  Row s of every array here is window slot s,
// so pass rcv_dt = &rcv_dt[first_idx - 1][0] where the others get &X[first_idx] (host_writeback_test.cpp does).
inline void writeBackState(int W, const double* tmpTrans, const double* tmpQuat, const double* tmpSpeedBias, const double* tmp_rcv_dt,
                           double* Ps, double* Qs, double* Vs, double* para_speed_bias, double* Bas, double* Bgs, double* abs_poses,
                           double* rcv_dt) {
    for (int i = 0; i < W; ++i) {
        const double* t = tmpTrans + 3 * i; const double* q = tmpQuat + 4 * i; const double* sb = tmpSpeedBias + 9 * i;
        double dp = 0, dv = 0;
        for (int k = 0; k < 3; ++k) { dp += (Ps[3 * i + k] - t[k]) * (Ps[3 * i + k] - t[k]); dv += (Vs[3 * i + k] - sb[k]) * (Vs[3 * i + k] - sb[k]); }
        // dq = normalized(tmpQuat)^-1 * Rs ; qnorm = |dq.vec|
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double a[4] = {q[0] / qn, -q[1] / qn, -q[2] / qn, -q[3] / qn};
        const double* b = Qs + 4 * i;
        const double vx = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
        const double vy = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
        const double vz = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
        const double qnorm = std::sqrt(vx * vx + vy * vy + vz * vz);
        if (rcv_dt && tmp_rcv_dt) for (int k = 0; k < 3; ++k) rcv_dt[3 * i + k] = tmp_rcv_dt[3 * i + k];
        if (std::sqrt(dp) < 100) {
            for (int k = 0; k < 3; ++k) { Ps[3 * i + k] = t[k]; if (abs_poses) abs_poses[7 * i + 4 + k] = t[k]; }
        }
        if (qnorm < 10) {
            for (int k = 0; k < 4; ++k) { Qs[4 * i + k] = q[k] / qn; if (abs_poses) abs_poses[7 * i + k] = q[k]; }
        }
        if (std::sqrt(dv) < 100) for (int k = 0; k < 3; ++k) { Vs[3 * i + k] = sb[k]; para_speed_bias[9 * i + k] = sb[k]; }
        for (int k = 3; k < 9; ++k)
            if (std::fabs(para_speed_bias[9 * i + k] - sb[k]) < 22) {          // Q16: the first component that passes, and only that one
                para_speed_bias[9 * i + k] = sb[k];
                if (k < 6) { if (Bas) Bas[3 * i + k - 3] = sb[k]; } else if (Bgs) Bgs[3 * i + k - 6] = sb[k];
                break;
            }
    }
}

// featureSelection (Estimator.cpp:3894-3992), the draws only: which of `count` correspondences of a slot stay.  Returns false when nothing changes
// (count - 1 < feature_res_num: the early return at :3906-3909, quirk Q9 -- the set is kept WHOLE, not cut to feature_res_num); otherwise `kept` holds
// the original indices in draw order: feature_res_num draws.  The reference shuffles geneRandArrayNoRepeat(0, size - 1, rand_set_num)
// (random_generator.hpp:79-93), i.e. the indices 0 .. size - 2 of the `size` records still left, takes element rand_set_num - 1 of the shuffle
// (:3948-3957) and erases that record (:3964-3978): one draw uniform over the first size - 1 records left, whatever rand_set_num is -- the LAST record
// still left is never drawn.  random_select == false empties the slot (:3945 never enters the loop, :3981-3987 install the empty sets).
// The one count where the reference has no defined draw: count = feature_res_num + 1 with rand_set_num > 1 clamps rand_set_num to 0 (:3914-3916),
// the shuffle is never read and selected_id stays -1 (a read before the first record).  This port does not reproduce that: it draws there as for
// every other count (uniform over the first size - 1 records left), so parity is claimed for count > feature_res_num + 1 only.
// rand_below(n): uniform integer in [0, n) -- the reference seeds from std::random_device (random_generator.hpp:58), so the generator is the caller's.
// The Python twin is glio_amd/sliding.py::feature_selection_draws: same generator in, same indices out (tests/test_host_cpp.py).
template <typename RandBelow>
inline bool featureSelectionDraws(int64_t count, int feature_res_num, RandBelow&& rand_below, bool random_select, std::vector<int32_t>& kept) {
    kept.clear();
    if (count < 1 || count - 1 < (int64_t)feature_res_num) return false;
    if (!random_select) return true;
    // the d-th draw picks the k-th record STILL LEFT (k uniform below count - d - 1): its original index is k advanced past every removed index <= it.
    // `gone` stays sorted: O(feature_res_num^2) whatever the count (erasing from a 64k-element list per draw would be O(count) each)
    std::vector<int32_t> gone;
    gone.reserve((size_t)feature_res_num);
    for (int d = 0; d < feature_res_num; ++d) {
        int64_t v = (int64_t)rand_below((uint64_t)(count - d - 1));
        size_t pos = 0;
        while (pos < gone.size() && (int64_t)gone[pos] <= v) { ++v; ++pos; }
        gone.insert(gone.begin() + (std::ptrdiff_t)pos, (int32_t)v);
        kept.push_back((int32_t)v);
    }
    return true;
}

// how the caller's clouds lie in memory: records of stride_bytes, x y z as floats at offset 0, the intensity as a float at intensity_offset
struct PointLayout {
    int stride_bytes, intensity_offset;
    static PointLayout packed() { return {16, 12}; }
    static PointLayout pclXYZI() { return {32, 16}; }        // pcl::PointXYZI, the reference's PointType (GLIO/include/utils/common.h)
};

// buildLocalMapWithLandMark's bookkeeping (Estimator.cpp:3545-3610) without the clouds: what the call does to recent_surf_keyframes when the deque holds
// recent_size clouds, pose_keyframe n_keyframes poses and local_map_width = width.
//   MAP_REBUILD  the deque is thrown away and refilled with `frames` (oldest first) at their CURRENT poses (:3545-3579): whenever recent_size < width.  With
//                n_keyframes > width the loop's guard `i <= size - local_map_width` (:3550) ends it after width - 1 frames, so the deque never reaches `width`
//                again and EVERY later call rebuilds (quirk Q17: the permanent state after the first loop closure, whose correctPoses clears the deque,
//                :4660); with n_keyframes <= width it takes them all.  latest_frame_idx is not touched in this branch.
//   MAP_PUSH     the deque is full: the oldest cloud leaves, keyframe n_keyframes - 1 (= frames[0]) enters at the pose it has now (:3582-3609)
//   MAP_NOTHING  full and no new keyframe since the last push (:3582), or no keyframe yet (:3531-3543: the initial map is the caller's)
// The Python twin is sliding.local_map_plan (tests/test_map_schedule_host_cpu.py).
enum { MAP_NOTHING = 0, MAP_PUSH = 1, MAP_REBUILD = 2 };
struct LocalMapPlan { int action; std::vector<int32_t> frames; int recent_size, latest_frame_idx; };
inline LocalMapPlan localMapPlan(int recent_size, int n_keyframes, int width, int latest_frame_idx) {
    LocalMapPlan p{MAP_NOTHING, {}, recent_size, latest_frame_idx};
    const int n = n_keyframes;
    if (n < 1) return p;
    if (recent_size < width) {
        p.action = MAP_REBUILD;
        for (int i = n - 1; i >= 0; --i) {
            if (n > width && i <= n - width) break;
            p.frames.insert(p.frames.begin(), (int32_t)i);
            if ((int)p.frames.size() >= width) break;
        }
        p.recent_size = (int)p.frames.size();
        return p;
    }
    if (latest_frame_idx != n - 1) { p.action = MAP_PUSH; p.frames.push_back((int32_t)(n - 1)); p.latest_frame_idx = n - 1; }
    return p;
}

class ScanToMapOdometry;          // (3) below: the front end whose surf features setScanFromFrontEnd reads where they lie
class SlidingWindowBackend {
public:
    explicit SlidingWindowBackend(const glio_opts& opts, int device = 0) : opts_(opts), W_(opts.window) {
        check(glio_create(device, &opts_, &ctx_), "glio_create");
        tmpTrans.assign(3 * W_, 0.0); tmpQuat.assign(4 * W_, 0.0); tmpSpeedBias.assign(9 * W_, 0.0);
        for (int i = 0; i < W_; ++i) tmpQuat[4 * i] = 1.0;
    }
    ~SlidingWindowBackend() { glio_destroy(ctx_); }
    SlidingWindowBackend(const SlidingWindowBackend&) = delete;
    SlidingWindowBackend& operator=(const SlidingWindowBackend&) = delete;

    glio_ctx* ctx() const { return ctx_; }
    int window() const { return W_; }

    // Estimator.cpp:2056  kd_tree_surf_local_map->setInputCloud(surf_local_map_ds)
    void setLocalMap(const float* xyzi, int n) { check(glio_set_map(ctx_, xyzi, n), "glio_set_map"); map_points_ = n; }
    // the same straight from cloud->points.data() of a pcl::PointCloud<pcl::PointXYZI> (32-byte records, intensity at byte 16): PointLayout::pclXYZI()
    void setLocalMap(const void* points, int n, PointLayout l) { check(glio_set_map_strided(ctx_, points, n, l.stride_bytes, l.intensity_offset), "glio_set_map_strided"); map_points_ = n; }
    // `if (surf_local_map_ds->points.size() > 50)` (Estimator.cpp:2221,2244): with a smaller map the reference adds NO LiDAR factor
    // for the keyframe ("Not enough feature points from the map")
    bool mapLargeEnough() const { return map_points_ > 50; }
    // Estimator.cpp:2216-2222  Q2 = Q*q_lb^-1, T2 = T - Q2*t_lb, findCorrespondingSurfFeatures(idx-1, Q2, T2)
    int findCorrespondingSurfFeatures(int slot, const float* scan_xyzi, int n) {
        if (!mapLargeEnough()) {
            check(glio_set_scan(ctx_, slot, scan_xyzi, n), "glio_set_scan");
            check(glio_select_correspondences(ctx_, slot, nullptr, 0), "glio_select_correspondences");    // the slot carries no residuals
            return 0;
        }
        double q2[4], t2[3];
        lidarPose(slot, q2, t2);
        int cnt = 0;
        check(glio_associate(ctx_, slot, scan_xyzi, n, q2, t2, &cnt), "glio_associate");
        return cnt;
    }
    // Estimator.cpp:2223  featureSelection(idx-1, Q2_, T2_), right behind the slot's findCorrespondingSurfFeatures: `count` = what the search kept for the
    // slot (findCorrespondingSurfFeatures' return value / windowCounts()[slot]); the gather runs on the device.  Returns the slot's residual count.
    template <typename RandBelow>
    int featureSelection(int slot, int count, int feature_res_num, RandBelow&& rand_below, bool random_select = true) {
        if (!featureSelectionDraws(count, feature_res_num, rand_below, random_select, sel_)) return count;
        check(glio_select_correspondences(ctx_, slot, sel_.empty() ? nullptr : sel_.data(), (int)sel_.size()), "glio_select_correspondences");
        return (int)sel_.size();
    }
    // ... for all W slots of the window at once (the loop of :2198-2248 calls it slot after slot; the draws are made in slot order, exactly as W calls of
    // featureSelection() would make them -- same generator in, same records kept): one upload and two launches instead of W synchronising calls.
    // counts: in = what the searches kept (windowCounts()), out = the residual counts.
    template <typename RandBelow>
    void featureSelectionWindow(std::vector<int32_t>& counts, int feature_res_num, RandBelow&& rand_below, bool random_select = true) {
        std::vector<int32_t> offsets((size_t)W_ + 1, 0), idx;
        std::vector<uint8_t> changed((size_t)W_, 0);
        for (int s = 0; s < W_; ++s) {
            if (featureSelectionDraws(counts[s], feature_res_num, rand_below, random_select, sel_)) { changed[s] = 1; idx.insert(idx.end(), sel_.begin(), sel_.end()); counts[s] = (int32_t)sel_.size(); }
            offsets[s + 1] = (int32_t)idx.size();
        }
        check(glio_select_correspondences_window(ctx_, offsets.data(), idx.empty() ? nullptr : idx.data(), changed.data()), "glio_select_correspondences_window");
    }
    // Estimator.cpp:2182-2192 / 2153-2158 / 2329-2359
    void setImuFactors(const std::vector<glio_preint>& pre) {
        std::vector<int32_t> slots(pre.size());
        for (size_t k = 0; k < pre.size(); ++k) slots[k] = (int32_t)k;
        check(glio_set_imu(ctx_, (int)pre.size(), pre.data(), slots.data()), "glio_set_imu");
    }
    // the same with the edges taken from an ImuStore on the same device: edges[k] links slots k, k + 1 (glio_set_imu_from_store)
    void setImuFactorsFromStore(glio_imu* store, const std::vector<int32_t>& edges) {
        std::vector<int32_t> slots(edges.size());
        for (size_t k = 0; k < edges.size(); ++k) slots[k] = (int32_t)k;
        check(glio_set_imu_from_store(ctx_, store, (int)edges.size(), edges.data(), slots.data()), "glio_set_imu_from_store");
    }
    void setMarginalizationPrior(const glio_prior* prior) { check(glio_set_prior(ctx_, prior), "glio_set_prior"); }
    void setGnss(const glio_gnss_frame* frame, const std::vector<glio_dd_psr>& dd, const std::vector<glio_doppler>& dop) {
        check(glio_set_gnss(ctx_, frame, (int)dd.size(), dd.data(), (int)dop.size(), dop.data()), "glio_set_gnss");
    }

    // correctPoses' `marg = false` (Estimator.cpp:4785; the loop thread then deletes last_marginalization_info, :5264-5267 -- that half is the caller's
    // setMarginalizationPrior(nullptr)).  Armed, the next solve() installs SpeedBiasPriorFactorAutoDiff on tmpSpeedBias[0 .. W-2] as they stand when it is
    // called (:2164-2176), and the marginalization after it re-creates them at the solved state, keeps the blocks of slots 1 .. W-2 in the new prior and
    // disarms (`marg = true`, :2517).  Opt-in: loopClosed() alone does not arm.
    void armSpeedBiasPriors() { sbp_armed_ = true; }
    bool speedBiasPriorsArmed() const { return sbp_armed_; }

    // Estimator.cpp:2424-2433 ceres::Solve + :2439-2457 quaternion sign unification
    glio_summary solve(std::vector<double>* rcv_ddt = nullptr) {
        if (sbp_armed_) check(glio_set_speed_bias_priors(ctx_, W_ - 1, tmpSpeedBias.data()), "glio_set_speed_bias_priors");
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data();
        st.rcv_ddt = rcv_ddt && !rcv_ddt->empty() ? rcv_ddt->data() : nullptr;
        st.n_ddt = rcv_ddt ? (int)rcv_ddt->size() : 0;
        glio_summary sum;
        check(glio_solve(ctx_, &st, &sum), "glio_solve");
        for (int i = 0; i < W_; ++i)
            if (tmpQuat[4 * i] < 0) for (int k = 0; k < 4; ++k) tmpQuat[4 * i + k] = -tmpQuat[4 * i + k];   // unifyQuaternion
        return sum;
    }

    // The marginal covariance of the estimate (include/glio_cov.h) at the state solve() left: the 15 columns of every listed slot, in list order, as a
    // row-major [15 k][15 k] matrix; covarianceColumns: any list of columns of glio_linearize's H.  Call after solve() and before marginalizeAndKeep*(): the
    // marginalization replaces the prior, and with it the H the covariance belongs to.  A column no factor touches reports +inf ("no information"); a matrix
    // that is not positive definite throws.  info (may be null): the call's record.
    std::vector<double> covariance(const std::vector<int32_t>& slots, std::vector<double>* rcv_ddt = nullptr, glio_cov_info* info = nullptr) {
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data();
        st.rcv_ddt = rcv_ddt && !rcv_ddt->empty() ? rcv_ddt->data() : nullptr; st.n_ddt = rcv_ddt ? (int)rcv_ddt->size() : 0;
        const size_t m = 15 * slots.size();
        std::vector<double> out(m * m, 0.0);
        check(glio_covariance_slots(ctx_, &st, (int)slots.size(), slots.data(), out.data(), info), "glio_covariance_slots");
        return out;
    }
    std::vector<double> covarianceColumns(const std::vector<int32_t>& cols, std::vector<double>* rcv_ddt = nullptr, glio_cov_info* info = nullptr) {
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data();
        st.rcv_ddt = rcv_ddt && !rcv_ddt->empty() ? rcv_ddt->data() : nullptr; st.n_ddt = rcv_ddt ? (int)rcv_ddt->size() : 0;
        std::vector<double> out(cols.size() * cols.size(), 0.0);
        check(glio_covariance_columns(ctx_, &st, (int)cols.size(), cols.data(), out.data(), info), "glio_covariance_columns");
        return out;
    }

    // Estimator.cpp:2462-2607: marginalize the oldest keyframe at the solved state (call after solve()); the
    // result is what setMarginalizationPrior() takes for the next window.
    MarginalizationPrior marginalize() {
        int32_t n = 0, nb = 0;          // (6 (W-1) + 9 and 2 (W-1) + 1 but in the windows after a loop closure)
        check(glio_marginalize_size(ctx_, &n, &nb), "glio_marginalize_size");
        MarginalizationPrior m;
        m.linearized_jacobians.assign((size_t)n * n, 0.0); m.linearized_residuals.assign(n, 0.0); m.keep_block_data.assign((size_t)nb * 9, 0.0);
        m.keep_block_slot.assign(nb, 0); m.keep_block_kind.assign(nb, 0); m.keep_block_idx.assign(nb, 0);
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data(); st.rcv_ddt = nullptr; st.n_ddt = 0;
        int32_t on = 0, onb = 0;
        check(glio_marginalize(ctx_, &st, m.linearized_jacobians.data(), m.linearized_residuals.data(), m.keep_block_slot.data(),
                               m.keep_block_kind.data(), m.keep_block_idx.data(), m.keep_block_data.data(), &on, &onb), "glio_marginalize");
        m.n = on;
        disarmSpeedBiasPriors(true);        // (glio_marginalize leaves the context as it found it)
        return m;
    }

    // ---- the same keyframe cycle with everything kept on the device between keyframes (what glio_amd/sliding.py's
    // ResidentSlidingWindow does in Python): only the NEW keyframe's scan crosses PCIe, all W slots are associated in one
    // call, the marginalization result stays on the device as the next window's prior.
    // surf_frames bookkeeping of Estimator.cpp:4240-4300: slot s <- slot s+1 (scans and their correspondences)
    void slideWindow() { check(glio_slide_window(ctx_), "glio_slide_window"); }
    void setScan(int slot, const float* scan_xyzi, int n) { check(glio_set_scan(ctx_, slot, scan_xyzi, n), "glio_set_scan"); }
    void setScan(int slot, const void* points, int n, PointLayout l) { check(glio_set_scan_strided(ctx_, slot, points, n, l.stride_bytes, l.intensity_offset), "glio_set_scan_strided"); }
    // the loop over idx of Estimator.cpp:2216-2222 for the whole window, with the poses held in tmpTrans / tmpQuat
    std::vector<int32_t> findCorrespondingSurfFeaturesWindow() {
        std::vector<double> q2(4 * W_), t2(3 * W_);
        for (int s = 0; s < W_; ++s) lidarPose(s, &q2[4 * s], &t2[3 * s]);
        std::vector<int32_t> counts(W_, 0);
        if (!mapLargeEnough()) {                                    // Estimator.cpp:2221: no LiDAR factors from a map of <= 50 points
            for (int s = 0; s < W_; ++s) check(glio_select_correspondences(ctx_, s, nullptr, 0), "glio_select_correspondences");
            return counts;
        }
        check(glio_associate_window(ctx_, q2.data(), t2.data(), counts.data()), "glio_associate_window");
        return counts;
    }
    // the same without waiting: the searches are enqueued and the call returns -- the caller fills the window's factor tables (setImuFactors, setGnss)
    // while the GPU searches; windowCounts() (or the next solve) waits and returns the per-slot correspondence counts
    void findCorrespondingSurfFeaturesWindowAsync() {
        if (!mapLargeEnough()) {
            for (int s = 0; s < W_; ++s) check(glio_select_correspondences(ctx_, s, nullptr, 0), "glio_select_correspondences");
            return;
        }
        std::vector<double> q2(4 * W_), t2(3 * W_);
        for (int s = 0; s < W_; ++s) lidarPose(s, &q2[4 * s], &t2[3 * s]);
        check(glio_associate_window_async(ctx_, q2.data(), t2.data()), "glio_associate_window_async");
    }
    std::vector<int32_t> windowCounts() {
        std::vector<int32_t> counts(W_, 0);
        if (mapLargeEnough()) check(glio_associate_window_counts(ctx_, counts.data()), "glio_associate_window_counts");
        return counts;
    }
    // the keyframe cloud that setScan() just put into window slot `scan_slot` goes into the local map from device memory (no second upload):
    // body point = scan point - lidar_offset; then the ring map and its search structure are rebuilt
    int pushScanAndBuildLocalMap(int scan_slot, const float lidar_offset[3], const double q[4], const double t[3]) {
        check(glio_localmap_push_scan(ctx_, scan_slot, lidar_offset, q, t), "glio_localmap_push_scan");
        int pts = 0;
        check(glio_localmap_build(ctx_, &pts), "glio_localmap_build");
        map_points_ = pts;
        return pts;
    }
    // Estimator.cpp:2462-2607 with the result kept resident as the prior of the next window (no J0 read-back)
    // (rcv_ddt: the clock-drift slots of the solved state when the window carries Doppler factors -- the state handed over must be the solve's)
    void marginalizeAndKeep(std::vector<double>* rcv_ddt = nullptr) {
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data();
        st.rcv_ddt = rcv_ddt && !rcv_ddt->empty() ? rcv_ddt->data() : nullptr; st.n_ddt = rcv_ddt ? (int)rcv_ddt->size() : 0;
        check(glio_marginalize_keep(ctx_, &st), "glio_marginalize_keep");
        disarmSpeedBiasPriors(false);       // (glio_marginalize_keep removed them from the context)
    }
    // the same in two halves: the marginalization enqueued (the host is free: setScanAhead() of the next keyframe's cloud, say), then waited for
    void marginalizeAndKeepAsync(std::vector<double>* rcv_ddt = nullptr) {
        glio_state st;
        st.trans = tmpTrans.data(); st.quat = tmpQuat.data(); st.speed_bias = tmpSpeedBias.data();
        st.rcv_ddt = rcv_ddt && !rcv_ddt->empty() ? rcv_ddt->data() : nullptr; st.n_ddt = rcv_ddt ? (int)rcv_ddt->size() : 0;
        check(glio_marginalize_keep_async(ctx_, &st), "glio_marginalize_keep_async");
        disarmSpeedBiasPriors(false);
    }
    void marginalizeFinish() { check(glio_marginalize_keep_finish(ctx_), "glio_marginalize_keep_finish"); }
    // the NEXT keyframe's cloud, sent during this keyframe's call (after the solve): the next call's slideWindow() finds it in slot W - 1 and makes no setScan()
    void setScanAhead(const float* scan_xyzi, int n) { check(glio_set_scan_ahead(ctx_, scan_xyzi, n), "glio_set_scan_ahead"); }
    void setScanAhead(const void* points, int n, PointLayout l) { check(glio_set_scan_ahead_strided(ctx_, points, n, l.stride_bytes, l.intensity_offset), "glio_set_scan_ahead_strided"); }

    // ---- the keyframe cloud: LidarOdometry::publishCloudLast's undistortion(surf_features, trans, quat) (LidarOdometry.cpp:180-201, :619-627, only with
    // if_to_deskew) + Estimator::downSampleCloud's ds_filter_surf (Estimator.cpp:3628-3630, surfDSRange) + setScan, on the device.  The cloud is the
    // UNFILTERED surf cloud; deskew_trans = nullptr: if_to_deskew false; deskew_quat = nullptr: the identity (the reference's only call).  Returns the
    // slot's point count (surf_frames[slot]->size()).
    void configureScanFilter(int max_input_points) { check(glio_scan_filter_config(ctx_, max_input_points), "glio_scan_filter_config"); }
    int setScanFiltered(int slot, const float* xyzi, int n, float leaf, const double* deskew_trans = nullptr, const double* deskew_quat = nullptr) {
        int out = 0;
        check(glio_set_scan_filtered(ctx_, slot, xyzi, n, leaf, deskew_trans, deskew_quat, &out), "glio_set_scan_filtered");
        return out;
    }
    int setScanFiltered(int slot, const void* points, int n, PointLayout l, float leaf, const double* deskew_trans = nullptr, const double* deskew_quat = nullptr) {
        int out = 0;
        check(glio_set_scan_filtered_strided(ctx_, slot, points, n, l.stride_bytes, l.intensity_offset, leaf, deskew_trans, deskew_quat, &out), "glio_set_scan_filtered_strided");
        return out;
    }
    // ... into the row that is slot W - 1 after the next slideWindow() (setScanAhead), on the upload stream
    int setScanFilteredAhead(const float* xyzi, int n, float leaf, const double* deskew_trans = nullptr, const double* deskew_quat = nullptr) {
        int out = 0;
        check(glio_set_scan_filtered_ahead(ctx_, xyzi, n, leaf, deskew_trans, deskew_quat, &out), "glio_set_scan_filtered_ahead");
        return out;
    }
    int setScanFilteredAhead(const void* points, int n, PointLayout l, float leaf, const double* deskew_trans = nullptr, const double* deskew_quat = nullptr) {
        int out = 0;
        check(glio_set_scan_filtered_ahead_strided(ctx_, points, n, l.stride_bytes, l.intensity_offset, leaf, deskew_trans, deskew_quat, &out), "glio_set_scan_filtered_ahead_strided");
        return out;
    }
    // the same from the surf features of the front end's last runRaw(), read where they lie on the device.  deskew = true: the reference's call with
    // if_to_deskew -- the translation of the front end's rel_pose, the identity rotation (:620-624).  (Defined behind ScanToMapOdometry.)
    inline int setScanFromFrontEnd(int slot, const ScanToMapOdometry& front_end, float leaf, bool deskew);
    inline int setScanFromFrontEndAhead(const ScanToMapOdometry& front_end, float leaf, bool deskew);
    // what a slot holds, in the caller's order
    std::vector<float> getScan(int slot) {
        int n = 0;
        check(glio_get_scan(ctx_, slot, nullptr, 0, &n), "glio_get_scan");
        std::vector<float> out((size_t)n * 4 + 4);
        check(glio_get_scan(ctx_, slot, out.data(), n, &n), "glio_get_scan");
        out.resize((size_t)n * 4);
        return out;
    }
    // ... and the next call's local map behind it (the cloud just sent ahead pushed at the new keyframe's pose, the ring map and its search structure rebuilt): the
    // next call makes no pushScanAndBuildLocalMap()
    int pushScanAheadAndBuildLocalMap(const float lidar_offset[3], const double q[4], const double t[3]) {
        int pts = 0;
        check(glio_localmap_push_scan_ahead_and_build(ctx_, lidar_offset, q, t, &pts), "glio_localmap_push_scan_ahead_and_build");
        map_points_ = pts;
        return pts;
    }
    // buildLocalMapWithLandMark + downSampleCloud (Estimator.cpp:3529-3631) on the device: push the new keyframe's cloud
    // (body frame) with its pose, rebuild the voxel-averaged ring map and its search structure; returns the map size
    void configureLocalMap(int width, float leaf, int max_points_per_keyframe) {
        check(glio_localmap_config(ctx_, width, leaf, max_points_per_keyframe), "glio_localmap_config");
    }
    int pushKeyframeAndBuildLocalMap(const void* points, int n, PointLayout l, const double q[4], const double t[3]) {
        check(glio_localmap_push_strided(ctx_, points, n, l.stride_bytes, l.intensity_offset, q, t), "glio_localmap_push_strided");
        int pts = 0;
        check(glio_localmap_build(ctx_, &pts), "glio_localmap_build");
        map_points_ = pts;
        return pts;
    }
    int pushKeyframeAndBuildLocalMap(const float* cloud_xyzi, int n, const double q[4], const double t[3]) {
        check(glio_localmap_push(ctx_, cloud_xyzi, n, q, t), "glio_localmap_push");
        int pts = 0;
        check(glio_localmap_build(ctx_, &pts), "glio_localmap_build");
        map_points_ = pts;
        return pts;
    }
    // buildLocalMapWithLandMark's rebuild branch (Estimator.cpp:3545-3579) + downSampleCloud + setInputCloud: the ring becomes the keyframes frame_idx (oldest
    // first) of the clouds resident in a batch association (BatchAssociationBackend::handle()), at poses [n][7] = t, q (q_po * q_bl, q_po * t_bl + t_po)
    int rebuildLocalMapFromFrames(glio_bassoc* frames, const std::vector<int32_t>& frame_idx, const double* poses) {
        int pts = 0;
        check(glio_localmap_rebuild_from_frames(ctx_, frames, (int)frame_idx.size(), frame_idx.data(), poses, &pts), "glio_localmap_rebuild_from_frames");
        map_points_ = pts;
        return pts;
    }
    // ---- the reference's map schedule (opt-in; without it the caller pushes each keyframe once, pushScanAndBuildLocalMap, and never re-poses it): every keyframe
    // call asks localMapPlan and either rebuilds the ring from the resident keyframes at the poses pose_info_keyframe holds NOW or pushes the newest keyframe's
    // resident scan.  loopClosed() is correctPoses' recent_surf_keyframes.clear() (:4660).  The Python twin is sliding.ReferenceMapSchedule.
    void enableReferenceMapSchedule(int local_map_width, const double q_bl[4], const double t_bl[3]) {
        ref_map_ = true; ref_width_ = local_map_width; ref_recent_ = 0; ref_latest_ = -1;
        for (int k = 0; k < 4; ++k) ref_qbl_[k] = q_bl[k];
        for (int k = 0; k < 3; ++k) ref_tbl_[k] = t_bl[k];
    }
    bool referenceMapSchedule() const { return ref_map_; }
    void loopClosed() { ref_recent_ = 0; }
    // a call whose plan says "rebuild" does not use a map built ahead: ask before pushScanAheadAndBuildLocalMap
    bool nextLocalMapCallRebuilds(int n_keyframes) const { return ref_map_ && localMapPlan(ref_recent_, n_keyframes, ref_width_, ref_latest_).action == MAP_REBUILD; }
    // pose_info [>= n_keyframes][7] = t_po, q_po of every keyframe; the newest keyframe's scan is resident in window slot scan_slot and its own-frame cloud in
    // `frames` (setFrameFromScan).  Returns the plan's action; the map size is mapPoints().
    int updateLocalMapByReferenceSchedule(glio_bassoc* frames, int n_keyframes, const double* pose_info, int scan_slot, const float lidar_offset[3]) {
        if (!ref_map_) throw std::runtime_error("updateLocalMapByReferenceSchedule: enableReferenceMapSchedule first");
        const LocalMapPlan p = localMapPlan(ref_recent_, n_keyframes, ref_width_, ref_latest_);
        ref_recent_ = p.recent_size; ref_latest_ = p.latest_frame_idx;
        if (p.action == MAP_NOTHING) return p.action;
        std::vector<double> poses(7 * p.frames.size());
        for (size_t f = 0; f < p.frames.size(); ++f) {
            const double* in = pose_info + 7 * (size_t)p.frames[f];
            const double* q = in + 3; const double* b = ref_qbl_; const double* v = ref_tbl_;
            double* out = &poses[7 * f];
            out[3] = q[0] * b[0] - q[1] * b[1] - q[2] * b[2] - q[3] * b[3];
            out[4] = q[0] * b[1] + q[1] * b[0] + q[2] * b[3] - q[3] * b[2];
            out[5] = q[0] * b[2] + q[2] * b[0] + q[3] * b[1] - q[1] * b[3];
            out[6] = q[0] * b[3] + q[3] * b[0] + q[1] * b[2] - q[2] * b[1];
            double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
            uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
            const double uuv[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
            for (int k = 0; k < 3; ++k) out[k] = (v[k] + q[0] * uv[k] + uuv[k]) + in[k];
        }
        if (p.action == MAP_REBUILD) rebuildLocalMapFromFrames(frames, p.frames, poses.data());
        else pushScanAndBuildLocalMap(scan_slot, lidar_offset, &poses[3], &poses[0]);
        return p.action;
    }
    int mapPoints() const { return map_points_; }
    // shift the host-side state like the reference's slideWindow(): the newest slot is initialised by the caller
    void slideState(const double new_t[3], const double new_q[4], const double new_sb[9]) {
        for (int i = 0; i + 1 < W_; ++i) {
            for (int k = 0; k < 3; ++k) tmpTrans[3 * i + k] = tmpTrans[3 * (i + 1) + k];
            for (int k = 0; k < 4; ++k) tmpQuat[4 * i + k] = tmpQuat[4 * (i + 1) + k];
            for (int k = 0; k < 9; ++k) tmpSpeedBias[9 * i + k] = tmpSpeedBias[9 * (i + 1) + k];
        }
        for (int k = 0; k < 3; ++k) tmpTrans[3 * (W_ - 1) + k] = new_t[k];
        for (int k = 0; k < 4; ++k) tmpQuat[4 * (W_ - 1) + k] = new_q[k];
        for (int k = 0; k < 9; ++k) tmpSpeedBias[9 * (W_ - 1) + k] = new_sb[k];
    }

    // Estimator.cpp:2611-2726 write-back with the reference's sanity gates (writeBackState below, on this backend's tmp arrays)
    void writeBack(double* Ps, double* Qs, double* Vs, double* para_speed_bias, double* Bas = nullptr, double* Bgs = nullptr,
                   double* abs_poses = nullptr, double* rcv_dt = nullptr, const double* tmp_rcv_dt = nullptr) const {
        writeBackState(W_, tmpTrans.data(), tmpQuat.data(), tmpSpeedBias.data(), tmp_rcv_dt, Ps, Qs, Vs, para_speed_bias, Bas, Bgs, abs_poses, rcv_dt);
    }

    // state, laid out like the reference's double arrays
    std::vector<double> tmpTrans, tmpQuat, tmpSpeedBias;

private:
    void lidarPose(int slot, double q2[4], double t2[3]) const {
        const double* q = &tmpQuat[4 * slot]; const double* t = &tmpTrans[3 * slot];
        const double* l = opts_.q_lb;
        const double n2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2] + l[3] * l[3];
        const double li[4] = {l[0] / n2, -l[1] / n2, -l[2] / n2, -l[3] / n2};
        q2[0] = q[0] * li[0] - q[1] * li[1] - q[2] * li[2] - q[3] * li[3];
        q2[1] = q[0] * li[1] + q[1] * li[0] + q[2] * li[3] - q[3] * li[2];
        q2[2] = q[0] * li[2] + q[2] * li[0] + q[3] * li[1] - q[1] * li[3];
        q2[3] = q[0] * li[3] + q[3] * li[0] + q[1] * li[2] - q[2] * li[1];
        // T2 = T - Q2 * t_lb  (Eigen q*v)
        const double* v = opts_.t_lb;
        double uv[3] = {q2[2] * v[2] - q2[3] * v[1], q2[3] * v[0] - q2[1] * v[2], q2[1] * v[1] - q2[2] * v[0]};
        for (double& x : uv) x += x;
        const double uuv[3] = {q2[2] * uv[2] - q2[3] * uv[1], q2[3] * uv[0] - q2[1] * uv[2], q2[1] * uv[1] - q2[2] * uv[0]};
        for (int k = 0; k < 3; ++k) t2[k] = t[k] - (v[k] + q2[0] * uv[k] + uuv[k]);
    }
    glio_opts opts_;
    int W_;
    std::vector<int32_t> sel_;
    int map_points_ = 0;
    bool sbp_armed_ = false;      // armSpeedBiasPriors
    void disarmSpeedBiasPriors(bool clear_context) {
        if (!sbp_armed_) return;
        if (clear_context) check(glio_set_speed_bias_priors(ctx_, 0, nullptr), "glio_set_speed_bias_priors");
        sbp_armed_ = false;
    }
    bool ref_map_ = false; int ref_width_ = 0, ref_recent_ = 0, ref_latest_ = -1; double ref_qbl_[4] = {1, 0, 0, 0}, ref_tbl_[3] = {0, 0, 0};      // enableReferenceMapSchedule
    glio_ctx* ctx_ = nullptr;
};

// qIMU of Preprocessing (GLIO/src/Preprocessing.cpp): imuHandler (:260-292), processIMU (:223-259) with solveRotation (:202-207) and the
// NON-normalised deltaQ of math_tools.h (w = 1, xyz = theta / 2), the NaN guard (:415-417) and the reset after each cloud (:675).  addImu per IMU
// message; forScan(t_scan_next, q) per cloud (t_scan_next: the stamp of the NEXT cloud in the queue, :356-371) gives the q_imu of
// glio_features_extract, or returns false where the reference waits for IMU data (:373-377) and drops the cloud.  The Python twin is
// glio_amd/features.py::ScanRotation (tests/test_host_scan_rotation.py holds the two to each other).
class ScanRotation {
public:
    void addImu(double t, const double gyro[3]) {
        buf_.push_back({{t, gyro[0], gyro[1], gyro[2]}});
        if (current_time_imu_ < 0) current_time_imu_ = t;                          // the first sample's dt is 0
        if (!first_imu_) { first_imu_ = true; gyr0_[0] = gyro[0]; gyr0_[1] = gyro[1]; gyr0_[2] = gyro[2]; }
    }
    bool forScan(double t_scan_next, double q_out[4]) {
        const size_t tmp = idx_imu_ > 0 ? idx_imu_ - 1 : 0;
        if (buf_.empty() || buf_[tmp][0] > t_scan_next) return false;
        if (first_imu_) process(t_scan_next);
        if (std::isnan(q_[0]) || std::isnan(q_[1]) || std::isnan(q_[2]) || std::isnan(q_[3])) { q_[0] = 1; q_[1] = q_[2] = q_[3] = 0; }
        for (int k = 0; k < 4; ++k) q_out[k] = q_[k];
        q_[0] = 1; q_[1] = q_[2] = q_[3] = 0;
        return true;
    }
private:
    void solve(double dt, const double w[3]) {
        double dq[4] = {1.0, 0, 0, 0};
        for (int k = 0; k < 3; ++k) { const double un = 0.5 * (gyr0_[k] + w[k]); const double th = un * dt; dq[1 + k] = th / 2.0; }
        const double a[4] = {q_[0], q_[1], q_[2], q_[3]};
        q_[0] = a[0] * dq[0] - a[1] * dq[1] - a[2] * dq[2] - a[3] * dq[3];
        q_[1] = a[0] * dq[1] + a[1] * dq[0] + a[2] * dq[3] - a[3] * dq[2];
        q_[2] = a[0] * dq[2] + a[2] * dq[0] + a[3] * dq[1] - a[1] * dq[3];
        q_[3] = a[0] * dq[3] + a[3] * dq[0] + a[1] * dq[2] - a[2] * dq[1];
        for (int k = 0; k < 3; ++k) gyr0_[k] = w[k];
    }
    void process(double t_cur) {
        double r[3] = {0, 0, 0};
        size_t i = idx_imu_;
        if (i >= buf_.size()) i--;
        while (buf_[i][0] < t_cur) {
            const double t = buf_[i][0];
            if (current_time_imu_ < 0) current_time_imu_ = t;
            const double dt = t - current_time_imu_;
            current_time_imu_ = buf_[i][0];
            r[0] = buf_[i][1]; r[1] = buf_[i][2]; r[2] = buf_[i][3];
            solve(dt, r);
            i++;
            if (i >= buf_.size()) break;
        }
        if (i < buf_.size()) {                                                      // the interpolated last step at t_cur
            const double dt1 = t_cur - current_time_imu_, dt2 = buf_[i][0] - t_cur;
            const double w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2);
            for (int k = 0; k < 3; ++k) r[k] = w1 * r[k] + w2 * buf_[i][1 + k];
            solve(dt1, r);
        }
        current_time_imu_ = t_cur;
        idx_imu_ = i;
    }
    std::vector<std::array<double, 4>> buf_;
    size_t idx_imu_ = 0;
    double current_time_imu_ = -1;
    double gyr0_[3] = {0, 0, 0};
    double q_[4] = {1, 0, 0, 0};
    bool first_imu_ = false;
};

// ---- raw IMU input ------------------------------------------------------------------------------------
// One push_back(dt, acc, gyr) is a glio_imu_sample.  keyframeImuSamples is the sample preparation of saveKeyFramesAndFactors (Estimator.cpp:4162-4229):
// from the time-stamped IMU buffer (stamps / acc / gyr [n]), the running index idx_imu and cur_time_imu, the list processIMU is called with for the
// keyframe at kf_time -- every sample from idx_imu with a stamp strictly before kf_time (dt against cur_time_imu, 0 for the very first sample; acc clamped
// to +-15 / +-15 / +-18, :4176-4182), up to the buffer's end (the early break, :4194), then the closing sample interpolated between the last one taken and the
// next (w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2), clamped again, :4199-4227), none when the buffer ended.  idx_imu / cur_time_imu are left as the
// reference leaves them (:4243, :4229).  The Python twin is glio_amd/imu.py::keyframe_samples: the same doubles, bit for bit (tests/test_imu_host_cpu.py).
inline double clampImuAcc(double v, double lim) { if (v > lim) v = lim; if (v < -lim) v = -lim; return v; }
inline std::vector<glio_imu_sample> keyframeImuSamples(const std::vector<double>& stamps, const std::vector<std::array<double, 3>>& acc,
                                                       const std::vector<std::array<double, 3>>& gyr, size_t& idx_imu, double& cur_time_imu, double kf_time) {
    static const double lim[3] = {15.0, 15.0, 18.0};
    std::vector<glio_imu_sample> out;
    const size_t n = stamps.size();
    size_t i = idx_imu;
    double d[3] = {0, 0, 0}, r[3] = {0, 0, 0};
    while (i < n && stamps[i] < kf_time) {
        const double t = stamps[i];
        if (cur_time_imu < 0) cur_time_imu = t;
        glio_imu_sample s;
        s.dt = t - cur_time_imu;
        cur_time_imu = t;
        for (int k = 0; k < 3; ++k) { d[k] = clampImuAcc(acc[i][k], lim[k]); r[k] = gyr[i][k]; s.acc[k] = d[k]; s.gyr[k] = r[k]; }
        out.push_back(s);
        i++;
        if (i >= n) break;
    }
    if (i < n) {
        const double dt1 = kf_time - cur_time_imu, dt2 = stamps[i] - kf_time;
        const double w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2);
        glio_imu_sample s;
        s.dt = dt1;
        for (int k = 0; k < 3; ++k) {
            d[k] = clampImuAcc(w1 * d[k] + w2 * acc[i][k], lim[k]);
            r[k] = w1 * r[k] + w2 * gyr[i][k];
            s.acc[k] = d[k]; s.gyr[k] = r[k];
        }
        out.push_back(s);
    }
    cur_time_imu = kf_time;
    idx_imu = i;
    return out;
}
// Rs / Ps / Vs of processIMU (Estimator.cpp:1592-1598) over the samples of one edge, beside the pre-integration (which the store does on the device):
// midpoint propagation in the world frame with deltaQ(un_gyr dt) = (1, un_gyr dt / 2) turned into a matrix by Eigen's toRotationMatrix() without
// normalisation.  R [9] row-major, P, V [3] in/out; acc0 / gyr0 [3] in/out (acc_0 / gyr_0 of the estimator); g = the gravity vector.  ~30 flops per sample,
// and the caller needs the result at once: this stays on the host.  Python twin: imu.propagate_state.
inline void propagateImuState(double R[9], double P[3], double V[3], const double ba[3], const double bg[3], double acc0[3], double gyr0[3],
                              const std::vector<glio_imu_sample>& samples, const double g[3]) {
    for (const glio_imu_sample& s : samples) {
        const double dt = s.dt;
        double e0[3], un0[3], ug[3], e1[3], un1[3];
        for (int k = 0; k < 3; ++k) e0[k] = acc0[k] - ba[k];
        for (int i = 0; i < 3; ++i) un0[i] = R[i * 3 + 0] * e0[0] + R[i * 3 + 1] * e0[1] + R[i * 3 + 2] * e0[2] - g[i];
        for (int k = 0; k < 3; ++k) ug[k] = 0.5 * (gyr0[k] + s.gyr[k]) - bg[k];
        const double qw = 1.0, qx = ug[0] * dt / 2.0, qy = ug[1] * dt / 2.0, qz = ug[2] * dt / 2.0;
        const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
        const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
        const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
        const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
        const double D[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
        double Rn[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = R[i * 3 + 0] * D[0 * 3 + j] + R[i * 3 + 1] * D[1 * 3 + j] + R[i * 3 + 2] * D[2 * 3 + j];
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
        for (int k = 0; k < 3; ++k) e1[k] = s.acc[k] - ba[k];
        for (int i = 0; i < 3; ++i) un1[i] = R[i * 3 + 0] * e1[0] + R[i * 3 + 1] * e1[1] + R[i * 3 + 2] * e1[2] - g[i];
        for (int k = 0; k < 3; ++k) {
            const double un = 0.5 * (un0[k] + un1[k]);
            P[k] = P[k] + (dt * V[k] + 0.5 * dt * dt * un);
            V[k] = V[k] + dt * un;
        }
        for (int k = 0; k < 3; ++k) { acc0[k] = s.acc[k]; gyr0[k] = s.gyr[k]; }
    }
}
// The pre_integrations vector (Estimator.cpp:1582-1600) on the device: processIMU's `new Preintegration(acc_0, gyr_0, Bas.back(), Bgs.back())` + push_back per
// sample become ONE integrate() per keyframe with the list keyframeImuSamples made.  Edges are addressed by index (a ring, if the
// caller wishes); SlidingWindowBackend::setImuFactorsFromStore and BatchBackend::setImuFromStore take them without a trip through the host.
class ImuStore {
public:
    struct Start { double acc0[3], gyr0[3], linearized_ba[3], linearized_bg[3]; };
    ImuStore(int max_edges, int max_samples_per_edge, const glio_imu_noise* noise = nullptr, int device = 0) {
        glio_imu_noise n;
        if (noise) n = *noise; else glio_imu_noise_default(&n);
        check(glio_imu_create(device, max_edges, max_samples_per_edge, &n, &h_), "glio_imu_create");
    }
    ~ImuStore() { glio_imu_destroy(h_); }
    ImuStore(const ImuStore&) = delete;
    ImuStore& operator=(const ImuStore&) = delete;
    glio_imu* handle() const { return h_; }
    // one edge (asynchronous: returns when the samples have been copied)
    void integrate(int edge, const Start& start, const std::vector<glio_imu_sample>& samples) {
        const int32_t off[2] = {0, (int32_t)samples.size()};
        check(glio_imu_integrate(h_, edge, 1, off, samples.empty() ? nullptr : samples.data(), start.acc0), "glio_imu_integrate");
    }
    // edges first_edge .. in one launch: sample_offset [n_edges + 1] into samples, start [n_edges]
    void integrate(int first_edge, const std::vector<int32_t>& sample_offset, const std::vector<glio_imu_sample>& samples, const std::vector<Start>& start) {
        check(glio_imu_integrate(h_, first_edge, (int)start.size(), sample_offset.data(), samples.empty() ? nullptr : samples.data(),
                                 start.empty() ? nullptr : start[0].acc0), "glio_imu_integrate");
    }
    std::vector<glio_preint> read(int first_edge, int n) {
        std::vector<glio_preint> out((size_t)n);
        check(glio_imu_read(h_, first_edge, n, out.data()), "glio_imu_read");
        return out;
    }
    float lastDeviceMs() { float ms = 0; check(glio_imu_last_device_ms(h_, &ms), "glio_imu_last_device_ms"); return ms; }
private:
    glio_imu* h_ = nullptr;
};
static_assert(sizeof(ImuStore::Start) == 12 * sizeof(double), "glio_imu_integrate takes start values as [n][12] doubles");

// ---- the keyframe rule of the front end (LidarOdometry.cpp:566-578, with the initial values of :71-75): which scans are handed over to the window.
//   dis = |t - t_last_kf|, ang = 2 acos((q_last_kf^-1 q).w)                  (a NaN ang -- acos beyond 1 by rounding -- compares false)
//   kf  = ((dis > 0.2 || ang > 0.1) && size - kf_num > 1) || size - kf_num > 2 || size <= 1
// size = pose_cloud_frame->points.size() when the scan is judged: the scans saved BEFORE it (savePoses follows, :682).  A keyframe takes the pose over
// and sets kf_num to the size after savePoses (:684-685).  The initialisation scan (:671-675) is not judged and publishes nothing.
// glio_amd/odometry.py::KeyframeGate is the Python twin (tests/test_keyframe_cloud_abi.py holds the two to each other).
class KeyframeGate {
public:
    bool update(const double q[4], const double t[3], int size) {
        const double d[3] = {t[0] - t_last_[0], t[1] - t_last_[1], t[2] - t_last_[2]};
        const double dis = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        const double n2 = q_last_[0] * q_last_[0] + q_last_[1] * q_last_[1] + q_last_[2] * q_last_[2] + q_last_[3] * q_last_[3];      // inverse(): conjugate / squaredNorm
        const double iw = q_last_[0] / n2, ix = -q_last_[1] / n2, iy = -q_last_[2] / n2, iz = -q_last_[3] / n2;
        const double w = iw * q[0] - ix * q[1] - iy * q[2] - iz * q[3];
        const double ang = 2 * std::acos(w);
        kf_ = ((dis > 0.2 || ang > 0.1) && size - kf_num_ > 1) || size - kf_num_ > 2 || size <= 1;
        if (kf_) {
            for (int k = 0; k < 3; ++k) t_last_[k] = t[k];
            for (int k = 0; k < 4; ++k) q_last_[k] = q[k];
            kf_num_ = size + 1;
        }
        return kf_;
    }
    // after run() / runRaw() of the front end: its abs_pose, judged with the scans saved before this one (false for the initialisation scan)
    inline bool update(const ScanToMapOdometry& front_end);
    bool keyframe() const { return kf_; }
    int keyframeNumber() const { return kf_num_; }
private:
    bool kf_ = true;
    int kf_num_ = 0;
    double t_last_[3] = {0, 0, 0}, q_last_[4] = {1, 0, 0, 0};
};

// ---- (3) the front end -------------------------------------------------------------------------------
// LidarOdometry (GLIO/src/LidarOdometry.cpp): scan-to-map odometry on the same C-ABI with a one-keyframe window.  Per scan, run() (:661-699):
//   poseInitialization (:405-432)  abs_pose <- abs_pose o rel_pose
//   buildLocalMap (:268-292)       the map = the LAST 20 frames' downsampled surf clouds at their solved poses (recent_surf_frames; frame 0 never enters:
//                                  while fewer than 2 poses exist the map is the current scan itself, :271-275) -- here the device-resident ring
//                                  (glio_localmap_config(20, 0.2): one cloud crosses PCIe per scan)
//   downSampleCloud (:306-314)     VoxelGrid 0.2 m over the map (glio_localmap_build); the scan arrives downsampled (surf_last_ds: the caller's filter)
//   updateTransformationWithCeres (:474-581)  match_cnt rounds (8 while fewer than 2 poses exist, else scan_match_cnt, :492-497) of
//                                  [findCorrespondingSurfFeatures at the current abs_pose (:343-404: gates 1.0 / 0.06 / 0.4), one problem of
//                                  LidarPlaneNormIncreFactor under HuberLoss(0.1), Levenberg-Marquardt, max_num_iter, 15 ms budget, unifyQuaternion]
//   savePoses (:316-341), computeRelative (:434-471)  rel_pose <- pose[previous]^-1 o abs_pose
// update() is the solve alone against a map the caller set (kd_tree_surf_last->setInputCloud(surf_from_map_ds), :482).
// The Python twin is glio_amd/odometry.py::ScanToMapOdometry (tests/test_host_cpp.py holds the two to each other bit for bit).
class ScanToMapOdometry {
public:
    struct Round { glio_summary summary; int kept; };
    // glio_opts of the front end: the yaml's `lidar_odometry` block + the constants of LidarOdometry.cpp (odometry.frontend_opts)
    static glio_opts frontendOpts(int max_points, int max_map_points, int max_num_iter = 12) {
        glio_opts o;
        glio_opts_default(&o);
        o.window = 1; o.max_iterations = max_num_iter;                              // config_urban_hk.yaml:19
        o.max_points_per_scan = max_points > 64 ? max_points : 64; o.max_map_points = max_map_points > 64 ? max_map_points : 64; o.max_ddt_epochs = 0;
        o.jacobi_scaling = 1;
        o.kd_max_radius = 1.0; o.surf_dist_thres = 0.06; o.weight_gate = 0.4;       // LidarOdometry.cpp:356,379,392
        o.huber_delta = 0.1; o.doppler_huber_delta = 1.0;                           // :499
        o.q_lb[0] = 1.0; o.q_lb[1] = o.q_lb[2] = o.q_lb[3] = 0.0;
        o.t_lb[0] = o.t_lb[1] = o.t_lb[2] = 0.0;                                    // LidarPlaneNormIncreFactor applies no extrinsic
        o.lidar_const = 7.5;
        o.unit_scores = 1;                                                          // ... and carries no score (LidarKeyframeFactor.h:222-257)
        o.trust_region_strategy = 1;                                                // Ceres default LEVENBERG_MARQUARDT (solverOptions :521-527)
        o.max_solver_time_s = 0.015;                                                // :524
        return o;
    }
    explicit ScanToMapOdometry(const glio_opts& opts, int device = 0, int scan_match_cnt = 1, int local_map_width = 20, float leaf = 0.2f)
        : opts_(opts), scan_match_cnt_(scan_match_cnt) {
        if (opts.window != 1) throw std::invalid_argument("ScanToMapOdometry: the front end is a one-keyframe window");
        check(glio_create(device, &opts_, &ctx_), "glio_create");
        check(glio_localmap_config(ctx_, local_map_width, leaf, opts_.max_points_per_scan), "glio_localmap_config");
        // the window never carries another factor
        check(glio_set_imu(ctx_, 0, nullptr, nullptr), "glio_set_imu");
        check(glio_set_prior(ctx_, nullptr), "glio_set_prior");
        check(glio_set_gnss(ctx_, nullptr, 0, nullptr, 0, nullptr), "glio_set_gnss");
        abs_pose = {{1, 0, 0, 0, 0, 0, 0}}; rel_pose = {{1, 0, 0, 0, 0, 0, 0}};
    }
    ~ScanToMapOdometry() { glio_destroy(ctx_); }
    ScanToMapOdometry(const ScanToMapOdometry&) = delete;
    ScanToMapOdometry& operator=(const ScanToMapOdometry&) = delete;
    glio_ctx* ctx() const { return ctx_; }

    // kd_tree_surf_last->setInputCloud(surf_from_map_ds) (:482) with a map the caller built
    void setMap(const float* xyzi, int n) { check(glio_set_map(ctx_, xyzi, n), "glio_set_map"); map_points_ = n; }
    void setMap(const void* points, int n, PointLayout l) { check(glio_set_map_strided(ctx_, points, n, l.stride_bytes, l.intensity_offset), "glio_set_map_strided"); map_points_ = n; }

    // updateTransformationWithCeres (:474-581) from the given pose (q w,x,y,z then t, the reference's abs_pose[7]); returns the new pose
    std::array<double, 7> update(const float* surf_last_ds, int n, const std::array<double, 7>& pose, int match_cnt, std::vector<Round>* rounds = nullptr) {
        std::array<double, 7> p = pose;
        if (rounds) rounds->clear();
        if (map_points_ < 10) return p;                                             // "Not enough feature points from the map" (:477-480)
        if (surf_last_ds) check(glio_set_scan(ctx_, 0, surf_last_ds, n), "glio_set_scan");      // (null: already resident in slot 0, runRaw)
        double sb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int it = 0; it < match_cnt; ++it) {
            int kept = 0;
            check(glio_associate_resident(ctx_, 0, &p[0], &p[4], &kept), "glio_associate_resident");
            glio_state st;
            st.trans = &p[4]; st.quat = &p[0]; st.speed_bias = sb; st.rcv_ddt = nullptr; st.n_ddt = 0;
            glio_summary sum;
            check(glio_solve(ctx_, &st, &sum), "glio_solve");
            if (p[0] < 0) for (int k = 0; k < 4; ++k) p[k] = -p[k];                 // unifyQuaternion (:532-542)
            if (rounds) rounds->push_back({sum, kept});
        }
        return p;
    }

    // LidarOdometry::run() (:661-699) for one scan; surf_last_ds = the scan after the caller's 0.2 m filter (down_size_filter_surf, :312-313).  Returns abs_pose.
    std::array<double, 7> run(const float* surf_last_ds, int n, std::vector<Round>* rounds = nullptr) {
        if (rounds) rounds->clear();
        if (poses_ == 0) {                                                          // !system_initialized: savePoses(), nothing else (:671-675)
            savePoses(surf_last_ds, n);
            return abs_pose;
        }
        // poseInitialization: t0 = q0 * dt + t0, q0 = q0 * dq
        {
            double t[3], q[4];
            rotate(&abs_pose[0], &rel_pose[4], t);
            for (int k = 0; k < 3; ++k) t[k] += abs_pose[4 + k];
            qmul(&abs_pose[0], &rel_pose[0], q);
            for (int k = 0; k < 4; ++k) abs_pose[k] = q[k];
            for (int k = 0; k < 3; ++k) abs_pose[4 + k] = t[k];
        }
        // buildLocalMap + downSampleCloud
        if (poses_ <= 1) setMap(surf_last_ds, n);                                   // the current scan is its own map (:271-275; the two filters see the same cloud)
        else {
            check(glio_localmap_push(ctx_, last_cloud_.data(), (int)(last_cloud_.size() / 4), &last_pose_[0], &last_pose_[4]), "glio_localmap_push");
            int pts = 0;
            check(glio_localmap_build(ctx_, &pts), "glio_localmap_build");
            map_points_ = pts;
        }
        abs_pose = update(surf_last_ds, n, abs_pose, poses_ < 2 ? 8 : scan_match_cnt_, rounds);
        const std::array<double, 7> prev = last_pose_;
        savePoses(surf_last_ds, n);
        computeRelative(prev);
        return abs_pose;
    }
    // run() from the RAW scan: Preprocessing::cloudHandler on the device (glio_features_extract; the context configured with featuresConfig), then the
    // surf features voxel-filtered at 0.2 m on the device into slot 0 (glio_features_to_scan: down_size_filter_surf, :306-314).  The previous scan is
    // pushed into the 20-frame ring from slot 0 BEFORE the new one overwrites it; then the same update rounds as run() without glio_set_scan.  After
    // the first two scans only counts cross PCIe.  glio_amd/odometry.py::ScanToMapOdometry.run_raw is the Python twin.
    void featuresConfig(const glio_feat_opts& o) { check(glio_features_config(ctx_, &o), "glio_features_config"); }
    std::array<double, 7> runRaw(const void* raw, int n, PointLayout l, const double q_imu[4], std::vector<Round>* rounds = nullptr, glio_feat_counts* counts = nullptr) {
        if (rounds) rounds->clear();
        glio_feat_counts cnt;
        check(glio_features_extract_strided(ctx_, raw, n, l.stride_bytes, l.intensity_offset, q_imu, &cnt), "glio_features_extract_strided");
        if (counts) *counts = cnt;
        const float zero[3] = {0.f, 0.f, 0.f};
        if (poses_ >= 2) check(glio_localmap_push_scan(ctx_, 0, zero, &last_pose_[0], &last_pose_[4]), "glio_localmap_push_scan");
        int ns = 0;
        check(glio_features_to_scan(ctx_, 0, 0.2f, &ns), "glio_features_to_scan");
        if (poses_ == 0) { last_pose_ = abs_pose; ++poses_; return abs_pose; }
        {
            double t[3], q[4];
            rotate(&abs_pose[0], &rel_pose[4], t);
            for (int k = 0; k < 3; ++k) t[k] += abs_pose[4 + k];
            qmul(&abs_pose[0], &rel_pose[0], q);
            for (int k = 0; k < 4; ++k) abs_pose[k] = q[k];
            for (int k = 0; k < 3; ++k) abs_pose[4 + k] = t[k];
        }
        if (poses_ <= 1) {                                                          // the scan is its own map: read back once
            std::vector<float> cloud((size_t)ns * 4 + 4);
            int got = 0;
            check(glio_features_read(ctx_, GLIO_FEAT_LAST_SCAN, cloud.data(), ns, &got), "glio_features_read");
            setMap(cloud.data(), got);
        } else {
            int pts = 0;
            check(glio_localmap_build(ctx_, &pts), "glio_localmap_build");
            map_points_ = pts;
        }
        abs_pose = update(nullptr, ns, abs_pose, poses_ < 2 ? 8 : scan_match_cnt_, rounds);
        const std::array<double, 7> prev = last_pose_;
        last_pose_ = abs_pose;
        ++poses_;
        computeRelative(prev);
        return abs_pose;
    }
    int frames() const { return poses_; }
    int mapPoints() const { return map_points_; }

    std::array<double, 7> abs_pose, rel_pose;          // q (w,x,y,z), t -- the reference's abs_pose[7] / rel_pose[7]

private:
    // computeRelative: rel = prev^-1 o abs
    void computeRelative(const std::array<double, 7>& prev) {
        {
            const double qi[4] = {prev[0], -prev[1], -prev[2], -prev[3]};           // (unit quaternions: the inverse is the conjugate, as Eigen's inverse() of a normalised one)
            const double n2 = prev[0] * prev[0] + prev[1] * prev[1] + prev[2] * prev[2] + prev[3] * prev[3];
            const double qin[4] = {qi[0] / n2, qi[1] / n2, qi[2] / n2, qi[3] / n2};
            double q[4], d[3] = {abs_pose[4] - prev[4], abs_pose[5] - prev[5], abs_pose[6] - prev[6]}, t[3];
            qmul(qin, &abs_pose[0], q);
            rotate(qin, d, t);
            for (int k = 0; k < 4; ++k) rel_pose[k] = q[k];
            for (int k = 0; k < 3; ++k) rel_pose[4 + k] = t[k];
        }
    }
    void savePoses(const float* cloud, int n) {
        last_pose_ = abs_pose;
        last_cloud_.assign(cloud, cloud + 4 * (size_t)n);
        ++poses_;
    }
    static void qmul(const double a[4], const double b[4], double o[4]) {
        o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
        o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
        o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
        o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
    }
    static void rotate(const double q[4], const double v[3], double o[3]) {        // Eigen's q * v: v + 2 w (u x v) + 2 u x (u x v)
        double uv[3] = {q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]};
        for (double& x : uv) x += x;
        const double uuv[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
        for (int k = 0; k < 3; ++k) o[k] = v[k] + q[0] * uv[k] + uuv[k];
    }
    glio_opts opts_;
    int scan_match_cnt_;
    glio_ctx* ctx_ = nullptr;
    int poses_ = 0, map_points_ = 0;
    std::array<double, 7> last_pose_{{1, 0, 0, 0, 0, 0, 0}};
    std::vector<float> last_cloud_;
};

inline bool KeyframeGate::update(const ScanToMapOdometry& fe) {
    const int size = fe.frames() - 1;
    if (size < 1) return false;
    return update(&fe.abs_pose[0], &fe.abs_pose[4], size);
}
inline int SlidingWindowBackend::setScanFromFrontEnd(int slot, const ScanToMapOdometry& fe, float leaf, bool deskew) {
    int out = 0;
    check(glio_set_scan_from_features(ctx_, slot, fe.ctx(), leaf, deskew ? &fe.rel_pose[4] : nullptr, nullptr, &out), "glio_set_scan_from_features");
    return out;
}
inline int SlidingWindowBackend::setScanFromFrontEndAhead(const ScanToMapOdometry& fe, float leaf, bool deskew) {
    int out = 0;
    check(glio_set_scan_from_features_ahead(ctx_, fe.ctx(), leaf, deskew ? &fe.rel_pose[4] : nullptr, nullptr, &out), "glio_set_scan_from_features_ahead");
    return out;
}

}  // namespace glio

"""ctypes mirrors of include/glio_types.h (plain-old-data buffer contracts of the hot path).

Field order and sizes must match the header exactly; tests/test_abi.py checks sizeof() of every
struct against the values the compiled library reports.
"""
import ctypes as C

import numpy as np

GLIO_DD_MAX_SAT = 20
BLK_TRANS, BLK_QUAT, BLK_SPEEDBIAS = 0, 1, 2

TERMINATION = {0: "NO_CONVERGENCE", 1: "FUNCTION_TOLERANCE", 2: "PARAMETER_TOLERANCE",
               3: "GRADIENT_TOLERANCE", 4: "MIN_RADIUS", 5: "FAILURE"}

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)


class GlioOpts(C.Structure):
    _fields_ = [
        ("window", C.c_int32), ("max_iterations", C.c_int32), ("max_points_per_scan", C.c_int32),
        ("max_map_points", C.c_int32), ("max_ddt_epochs", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("huber_delta", C.c_double), ("doppler_huber_delta", C.c_double),
        ("q_lb", C.c_double * 4), ("t_lb", C.c_double * 3),
        ("lidar_const", C.c_double), ("surf_dist_thres", C.c_double),
        ("kd_max_radius", C.c_double), ("weight_gate", C.c_double), ("gravity", C.c_double),
        ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("trust_region_strategy", C.c_int32), ("unit_scores", C.c_int32),
        ("lidar_precision", C.c_int32), ("reserved_", C.c_int32), ("max_solver_time_s", C.c_double),
    ]


class GlioBatchTrOpts(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("use_nonmonotonic_steps", C.c_int32), ("max_consecutive_nonmonotonic_steps", C.c_int32),
                ("jacobi_scaling", C.c_int32), ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double), ("min_relative_decrease", C.c_double), ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("dogleg_type", C.c_int32), ("reserved_", C.c_int32)]


DOGLEG_TRADITIONAL, DOGLEG_SUBSPACE = 0, 1


def batch_tr_opts(max_iterations=100, dogleg=DOGLEG_SUBSPACE):
    """ceres::Solver::Options of the batch solve (Estimator.cpp:3275-3281: DOGLEG, SUBSPACE_DOGLEG, non-monotonic steps; yaml
    max_num_iter: 100) + Ceres 1.14 defaults."""
    o = GlioBatchTrOpts()
    o.dogleg_type = dogleg
    o.max_iterations, o.use_nonmonotonic_steps, o.max_consecutive_nonmonotonic_steps, o.jacobi_scaling = max_iterations, 1, 5, 1
    o.initial_trust_region_radius, o.max_trust_region_radius, o.min_trust_region_radius = 1e4, 1e16, 1e-32
    o.min_relative_decrease, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance = 1e-3, 1e-6, 1e-10, 1e-8
    return o


class GlioState(C.Structure):
    _fields_ = [("trans", c_double_p), ("quat", c_double_p), ("speed_bias", c_double_p),
                ("rcv_ddt", c_double_p), ("n_ddt", C.c_int32)]


class GlioPreint(C.Structure):
    _fields_ = [("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
                ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
                ("sum_dt", C.c_double), ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225)]


class GlioPrior(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_blocks", C.c_int32), ("lin_jac", c_double_p), ("lin_res", c_double_p),
                ("blk_slot", c_int32_p), ("blk_kind", c_int32_p), ("blk_idx", c_int32_p), ("blk_x0", c_double_p)]


class GlioDdPsr(C.Structure):
    _fields_ = [("slot_i", C.c_int32), ("slot_j", C.c_int32), ("n_sat", C.c_int32), ("master", C.c_int32),
                ("ratio", C.c_double), ("threshold", C.c_double), ("station", C.c_double * 3),
                ("user_sat_pos", (C.c_double * 3) * GLIO_DD_MAX_SAT), ("ref_sat_pos", (C.c_double * 3) * GLIO_DD_MAX_SAT),
                ("user_psr", C.c_double * GLIO_DD_MAX_SAT), ("ref_psr", C.c_double * GLIO_DD_MAX_SAT),
                ("weight", C.c_double * ((GLIO_DD_MAX_SAT - 1) ** 2))]


class GlioDoppler(C.Structure):
    _fields_ = [("slot_i", C.c_int32), ("slot_j", C.c_int32), ("epoch", C.c_int32), ("pad_", C.c_int32),
                ("ratio", C.c_double), ("var", C.c_double), ("sat_pos", C.c_double * 3), ("sat_vel", C.c_double * 3),
                ("sv_ddt", C.c_double), ("doppler", C.c_double), ("lamda", C.c_double),
                ("lever_arm", C.c_double * 3), ("R_ecef_local", C.c_double * 9)]


class GlioGnssFrame(C.Structure):
    _fields_ = [("yaw_enu_local", C.c_double), ("anc_ecef", C.c_double * 3)]


class GlioBatchCovInfo(C.Structure):
    """glio_batch_cov_info (include/glio_batch_cov.h)"""
    _fields_ = [("n", C.c_int32), ("B", C.c_int32), ("anchor", C.c_int32), ("bad_keyframe", C.c_int32), ("levels", C.c_int32), ("pad_", C.c_int32),
                ("min_pivot", C.c_double), ("max_pivot", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class GlioSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("termination", C.c_int32),
                ("n_lidar_residuals", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double), ("gradient_max_norm", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["termination_name"] = TERMINATION.get(self.termination, "?")
        return d


class GlioFeatOpts(C.Structure):
    """glio_feat_opts (include/glio_types.h): Preprocessing's parameters"""
    _fields_ = [("n_scans", C.c_int32), ("ds_rate", C.c_int32), ("edge_threshold", C.c_double), ("surf_threshold", C.c_double),
                ("ds_leaf", C.c_float), ("min_range", C.c_float), ("q_lb", C.c_double * 4), ("max_raw_points", C.c_int32),
                ("reserved_", C.c_int32)]


class GlioFeatCounts(C.Structure):
    """glio_feat_counts: point counts of the last extraction"""
    _fields_ = [("in_", C.c_int32), ("kept", C.c_int32), ("cut", C.c_int32), ("sharp", C.c_int32), ("less_sharp", C.c_int32),
                ("flat", C.c_int32), ("surf", C.c_int32), ("reserved_", C.c_int32)]

    def as_dict(self):
        return {"in": self.in_, "kept": self.kept, "cut": self.cut, "sharp": self.sharp, "less_sharp": self.less_sharp, "flat": self.flat, "surf": self.surf}


class GlioImuNoise(C.Structure):
    """glio_imu_noise: acc_n, gyr_n, acc_w, gyr_w of class Preintegration (Preintegration.h:48-51)"""
    _fields_ = [("acc_n", C.c_double), ("gyr_n", C.c_double), ("acc_w", C.c_double), ("gyr_w", C.c_double)]


class GlioImuSample(C.Structure):
    """glio_imu_sample: one push_back(dt, acc, gyr); a [n][7] float64 array has the same bytes"""
    _fields_ = [("dt", C.c_double), ("acc", C.c_double * 3), ("gyr", C.c_double * 3)]


FEAT_SURF, FEAT_EDGE_LESS_SHARP, FEAT_SHARP, FEAT_FLAT, FEAT_CUT_CLOUD, FEAT_LAST_SCAN = range(6)
FEAT_MAX_RAW_POINTS = 400000


class GlioLoopOpts(C.Structure):
    """glio_loop_opts (include/glio_types.h): the submaps' leaf, pcl::IterativeClosestPoint's settings of Estimator.cpp:5197-5200, capacities"""
    _fields_ = [("max_corr_dist", C.c_double), ("transformation_eps", C.c_double), ("fitness_eps", C.c_double), ("abs_mse_eps", C.c_double),
                ("leaf", C.c_float), ("max_iterations", C.c_int32), ("min_correspondences", C.c_int32), ("max_source_points", C.c_int32),
                ("max_target_points", C.c_int32), ("max_frames_per_submap", C.c_int32)]


class GlioLoopResult(C.Structure):
    """glio_loop_result: icp.align + hasConverged + getFitnessScore + getFinalTransformation"""
    _fields_ = [("fitness", C.c_double), ("last_mse", C.c_double), ("transform", C.c_float * 16), ("converged", C.c_int32), ("state", C.c_int32),
                ("iterations", C.c_int32), ("last_n_corr", C.c_int32), ("rank_deficient", C.c_int32), ("reserved_", C.c_int32)]


class GlioLoopStepResult(C.Structure):
    """glio_loop_step_result: one round"""
    _fields_ = [("mse", C.c_double), ("transform", C.c_float * 16), ("n_corr", C.c_int32), ("state", C.c_int32), ("n_fallback", C.c_int32),
                ("rank_deficient", C.c_int32)]


class GlioGmapOpts(C.Structure):
    """glio_gmap_opts (include/glio_types.h): the global map's leaf (Estimator.cpp:856) and capacities"""
    _fields_ = [("leaf", C.c_float), ("max_voxels", C.c_int32), ("max_points_per_add", C.c_int32), ("reserved_", C.c_int32)]


class GlioGmapInfo(C.Structure):
    """glio_gmap_info: what glio_gmap_add_frames reports"""
    _fields_ = [("n_points_total", C.c_int64), ("n_voxels", C.c_int32), ("radix_passes", C.c_int32), ("pcl_index_overflow", C.c_int32), ("reserved_", C.c_int32)]


class GlioPgraphOpts(C.Structure):
    """glio_pgraph_opts (include/glio_types.h): Gauss-Newton's termination, the reference's noise variances (Estimator.cpp:864-865, :1986), capacities"""
    _fields_ = [("relative_error_tol", C.c_double), ("absolute_error_tol", C.c_double), ("prior_var", C.c_double * 6), ("odom_var", C.c_double * 6),
                ("gps_var_floor", C.c_double), ("max_iterations", C.c_int32), ("max_nodes", C.c_int32), ("max_loops", C.c_int32), ("max_unary", C.c_int32),
                ("segment_nodes", C.c_int32), ("reserved_", C.c_int32)]


class GlioPgraphInfo(C.Structure):
    """glio_pgraph_info: what glio_pgraph_solve reports"""
    _fields_ = [("initial_error", C.c_double), ("final_error", C.c_double), ("device_ms", C.c_float), ("stage_ms", C.c_float * 4), ("iterations", C.c_int32),
                ("termination", C.c_int32), ("separators", C.c_int32), ("segments", C.c_int32), ("reserved_", C.c_int32)]


PGRAPH_NOT_RUN, PGRAPH_CONVERGED, PGRAPH_ITERATION_LIMIT, PGRAPH_NONPOSITIVE_PIVOT = range(4)
PGRAPH_TERMINATION_NAMES = ("NOT_RUN", "CONVERGED", "ITERATION_LIMIT", "NONPOSITIVE_PIVOT")
PGRAPH_MIN_RADIUS = 4                   # glio_pgraph_solve_damped alone
PGRAPH_LM_TERMINATION_NAMES = PGRAPH_TERMINATION_NAMES + ("MIN_RADIUS",)


class GlioPgraphLmOpts(C.Structure):
    """glio_pgraph_lm_opts: the damped solve's radius rule (Ceres 1.14's LevenbergMarquardtStrategy defaults)"""
    _fields_ = [("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double), ("min_relative_decrease", C.c_double),
                ("min_diagonal", C.c_double), ("max_diagonal", C.c_double), ("max_trials", C.c_int32), ("reserved_", C.c_int32)]


class GlioPgraphLmInfo(C.Structure):
    """glio_pgraph_lm_info: what glio_pgraph_solve_damped reports beside glio_pgraph_info"""
    _fields_ = [("final_radius", C.c_double), ("accepted", C.c_int32), ("rejected", C.c_int32), ("invalid", C.c_int32), ("trials", C.c_int32)]


class GlioPgraphCovInfo(C.Structure):
    """glio_pgraph_cov_info (include/glio_pgraph_cov.h): the plan glio_pgraph_covariance_all used, the factor's squared diagonal, the node of a failed pivot"""
    _fields_ = [("n_nodes", C.c_int32), ("separators", C.c_int32), ("full_row_separators", C.c_int32), ("segment_nodes", C.c_int32),
                ("bad_node", C.c_int32), ("pad_", C.c_int32), ("min_pivot", C.c_double), ("max_pivot", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


LOOP_SOURCE, LOOP_TARGET = 0, 1
LOOP_NOT_CONVERGED, LOOP_ITERATIONS, LOOP_TRANSFORM, LOOP_ABS_MSE, LOOP_REL_MSE, LOOP_NO_CORRESPONDENCES = range(6)
LOOP_STATE_NAMES = ("NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES")


def dptr(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def fptr(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_float_p)


def iptr(a):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int32_p)


class WindowState:
    """tmpTrans / tmpQuat / tmpSpeedBias / para_rcv_ddt of the reference (Estimator.cpp:345-348,309)."""

    def __init__(self, W, n_ddt=0):
        self.W = W
        self.trans = np.zeros((W, 3))
        self.quat = np.zeros((W, 4))
        self.quat[:, 0] = 1.0
        self.speed_bias = np.zeros((W, 9))
        self.rcv_ddt = np.zeros(max(n_ddt, 1))
        self.n_ddt = n_ddt

    def copy(self):
        s = WindowState(self.W, self.n_ddt)
        s.trans[:] = self.trans
        s.quat[:] = self.quat
        s.speed_bias[:] = self.speed_bias
        s.rcv_ddt = self.rcv_ddt.copy()
        return s

    def c(self):
        return GlioState(dptr(self.trans), dptr(self.quat), dptr(self.speed_bias), dptr(self.rcv_ddt), self.n_ddt)


def preint_array(n):
    return (GlioPreint * max(n, 1))()


# ---- the keyframe cloud (glio_scan_filter_config, glio_set_scan_filtered*, glio_set_scan_from_features*, glio_get_scan): the argument types as
# include/glio_hip.h declares them; capi.load() applies them, so a call with a float where the header has an int fails in Python, not in the library
c_int_p = C.POINTER(C.c_int)
KEYFRAME_CLOUD_PROTOTYPES = {
    "glio_scan_filter_config": [C.c_void_p, C.c_int],
    "glio_set_scan_filtered_strided": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_set_scan_filtered": [C.c_void_p, C.c_int, c_float_p, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_set_scan_filtered_ahead_strided": [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_set_scan_filtered_ahead": [C.c_void_p, c_float_p, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_set_scan_from_features": [C.c_void_p, C.c_int, C.c_void_p, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_set_scan_from_features_ahead": [C.c_void_p, C.c_void_p, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_get_scan": [C.c_void_p, C.c_int, c_float_p, C.c_int, c_int_p],
    "glio_scan_filter_last_device_ms": [C.c_void_p, c_float_p],
}
# ---- the dense store and the global map over it (include/glio_dense.h)
c_void_pp = C.POINTER(C.c_void_p)
DENSE_PROTOTYPES = {
    "glio_dense_create": [C.c_int, C.c_int, C.c_int, C.c_int, c_void_pp],
    "glio_dense_set_frame_strided": [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_dense_set_frame": [C.c_void_p, C.c_int, c_float_p, C.c_int, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_dense_set_frame_from_features": [C.c_void_p, C.c_int, C.c_void_p, C.c_float, c_double_p, c_double_p, c_int_p],
    "glio_dense_read_frame": [C.c_void_p, C.c_int, c_float_p, C.c_int, c_int_p],
    "glio_dense_frame_count": [C.c_void_p, C.c_int, c_int_p],
    "glio_dense_last_device_ms": [C.c_void_p, c_float_p],
    "glio_dense_world_cloud": [C.c_void_p, c_double_p, c_float_p, C.c_int, c_int_p],
    "glio_gmap_create_on_dense": [C.c_void_p, C.c_void_p, c_void_pp],
}


# ---- the GNSS frame estimate (include/glio_align.h)
ALIGN_MAX_ROUNDS, ALIGN_MAX_HYPOTHESES, ALIGN_MAX_ITERATIONS = 8, 4096, 64
ALIGN_OK, ALIGN_WEAK, ALIGN_UNOBSERVABLE = 0, 1, 2
ALIGN_STATUS = {0: "OK", 1: "WEAK", 2: "UNOBSERVABLE"}


class GlioAlignOpts(C.Structure):
    """glio_align_opts"""
    _fields_ = [("n_hypotheses", C.c_int32), ("n_rounds", C.c_int32), ("max_iterations_per_round", C.c_int32), ("reserved_", C.c_int32),
                ("thresholds", C.c_double * ALIGN_MAX_ROUNDS), ("yaw_tolerance", C.c_double), ("pos_tolerance", C.c_double), ("max_yaw_sigma", C.c_double)]


class GlioAlignInfo(C.Structure):
    """glio_align_info"""
    _fields_ = [("status", C.c_int32), ("winner", C.c_int32), ("n_rows", C.c_int32), ("n_rounds", C.c_int32),
                ("round_iterations", C.c_int32 * ALIGN_MAX_ROUNDS), ("round_downweighted", C.c_int32 * ALIGN_MAX_ROUNDS),
                ("coarse_cost", C.c_double), ("runner_up_cost", C.c_double), ("round_cost", C.c_double * ALIGN_MAX_ROUNDS),
                ("yaw_sigma", C.c_double), ("yaw_schur", C.c_double), ("h_yaw_yaw", C.c_double), ("covariance", C.c_double * 16)]

    def as_dict(self):
        n = int(self.n_rounds)
        return dict(status=int(self.status), status_name=ALIGN_STATUS.get(int(self.status), "?"), winner=int(self.winner), n_rows=int(self.n_rows),
                    rounds=[(int(self.round_iterations[k]), float(self.round_cost[k]), int(self.round_downweighted[k])) for k in range(n)],
                    coarse_cost=float(self.coarse_cost), runner_up_cost=float(self.runner_up_cost), yaw_sigma=float(self.yaw_sigma),
                    yaw_schur=float(self.yaw_schur), h_yaw_yaw=float(self.h_yaw_yaw), covariance=np.array(self.covariance[:], float).reshape(4, 4))


ALIGN_PROTOTYPES = {
    "glio_align_struct_sizes": [c_int32_p, C.c_int],
    "glio_align_create": [C.c_int, C.c_int, C.c_int, c_void_pp],
    "glio_align_set_opts": [C.c_void_p, C.POINTER(GlioAlignOpts)],
    "glio_align_set_factors": [C.c_void_p, C.c_int, C.c_void_p],
    "glio_align_set_positions": [C.c_void_p, C.c_int, c_double_p, C.c_int],
    "glio_align_solve": [C.c_void_p, C.POINTER(GlioGnssFrame), C.POINTER(GlioGnssFrame), C.POINTER(GlioAlignInfo)],
    "glio_align_cost": [C.c_void_p, C.POINTER(GlioGnssFrame), C.c_double, c_double_p, c_int32_p],
    "glio_align_read_coarse": [C.c_void_p, c_double_p, C.c_int, c_int32_p],
    "glio_align_last_device_ms": [C.c_void_p, c_float_p],
}


# include/glio_pgraph_cov.h
PGRAPH_COV_PROTOTYPES = {
    "glio_pgraph_cov_struct_sizes": [c_int32_p, C.c_int],
    "glio_pgraph_covariance_all": [C.c_void_p, c_double_p, c_double_p, C.POINTER(GlioPgraphCovInfo)],
    "glio_pgraph_covariance_all_dev": [C.c_void_p, c_void_pp, c_void_pp, c_int_p],
    "glio_pgraph_covariance_all_last_device_ms": [C.c_void_p, c_float_p],
    "glio_pgraph_covariance_all_last_stage_ms": [C.c_void_p, c_float_p],
}


# ---- place recognition (include/glio_place.h)
PLACE_RINGS, PLACE_SECTORS, PLACE_TOP_K_MAX = 20, 60, 8


class GlioPlaceOpts(C.Structure):
    """glio_place_opts"""
    _fields_ = [("max_places", C.c_int32), ("top_k_max", C.c_int32), ("max_radius", C.c_float), ("lidar_height", C.c_float)]


class GlioPlaceMatch(C.Structure):
    """glio_place_match"""
    _fields_ = [("place", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("yaw", C.c_float)]


c_uint64_p = C.POINTER(C.c_uint64)
PLACE_PROTOTYPES = {
    "glio_place_struct_sizes": [c_int32_p, C.c_int],
    "glio_place_tables": [C.c_float, c_float_p, c_float_p],
    "glio_place_create": [C.c_void_p, C.POINTER(GlioPlaceOpts), c_void_pp],
    "glio_place_create_on_dense": [C.c_void_p, C.POINTER(GlioPlaceOpts), c_void_pp],
    "glio_place_add_frames": [C.c_void_p, C.c_int, c_int32_p, c_int32_p, c_double_p, c_double_p],
    "glio_place_read_descriptor": [C.c_void_p, C.c_int, c_float_p, c_uint64_p, c_double_p, c_int32_p],
    "glio_place_set_descriptor": [C.c_void_p, C.c_int, c_float_p, C.c_uint64, C.c_double],
    "glio_place_clear": [C.c_void_p],
    "glio_place_query": [C.c_void_p, C.c_int, C.c_double, C.c_int, C.POINTER(GlioPlaceMatch), c_int32_p],
    "glio_place_query_many": [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(GlioPlaceMatch), c_int32_p],
    "glio_place_last_device_ms": [C.c_void_p, c_float_p],
}


# ---- the static map (include/glio_static.h)
STATIC_MAX_VIEWS, STATIC_PATH_AUTO, STATIC_PATH_GLOBAL, STATIC_LDS_LIMIT = 32, 0, 1, 163840


class GlioStaticOpts(C.Structure):
    """glio_static_opts"""
    _fields_ = [("rows", C.c_int32), ("cols_per_quadrant", C.c_int32), ("neighbourhood", C.c_int32), ("min_votes", C.c_int32), ("max_views", C.c_int32),
                ("image_path", C.c_int32), ("elev_min_deg", C.c_float), ("elev_max_deg", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float),
                ("range_gain", C.c_float), ("range_margin", C.c_float)]


class GlioStaticInfo(C.Structure):
    """glio_static_info"""
    _fields_ = [("n_points", C.c_int64), ("n_tested", C.c_int64), ("n_dynamic", C.c_int64), ("n_frames", C.c_int32), ("lds_path", C.c_int32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


c_uint8_p = C.POINTER(C.c_uint8)
STATIC_PROTOTYPES = {
    "glio_static_struct_sizes": [c_int32_p, C.c_int],
    "glio_static_tables": [C.POINTER(GlioStaticOpts), c_float_p, c_float_p],
    "glio_static_relative_pose": [c_double_p, c_double_p, c_float_p],
    "glio_static_create": [C.c_void_p, C.POINTER(GlioStaticOpts), c_void_pp],
    "glio_static_create_on_dense": [C.c_void_p, C.POINTER(GlioStaticOpts), c_void_pp],
    "glio_static_classify": [C.c_void_p, C.c_int, c_int32_p, c_double_p, c_int32_p, c_int32_p, C.POINTER(GlioStaticInfo)],
    "glio_static_read_frame": [C.c_void_p, C.c_int, c_float_p, C.c_int, c_int_p],
    "glio_static_frame_count": [C.c_void_p, C.c_int, c_int_p],
    "glio_static_read_votes": [C.c_void_p, C.c_int, c_uint8_p, c_uint8_p, C.c_int, c_int_p],
    "glio_static_read_image": [C.c_void_p, C.c_int, c_float_p, c_float_p],
    "glio_static_last_device_ms": [C.c_void_p, c_float_p],
    "glio_gmap_create_on_static": [C.c_void_p, C.c_void_p, c_void_pp],
}


def apply_prototypes(lib):
    for name, args in list(KEYFRAME_CLOUD_PROTOTYPES.items()) + list(DENSE_PROTOTYPES.items()) + list(ALIGN_PROTOTYPES.items()) + list(PGRAPH_COV_PROTOTYPES.items()) + \
            list(PLACE_PROTOTYPES.items()) + list(STATIC_PROTOTYPES.items()):
        fn = getattr(lib, name, None)
        if fn is None:
            raise AttributeError(f"{name} is missing from the library: it is stale, rebuild it with `python -m glio_amd.build`")
        fn.argtypes = args
        fn.restype = C.c_int
    lib.glio_dense_destroy.argtypes = [C.c_void_p]
    lib.glio_dense_destroy.restype = None
    lib.glio_align_destroy.argtypes = [C.c_void_p]
    lib.glio_align_destroy.restype = None
    lib.glio_align_opts_default.argtypes = [C.POINTER(GlioAlignOpts)]
    lib.glio_align_opts_default.restype = None
    lib.glio_place_destroy.argtypes = [C.c_void_p]
    lib.glio_place_destroy.restype = None
    lib.glio_place_opts_default.argtypes = [C.POINTER(GlioPlaceOpts)]
    lib.glio_place_opts_default.restype = None
    lib.glio_static_destroy.argtypes = [C.c_void_p]
    lib.glio_static_destroy.restype = None
    lib.glio_static_opts_default.argtypes = [C.POINTER(GlioStaticOpts)]
    lib.glio_static_opts_default.restype = None

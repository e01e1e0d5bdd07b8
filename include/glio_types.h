/*
 * glio_types.h -- plain-old-data buffer contracts for the GLIO sliding-window hot path.
 *
 * Every struct here restates (in flat C) a buffer that the reference keeps as an Eigen / PCL /
 * ROS-message member of `class Estimator` (reference: GLIO/src/Estimator.cpp) or of one of its
 * factor classes (reference: GLIO/include/factors/).  No HIP, torch or C++ types appear: this header
 * is what a cgo / ctypes / plain-C++ caller sees.  It is shared by the product library
 * (glio_amd/csrc, declared in glio_hip.h) and by the CPU oracle (oracle/glio_oracle.h) so that the
 * parity tests hand *identical bytes* to both sides.
 *
 * Conventions (all taken from the reference, file:line given per field):
 *   - quaternions are (w,x,y,z) doubles               Estimator.cpp:2103-2107
 *   - a keyframe state is T[3], Q[4], SpeedBias[9] = (v, ba, bg)   Estimator.cpp:345-348,2124-2126
 *   - points are PCL `PointXYZI` = 4 x float32 (x,y,z,intensity)   GLIO/include/utils/common.h
 *   - matrices are row-major unless said otherwise (Ceres Jacobian convention,
 *     GraphGNSSLibV1.1/docs/source/nnls_modeling.rst:75-140)
 */
#ifndef GLIO_TYPES_H_
#define GLIO_TYPES_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLIO_POSE_LOCAL 15      /* local (tangent) size of one keyframe: dt3 dtheta3 dv3 dba3 dbg3 */
#define GLIO_DD_MAX_SAT 20      /* dd_psr_factor_20: psr_size_20, dd_psr_factor.hpp:12 */
/* GLIO_MAX_WINDOW sizes the static per-slot tables (and the prior's limits); it is NOT the largest window glio_create accepts.
 * The trust-region step factors the 15 W + max_ddt_epochs unknowns densely inside one workgroup's 160 KiB of LDS, which
 * holds at most GLIO_MAX_UNKNOWNS of them: W <= 61 without clock-drift epochs, in general 15 W + max_ddt_epochs <= 928.
 * glio_create refuses a larger context with GLIO_E_ARG and an error that names the unknown count. */
#define GLIO_MAX_WINDOW 64
#define GLIO_MAX_UNKNOWNS 928
enum { GLIO_STRATEGY_DOGLEG = 0, GLIO_STRATEGY_LM = 1 };

/* Options that shape the hot path.  Defaults (glio_opts_default) are the shipped yaml /
 * hard-coded values: GLIO/config/config_urban_hk.yaml:60-104, Estimator.cpp:70,2424-2430. */
typedef struct glio_opts {
    int32_t window;              /* slide_window_width (yaml:66) -- number of keyframes W */
    int32_t max_iterations;      /* options.max_num_iterations = 15, Estimator.cpp:2427 */
    int32_t max_points_per_scan; /* device capacity per keyframe slot (scan points / correspondences) */
    int32_t max_map_points;      /* device capacity of the local surf map */
    int32_t max_ddt_epochs;      /* number of para_rcv_ddt slots carried as unknowns (<= EPOCH_SIZE 5000) */
    int32_t jacobi_scaling;      /* Ceres default true, nnls_solving.rst:1402-1404 */
    double huber_delta;          /* lossKernel 1.0, Estimator.cpp:70,2092 */
    double doppler_huber_delta;  /* HuberLoss(1.0) on tcdoppler, Estimator.cpp:2335 */
    double q_lb[4];              /* LiDAR->IMU extrinsic rotation (w,x,y,z), yaml:90-93 */
    double t_lb[3];              /* LiDAR->IMU extrinsic translation, yaml:95-97 */
    double lidar_const;          /* yaml:70 */
    double surf_dist_thres;      /* yaml:71 (plane gate) */
    double kd_max_radius;        /* yaml:72 (a double, Estimator.cpp:364) -- compared with the SQUARED float 5th-NN distance, :3651 */
    double weight_gate;          /* 0.3 -- `weight > 0.3` compares the float weight with a double literal, Estimator.cpp:3681 */
    double gravity;              /* IMU/gravity yaml:11 ; g_vec = (0,0,-gravity) Preintegration.h:58 */
    /* trust region (Ceres 1.14 defaults, nnls_solving.rst:1056-1188) */
    double initial_trust_region_radius; /* 1e4 */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_relative_decrease;       /* 1e-3 */
    double function_tolerance;          /* 1e-6 */
    double gradient_tolerance;          /* 1e-10 */
    double parameter_tolerance;         /* 1e-8 */
    /* 0 = DOGLEG (sliding window / batch, Estimator.cpp:2425), 1 = LEVENBERG_MARQUARDT (the Ceres default the
     * front end runs with, LidarOdometry.cpp:521-530) */
    int32_t trust_region_strategy;
    /* 0 = vec_surf_scores = lidar_const * weight (Estimator.cpp:3692); 1 = unit scores: the front end's
     * LidarPlaneNormIncreFactor carries no score (LidarKeyframeFactor.h:222-257) */
    int32_t unit_scores;
    /* arithmetic of the LiDAR plane linearisation (K3).  GLIO_LIDAR_F64 (default): everything in double, 40 B per residual
     * (the reference's Jet<double,7> evaluation).  GLIO_LIDAR_F32_MFMA (BASELINE config C5, the W = 50 x 256 k stress
     * shape): the score travels as a float in the point's 4th component (32 B per residual), the residual is still
     * formed in double, the 1x6 Jacobian in float, and the per-keyframe J^T J / J^T r contraction of each 64-residual
     * chunk runs on the matrix core (v_mfma_f32_16x16x4_f32) with double accumulation across chunks. */
    int32_t lidar_precision;
    int32_t reserved_;
    /* options.max_solver_time_in_seconds (the front end runs with 0.015, LidarOdometry.cpp:524; 0 = no limit, the sliding window's
     * default).  Checked where Ceres checks it -- at the start of an iteration, after the tolerance tests of the previous one: the
     * host's clock raises a flag in mapped memory, the device-resident loop reads it in its state machine and ends the solve with
     * GLIO_TERM_NO_CONVERGENCE at the current (last accepted) point. */
    double max_solver_time_s;
} glio_opts;
enum { GLIO_LIDAR_F64 = 0, GLIO_LIDAR_F32_MFMA = 1 };

/* Window state = the Ceres parameter blocks of the sliding-window problem.
 * Reference: tmpTrans/tmpQuat/tmpSpeedBias (Estimator.cpp:345-348), para_rcv_ddt (:309).
 * All pointers are caller-owned host memory. */
typedef struct glio_state {
    double* trans;       /* [W][3] */
    double* quat;        /* [W][4]  (w,x,y,z) */
    double* speed_bias;  /* [W][9]  (v, ba, bg) */
    double* rcv_ddt;     /* [n_ddt] receiver clock-drift slots touched by Doppler factors (may be NULL) */
    int32_t n_ddt;
} glio_state;

/* One IMU pre-integration between consecutive keyframes: the members of `class Preintegration`
 * (GLIO/include/factors/Preintegration.h:237-256) that ImuFactor::Evaluate reads. */
typedef struct glio_preint {
    double delta_p[3];
    double delta_q[4];        /* (w,x,y,z), normalised by Propagate (Preintegration.h:190) */
    double delta_v[3];
    double linearized_ba[3];
    double linearized_bg[3];
    double sum_dt;
    double jacobian[225];     /* 15x15 row-major, order P,R,V,BA,BG (Preintegration.h:15-21) */
    double covariance[225];   /* 15x15 row-major */
} glio_preint;

/* Kind of a kept parameter block inside the marginalization prior. */
enum { GLIO_BLK_TRANS = 0, GLIO_BLK_QUAT = 1, GLIO_BLK_SPEEDBIAS = 2 };

/* Marginalization prior = `MarginalizationInfo` members read by MarginalizationFactor::Evaluate
 * (GLIO/src/MarginalizationFactor.cpp:233-287): linearized_jacobians (n x n), linearized_residuals
 * (n), keep_block_{size,idx,data}.  Block b refers to window slot blk_slot[b], kind blk_kind[b];
 * its local offset inside the n-vector is blk_idx[b] (= keep_block_idx - m). */
typedef struct glio_prior {
    int32_t n;                /* number of rows/cols (0 = no prior) */
    int32_t n_blocks;
    const double* lin_jac;    /* [n][n] row-major */
    const double* lin_res;    /* [n] */
    const int32_t* blk_slot;  /* [n_blocks] */
    const int32_t* blk_kind;  /* [n_blocks] GLIO_BLK_* */
    const int32_t* blk_idx;   /* [n_blocks] */
    const double* blk_x0;     /* [n_blocks][9] linearisation point (first 3/4/9 entries used) */
} glio_prior;

/* One double-differenced pseudorange factor (dd_psr_factor_20, dd_psr_factor.hpp:15-171).
 * Per-satellite arrays have n_sat entries taken from the user / reference-station GNSS_Raw arrays
 * (nlosExclusion/msg/GNSS_Raw.msg:5-20). */
typedef struct glio_dd_psr {
    int32_t slot_i, slot_j;   /* Pi, Pj parameter blocks (tmpTrans[leftKey], tmpTrans[rightKey]) */
    int32_t n_sat;            /* <= 20 */
    int32_t master;           /* mPrn: index of the master satellite */
    double ratio;             /* ts_ratio */
    double threshold;         /* DDpsrThreshold */
    double station[3];        /* Station_pos (ECEF) */
    double user_sat_pos[GLIO_DD_MAX_SAT][3];  /* gnss_data.GNSS_Raws[i].sat_pos_{x,y,z} */
    double ref_sat_pos[GLIO_DD_MAX_SAT][3];   /* ref_gnss_data.GNSS_Raws[i].sat_pos_{x,y,z} */
    double user_psr[GLIO_DD_MAX_SAT];         /* gnss_data...raw_pseudorange */
    double ref_psr[GLIO_DD_MAX_SAT];          /* ref_gnss_data...raw_pseudorange */
    double weight[(GLIO_DD_MAX_SAT - 1) * (GLIO_DD_MAX_SAT - 1)]; /* DD_W_matrix, row-major (n_sat-1)^2 packed with stride n_sat-1 */
} glio_dd_psr;

/* One tightly-coupled Doppler row (tcdopplerFactor, dopp_factor.hpp:19-85). */
typedef struct glio_doppler {
    int32_t slot_i, slot_j;   /* statePi/stateVi from slot_i, statePj/stateVj from slot_j */
    int32_t epoch;            /* index into glio_state.rcv_ddt */
    int32_t pad_;
    double ratio;             /* ts_ratio */
    double var;               /* residual divided by var (dopp_factor.hpp:72) */
    double sat_pos[3], sat_vel[3];
    double sv_ddt;            /* gnss_data.ddt */
    double doppler, lamda;    /* gnss_data.doppler * gnss_data.lamda */
    double lever_arm[3];      /* lever_arm_T */
    double R_ecef_local[9];   /* row-major, fixed at construction (Estimator.cpp:2326) */
} glio_doppler;

/* Constant GNSS frame blocks: para_yaw_enu_local[1], para_anc_ecef[3] (Estimator.cpp:307-308;
 * SetParameterBlockConstant at :2141,2145). */
typedef struct glio_gnss_frame {
    double yaw_enu_local;
    double anc_ecef[3];
} glio_gnss_frame;

/* Solver summary: the subset of ceres::Solver::Summary the caller can observe. */
typedef struct glio_summary {
    int32_t iterations;           /* step attempts executed (successful + unsuccessful) */
    int32_t successful_steps;
    int32_t termination;          /* GLIO_TERM_* */
    int32_t n_lidar_residuals;
    double initial_cost;
    double final_cost;
    double final_radius;
    double gradient_max_norm;
} glio_summary;

enum {
    GLIO_TERM_NO_CONVERGENCE = 0,   /* hit max_iterations */
    GLIO_TERM_FUNCTION_TOL = 1,
    GLIO_TERM_PARAMETER_TOL = 2,
    GLIO_TERM_GRADIENT_TOL = 3,
    GLIO_TERM_MIN_RADIUS = 4,
    GLIO_TERM_FAILURE = 5
};

/* Trust-region options of the batch solve (ceres::Solver::Options as set at Estimator.cpp:3275-3281: DOGLEG, non-monotonic
 * steps, max_num_iter from the yaml; the rest are Ceres 1.14 defaults).  Shared by libglio_hip (glio_batch_solve_tr) and the oracle. */
typedef struct glio_batch_tr_opts {
    int32_t max_iterations;                      /* options.max_num_iterations = max_num_iter (yaml:65: 100) */
    int32_t use_nonmonotonic_steps;              /* true, Estimator.cpp:3281 */
    int32_t max_consecutive_nonmonotonic_steps;  /* Ceres default 5 */
    int32_t jacobi_scaling;                      /* Ceres default true */
    double initial_trust_region_radius;          /* 1e4 */
    double max_trust_region_radius;              /* 1e16 */
    double min_trust_region_radius;              /* 1e-32 */
    double min_relative_decrease;                /* 1e-3 */
    double function_tolerance;                   /* 1e-6 */
    double gradient_tolerance;                   /* 1e-10 */
    double parameter_tolerance;                  /* 1e-8 */
    int32_t dogleg_type;                         /* GLIO_DOGLEG_SUBSPACE: options.dogleg_type = SUBSPACE_DOGLEG, Estimator.cpp:3278 */
    int32_t reserved_;
} glio_batch_tr_opts;
enum { GLIO_DOGLEG_TRADITIONAL = 0, GLIO_DOGLEG_SUBSPACE = 1 };

/* One scan-to-multiscan constraint of the batch stage (BinaryLidarPlaneNormFactor,
 * LidarKeyframeFactor.h:124-164; built Estimator.cpp:3048,3071). */
typedef struct glio_batch_opts {
    int32_t n_keyframes;
    int32_t band;            /* max |idx - search_idx| (2*search_range at the ends, Estimator.cpp:3009-3017) */
    int32_t max_iterations;
    int32_t pad_;
    double lm_lambda;        /* fixed Levenberg damping used by the restated batch solve */
} glio_batch_opts;

/* LiDAR feature extraction from a raw scan (Preprocessing::cloudHandler, GLIO/src/Preprocessing.cpp:353-681).
 * Defaults (glio_feat_opts_default): config_urban_hk.yaml:14-18,90-93 and the node's members. */
typedef struct glio_feat_opts {
    int32_t n_scans;         /* line_num: 16, 32 or 64 (yaml: 32) */
    int32_t ds_rate;         /* rings with i % ds_rate != 0 are skipped (:542; yaml: 1) */
    double edge_threshold;   /* edgeThreshold (yaml: 1.0), compared as double (:566) */
    double surf_threshold;   /* surfThreshold (yaml: 0.1), compared as double (:607) */
    float ds_leaf;           /* ds_v = 0.4: the member default (:14), never read from the yaml */
    float min_range;         /* removeClosedPointCloud(.., 3.0) (:397), a float threshold squared in float */
    double q_lb[4];          /* ql2b_w/x/y/z (w,x,y,z; yaml: identity) */
    int32_t max_raw_points;  /* capacity of one raw scan: at most 400000, the node's static arrays (:9-12) */
    int32_t reserved_;
} glio_feat_opts;

/* point counts of the last glio_features_extract* */
typedef struct glio_feat_counts {
    int32_t in;              /* raw points handed in */
    int32_t kept;            /* finite and not inside min_range (removeNaNFromPointCloud + removeClosedPointCloud) */
    int32_t cut;             /* with a valid ring: /lidar_cloud_cutted */
    int32_t sharp;           /* cornerPointsSharp */
    int32_t less_sharp;      /* cornerPointsLessSharp: /edge_features */
    int32_t flat;            /* surfPointsFlat */
    int32_t surf;            /* surfPointsLessFlat after the per-ring VoxelGrid: /surf_features */
    int32_t reserved_;
} glio_feat_counts;

/* ---- raw IMU input: the pre_integrations vector on the device (glio_imu_*).
 * The process noise densities of class Preintegration (Preintegration.h:48-51, 64-70); /IMU/acc_n ... of the yaml. */
typedef struct glio_imu_noise {
    double acc_n, gyr_n, acc_w, gyr_w;
} glio_imu_noise;
/* one push_back(dt, acc, gyr) (Preintegration.h:73-78) */
typedef struct glio_imu_sample {
    double dt;
    double acc[3];
    double gyr[3];
} glio_imu_sample;
enum { GLIO_FEAT_SURF = 0, GLIO_FEAT_EDGE_LESS_SHARP = 1, GLIO_FEAT_SHARP = 2, GLIO_FEAT_FLAT = 3, GLIO_FEAT_CUT_CLOUD = 4,
       GLIO_FEAT_LAST_SCAN = 5 /* the cloud the last glio_features_to_scan wrote into its slot */ };
#define GLIO_FEAT_MAX_RAW_POINTS 400000

/* ---- loop closure: the submaps of detectLoopClosure and the pcl::IterativeClosestPoint of performLoopClosure (Estimator.cpp:5101-5273) on the
 * device (glio_loop_*).  Defaults (glio_loop_opts_default): Estimator.cpp:855 (the 0.4 m leaf of ds_filter_surf_map),  :5197-5201
 * (setMaxCorrespondenceDistance(30), setMaximumIterations(100), setTransformationEpsilon(1e-6), setEuclideanFitnessEpsilon(1e-6)) and PCL 1.8.1's
 * DefaultConvergenceCriteria (absolute MSE 1e-12) and min_number_correspondences_ (3). */
typedef struct glio_loop_opts {
    double max_corr_dist;          /* 30: a pair is kept when (double) d2 <= max_corr_dist^2 */
    double transformation_eps;     /* 1e-6 */
    double fitness_eps;            /* 1e-6: the relative MSE threshold (setEuclideanFitnessEpsilon) */
    double abs_mse_eps;            /* 1e-12 */
    float leaf;                    /* 0.4: VoxelGrid leaf of glio_loop_build_submap */
    int32_t max_iterations;        /* 100 */
    int32_t min_correspondences;   /* 3 */
    int32_t max_source_points;     /* capacity of the filtered source submap (65536) */
    int32_t max_target_points;     /* capacity of the filtered target submap (262144) */
    int32_t max_frames_per_submap; /* 64 */
} glio_loop_opts;
enum { GLIO_LOOP_SOURCE = 0, GLIO_LOOP_TARGET = 1 };
/* pcl::registration::DefaultConvergenceCriteria::ConvergenceState, by name */
enum { GLIO_LOOP_NOT_CONVERGED = 0, GLIO_LOOP_ITERATIONS = 1, GLIO_LOOP_TRANSFORM = 2, GLIO_LOOP_ABS_MSE = 3, GLIO_LOOP_REL_MSE = 4,
       GLIO_LOOP_NO_CORRESPONDENCES = 5 };
/* icp.align + hasConverged + getFitnessScore + getFinalTransformation */
typedef struct glio_loop_result {
    double fitness;                /* mean squared 1-NN distance of the final source to the target, no distance cap */
    double last_mse;               /* mean squared distance of the last round's kept pairs */
    float transform[16];           /* row major Matrix4f */
    int32_t converged;
    int32_t state;                 /* GLIO_LOOP_* */
    int32_t iterations;
    int32_t last_n_corr;
    int32_t rank_deficient;        /* 1: the last round's pairs were collinear (or one point); the transform of the rounds before is kept */
    int32_t reserved_;
} glio_loop_result;
/* one round (glio_loop_step) */
typedef struct glio_loop_step_result {
    double mse;
    float transform[16];           /* the round's incremental transform, row major */
    int32_t n_corr;
    int32_t state;                 /* what the convergence test of this round says (GLIO_LOOP_NOT_CONVERGED: go on) */
    int32_t n_fallback;            /* queries of this round's search that the grid could not certify and the brute-force scan answered */
    int32_t rank_deficient;
} glio_loop_step_result;

/* ---- the global map: mapVisualizationThread's save_pcd part and publishCompleteMap (Estimator.cpp:5315-5350, :5275-5313) on the device (glio_gmap_*).
 * Default leaf (glio_gmap_opts_default): ds_filter_global_map.setLeafSize(0.2 ...), Estimator.cpp:856. */
typedef struct glio_gmap_opts {
    float leaf;                    /* 0.2 */
    int32_t max_voxels;            /* capacity of the map (4194304); two voxel arrays of 44 B per voxel are held */
    int32_t max_points_per_add;    /* points one glio_gmap_add_frames may bring (4194304); 44 B of workspace per point */
    int32_t reserved_;
} glio_gmap_opts;
/* what glio_gmap_add_frames reports */
typedef struct glio_gmap_info {
    int64_t n_points_total;        /* points added since the last clear */
    int32_t n_voxels;              /* the map's size */
    int32_t radix_passes;          /* passes this call's sort ran: 8-bit digits of the call's voxel coordinates counted from the call's own minimum and packed
                                    * without gaps, ceil((bits(extent x) + bits(extent y) + bits(extent z)) / 8); 0 when every point falls into one voxel */
    int32_t pcl_index_overflow;    /* 1: the bounding box of everything added since the last clear holds more than INT32_MAX cells.  PCL 1.8.1's VoxelGrid then
                                    * warns and passes the cloud through UNFILTERED (Estimator.cpp:5343 would save the raw concatenation); this library still filters,
                                    * with a 64-bit index -- a stated deviation, reported here */
    int32_t reserved_;
} glio_gmap_info;

/* ---- the pose graph: the global graph of Estimator.cpp:4586-4652, 5251-5256 and the local graph of :4561-4581, 1915-2043 on the device (glio_pgraph_*).
 * GTSAM is not part of the reference tree: everything GTSAM-side is UNPINNED, restated from its published behaviour (include/glio_hip.h).
 * Defaults (glio_pgraph_opts_default): prior_noise and odom_noise of Estimator.cpp:864-865 (variances, rotation first), max(noise, 1) of :1986,
 * gtsam::GaussNewtonParams' published defaults (100 iterations, relative and absolute error tolerance 1e-5). */
typedef struct glio_pgraph_opts {
    double relative_error_tol;     /* 1e-5 */
    double absolute_error_tol;     /* 1e-5 */
    double prior_var[6];           /* 1e-2, 1e-2, pi^2, 1e8, 1e8, 1e8: what a null var of glio_pgraph_set_prior means */
    double odom_var[6];            /* 1e-6 x3, 1e-4 x3: what a null var of glio_pgraph_append means */
    double gps_var_floor;          /* 1: every GPS variance is max(var, gps_var_floor) */
    int32_t max_iterations;        /* 100 */
    int32_t max_nodes;             /* 65536 */
    int32_t max_loops;             /* 64 (at most 1024) */
    int32_t max_unary;             /* 4096: GPS factors */
    int32_t segment_nodes;         /* interior nodes per segment of the elimination; 0 = chosen by the library (about sqrt(nodes), 4 .. 255) */
    int32_t reserved_;
} glio_pgraph_opts;
enum { GLIO_PGRAPH_NOT_RUN = 0, GLIO_PGRAPH_CONVERGED = 1, GLIO_PGRAPH_ITERATION_LIMIT = 2, GLIO_PGRAPH_NONPOSITIVE_PIVOT = 3 };
/* what glio_pgraph_solve reports */
typedef struct glio_pgraph_info {
    double initial_error;          /* 1/2 |r|^2 at the estimate the solve started from */
    double final_error;            /* ... at the estimate it left */
    float device_ms;               /* the whole solve */
    float stage_ms[4];             /* the FIRST iteration by stage: linearise, segments, separator system, back-substitution + update */
    int32_t iterations;
    int32_t termination;           /* GLIO_PGRAPH_* */
    int32_t separators;
    int32_t segments;
    int32_t reserved_;
} glio_pgraph_info;
/* a termination of glio_pgraph_solve_damped alone (appended: the four values above keep their numbers) */
enum { GLIO_PGRAPH_MIN_RADIUS = 4 };
/* ---- the damped solve (glio_pgraph_solve_damped, include/glio_pgraph_lm.h): Ceres 1.14's LevenbergMarquardtStrategy and its monotonic trust-region loop on the
 * pose graph's own normal equations (UNPINNED like everything Ceres- or GTSAM-side; the rule is restated in include/glio_pgraph_lm.h).  Defaults
 * (glio_pgraph_lm_opts_default) are Ceres' published ones. */
typedef struct glio_pgraph_lm_opts {
    double initial_radius;         /* 1e4: every solve starts from it */
    double max_radius;             /* 1e16 */
    double min_radius;             /* 1e-32: a radius at or below it ends the solve MIN_RADIUS */
    double min_relative_decrease;  /* 1e-3: a trial is accepted when (E - E_candidate) / model decrease exceeds it; in [0, 1) */
    double min_diagonal;           /* 1e-6: the damping is clamp(H_ii, min_diagonal, max_diagonal) / radius */
    double max_diagonal;           /* 1e32 */
    int32_t max_trials;            /* 0 = glio_pgraph_opts.max_iterations; accepted, rejected and invalid trials all count */
    int32_t reserved_;
} glio_pgraph_lm_opts;
/* what glio_pgraph_solve_damped reports beside glio_pgraph_info */
typedef struct glio_pgraph_lm_info {
    double final_radius;
    int32_t accepted, rejected, invalid, trials;     /* rejected counts the invalid trials too: trials = accepted + rejected */
} glio_pgraph_lm_info;

#ifdef __cplusplus
}
#endif
#endif /* GLIO_TYPES_H_ */

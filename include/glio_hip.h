/*
 * glio_hip.h -- C-ABI of libglio_hip.so: the MI355X (gfx950) implementation of GLIO's
 * sliding-window hot path, Estimator::optimizeSlidingWindowWithLandMark
 * (reference: GLIO/src/Estimator.cpp:2046-2736).
 *
 * This is the drop-in boundary.  The reference has no plugin API; what it has are
 * (a) the Estimator member buffers the function reads and writes, and (b) the
 * ceres::CostFunction::Evaluate(double const* const*, double*, double**) contract of every factor.
 * Each entry point below names the reference interface it replaces.  Signatures carry plain
 * pointers and sizes only; every pointer is caller-owned HOST memory unless the name ends in
 * `_dev`.  All functions return 0 on success, a negative GLIO_E_* code otherwise; nothing throws.
 * A context owns one HIP stream and is not thread-safe; independent contexts (sliding window vs
 * batch thread, Estimator.cpp:5398-5404) may be used concurrently.
 */
#ifndef GLIO_HIP_H_
#define GLIO_HIP_H_

#include "glio_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GLIO_OK = 0,
    GLIO_E_ARG = -1,        /* bad argument / capacity exceeded */
    GLIO_E_HIP = -2,        /* HIP runtime error (no device, launch failure ...) */
    GLIO_E_STATE = -3,      /* call order violated (e.g. solve before any factor was set) */
    GLIO_E_NUMERIC = -4     /* solver failure (Cholesky breakdown with mu >= 1) */
};

typedef struct glio_ctx glio_ctx;

/* Library / device info.  `glio_device_count` < 1 means the HIP path is unusable: callers must fail. */
int glio_abi_version(void);
int glio_device_count(void);
const char* glio_last_error(void);
/* sizeof() of every POD struct, in the order opts,state,preint,prior,dd_psr,doppler,gnss_frame,summary,batch_tr_opts
 * (lets a foreign-language binding verify its struct layout); returns how many there are. */
int glio_struct_sizes(int32_t* out, int n);

/* yaml defaults: GLIO/config/config_urban_hk.yaml:60-104 + Estimator.cpp:70,2424-2430 */
void glio_opts_default(glio_opts* o);

/* Replaces: construction of the per-window Ceres problem + device residency of Estimator members. */
int glio_create(int device, const glio_opts* opts, glio_ctx** out);
void glio_destroy(glio_ctx* ctx);
/* Optional: run on a caller-provided hipStream_t (e.g. torch's current stream). NULL restores the own stream. */
int glio_set_stream(glio_ctx* ctx, void* hip_stream);
int glio_synchronize(glio_ctx* ctx);

/* ---- K1: local map.  Replaces kd_tree_surf_local_map->setInputCloud(surf_local_map_ds)
 * (Estimator.cpp:2056).  pts = PointXYZI[n] as 4 floats; builds the voxel hash on device. */
int glio_set_map(glio_ctx* ctx, const float* map_xyzi, int n);
/* ---- strided point input.  The reference hands its clouds around as pcl::PointCloud<PointType>, PointType = pcl::PointXYZI (GLIO/include/utils/common.h):
 * records of 32 bytes, x y z as floats at bytes 0-11, the intensity at byte 16.  Every cloud-taking entry point has a *_strided twin that takes
 * cloud->points.data() as it is: stride_bytes per record (>= 16, a multiple of 4), x y z at offset 0, intensity_offset in [12, stride - 4].  The raw
 * records travel in ONE copy and are unpacked on the device -- no packing pass over the scan / the map on the host.  (stride 16, offset 12 = the packed
 * float4 form the plain entry points take.)  Replaces the cloud hand-over of Estimator.cpp:2056 (map), :2198-2248 (scans), :3529-3631 (local map). */
int glio_set_map_strided(glio_ctx* ctx, const void* map_points, int n, int stride_bytes, int intensity_offset);

/* ---- device-resident local map.  Replaces buildLocalMapWithLandMark + downSampleCloud + setInputCloud
 * (Estimator.cpp:3529-3631, 2056) by a ring of the last `width` keyframe clouds kept on the device in the map frame:
 * per keyframe ONE scan crosses PCIe (glio_localmap_push), the concatenation is voxel-averaged (pcl::VoxelGrid
 * semantics, leaf = surf_ds_size) and hashed on the device (glio_localmap_build does what glio_set_map does).
 *   width = local_map_width (yaml: 50); q,t = q_po * q_bl, q_po * t_bl + t_po (:3569-3570).
 * A push is the reference's steady-state branch (:3580-3610: pop the oldest, append the newest at the pose it has now); the branch that re-poses the whole
 * deque (:3545-3579) is glio_localmap_rebuild_from_frames below. */
int glio_localmap_config(glio_ctx* ctx, int width, float leaf, int max_points_per_keyframe);
int glio_localmap_push(glio_ctx* ctx, const float* cloud_xyzi, int n, const double q[4], const double t[3]);
int glio_localmap_push_strided(glio_ctx* ctx, const void* cloud_points, int n, int stride_bytes, int intensity_offset, const double q[4], const double t[3]);
/* the same from the scan glio_set_scan already put into window slot `scan_slot` (LiDAR frame; body point = scan point - lidar_offset in float):
 * the newest keyframe's cloud crosses PCIe once for both the association and the map */
int glio_localmap_push_scan(glio_ctx* ctx, int scan_slot, const float lidar_offset[3], const double q[4], const double t[3]);
/* Voxel grid + hash of the ring's content; *out_points = the map's size.  The call waits ONCE in its middle (the voxel count sizes the rest) and returns with
 * the ordered output and the hash build still running on the context's stream: the searches are ordered behind them, glio_localmap_read waits.
 * GLIO_E_ARG when the ring holds more voxels than opts.max_map_points or its voxel table overflows: the ring stays as the pushes made it and the previous map
 * stays installed; the next build reconstructs the table from the ring and succeeds as soon as the ring fits (the offending keyframe evicted).  A ring that
 * holds no point gives a map of 0 points: no error, and an association against it keeps 0 correspondences. */
int glio_localmap_build(glio_ctx* ctx, int* out_points);
/* centroid arithmetic of the voxel grid: 0 (default) exact fixed-point sums; 1 = float sums in the order of the concatenated cloud, as the oracle's
 * restatement of pcl::VoxelGrid forms them (Estimator.cpp:3618-3631 through PCL): bit-identical to the ORACLE's map (stable order inside a voxel).  PCL itself
 * orders its point / voxel index vector with an unstable sort, so against a real PCL build the float sums may differ by an ulp -- the order inside a voxel is
 * not specified by PCL.  One extra pass over the ring per build.  The mode survives glio_localmap_config (re-applied to the new ring). */
int glio_localmap_set_accumulation(glio_ctx* ctx, int mode);
/* test hook: the down-sampled map (surf_local_map_ds), ordered by voxel index */
int glio_localmap_read(glio_ctx* ctx, float* out_xyzi, int capacity, int* out_n);

/* ---- K2: correspondences.  Replaces findCorrespondingSurfFeatures(idx, Q2, T2)
 * (Estimator.cpp:3633-3708) for window slot `slot`: uploads the scan (surf_frames[idx], PointXYZI[n],
 * LiDAR frame), runs exact 5-NN + plane fit + gates on device and leaves the compacted
 * vec_surf_cur_pts / vec_surf_normal / vec_surf_scores of that slot resident.  q,t = the LiDAR pose
 * Q2,T2 of Estimator.cpp:2216-2217.  *out_count receives vec_surf_res_cnt[slot]. */
int glio_associate(glio_ctx* ctx, int slot, const float* scan_xyzi, int n, const double q[4],
                   const double t[3], int* out_count);
/* Same, for a scan already resident from a previous glio_associate/glio_set_scan (re-association).
 * glio_set_scan returns when the caller's buffer has been read; the presort of the scan is enqueued behind the copy and not waited for. */
int glio_set_scan(glio_ctx* ctx, int slot, const float* scan_xyzi, int n);
int glio_set_scan_strided(glio_ctx* ctx, int slot, const void* scan_points, int n, int stride_bytes, int intensity_offset);
/* The NEXT keyframe's scan, sent while the current keyframe's call is still running (the reference hands surf_frames over from the front end before
 * optimizeSlidingWindowWithLandMark runs, Estimator.cpp:5372ff): it goes into the ring row that becomes slot W - 1 with the next glio_slide_window -- the row of
 * the CURRENT slot 0, whose scan is gone afterwards (no re-association of slot 0) -- on a stream of its own, beside the call's kernels, the presort behind it.
 * To be called once the window's association is through (after glio_associate_window_counts / the solve).  The next glio_slide_window takes the scan over; that
 * call then makes no glio_set_scan for slot W - 1.  Returns when the caller's buffer has been read. */
int glio_set_scan_ahead(glio_ctx* ctx, const float* scan_xyzi, int n);
int glio_set_scan_ahead_strided(glio_ctx* ctx, const void* scan_points, int n, int stride_bytes, int intensity_offset);
/* ... and, behind it, the next call's local map: glio_localmap_push_scan of the cloud just sent ahead at the new keyframe's pose + glio_localmap_build, on the same
 * stream beside the call's tail (the new keyframe's initial pose follows from this call's solve and the odometry: in its steady state -- the deque full,
 * Estimator.cpp:3580-3610 -- buildLocalMapWithLandMark pushes each keyframe once, at the pose it has when it arrives; the rebuild branch, :3545-3579, is
 * glio_localmap_rebuild_from_frames).  The next call then makes neither call; its glio_slide_window waits for the event. */
int glio_localmap_push_scan_ahead_and_build(glio_ctx* ctx, const float lidar_offset[3], const double q[4], const double t[3], int* out_points);
int glio_associate_resident(glio_ctx* ctx, int slot, const double q[4], const double t[3], int* out_count);
/* Slide the window by one keyframe: the resident scan of slot s+1 becomes that of slot s (the scans are a ring on the device: nothing is
 * copied, nothing waited for); slot W-1 is free for the new keyframe's glio_set_scan.  (surf_frames / keyframe_idx bookkeeping of
 * Estimator.cpp:4240-4300.) */
int glio_slide_window(glio_ctx* ctx);
/* The whole loop of Estimator.cpp:2198-2248 in one call: every slot's resident scan against the map with its own
 * LiDAR pose (quats [W][4], trans [W][3] = Q2, T2 per slot), one host synchronisation; out_counts [W]. */
int glio_associate_window(glio_ctx* ctx, const double* quats, const double* trans, int32_t* out_counts);
/* the same in two halves: _async enqueues the searches and returns (the host is free for glio_set_imu / glio_set_gnss while the GPU searches);
 * _counts waits and returns the per-slot counts (optional: every entry point that needs the correspondences waits by itself) */
int glio_associate_window_async(glio_ctx* ctx, const double* quats, const double* trans);
int glio_associate_window_counts(glio_ctx* ctx, int32_t* out_counts);
/* featureSelection (Estimator.cpp:3894-3992): keep records indices[0..n) of the slot, in that order (n = 0 empties the
 * slot, the reference's random_select == false case :3945,3981-3987).  The random draws stay with the caller (the
 * reference seeds from std::random_device, random_generator.hpp:58, so they are not reproducible anyway); the gather
 * runs on the device, nothing is read back.  glio_amd/sliding.py::feature_selection restates the draw procedure. */
int glio_select_correspondences(glio_ctx* ctx, int slot, const int32_t* indices, int n);
/* The same for every slot of the window in ONE call -- what the released configuration does in every keyframe call (featureSelection behind each slot's
 * search, Estimator.cpp:2222-2223; feature_res_num 100 of ~4 k records per slot): slot s keeps records indices[offsets[s] .. offsets[s+1]) of its own set, in
 * that order (offsets[0] = 0, W + 1 entries); changed[s] == 0 leaves slot s untouched (the early return of :3906-3909), changed == NULL changes all.  One
 * upload, two launches, no host wait: the solve that follows on the context is ordered behind it. */
int glio_select_correspondences_window(glio_ctx* ctx, const int32_t* offsets, const int32_t* indices, const uint8_t* changed);
/* Parity hook / featureSelection replacement: provide or read back a slot's correspondence arrays. */
int glio_set_correspondences(glio_ctx* ctx, int slot, const float* pts_xyzi, const float* planes,
                             const double* scores, int n);
int glio_get_correspondences(glio_ctx* ctx, int slot, float* pts_xyzi, float* planes, double* scores,
                             int capacity, int* out_count);

/* ---- factors of the window problem
 * glio_set_imu / glio_set_gnss may be called while the window's searches run (glio_associate_window_async): their tables travel as one pinned block
 * on a stream of the library's own into a device mirror, the call waits for that copy alone, and the kernel that installs the tables is enqueued on
 * the context's stream behind everything that still reads the old ones.  (GLIO_EARLY_UPLOAD=0 in the environment: copy and wait on the context's
 * stream, for A/B runs.) */
/* Replaces problem.AddResidualBlock(new ImuFactor(pre_integrations[idx+1]), NULL, ...)
 * (Estimator.cpp:2182-2192).  Edge `k` links slots slot_i and slot_i+1. */
int glio_set_imu(glio_ctx* ctx, int n_edges, const glio_preint* edges, const int32_t* slot_i);
/* Replaces problem.AddResidualBlock(new MarginalizationFactor(last_marginalization_info), NULL,
 * last_marginalization_parameter_blocks) (Estimator.cpp:2153-2158).  prior->n == 0 removes it. */
int glio_set_prior(glio_ctx* ctx, const glio_prior* prior);
/* Limits of a prior in a window of W keyframes: n <= max(6 W + 9, 15 (W-1)) columns in n_blocks <= max(2 W + 1, 3 (W-1)) blocks, and n <= 393 whatever W
 * (the prior's kernels keep three vectors of that length in LDS): windows of up to 27 keyframes hold every layout glio_marginalize can produce. */
/* Replaces the SpeedBiasPriorFactorAutoDiff blocks of the window after a loop closure (correctPoses ends with marg = false, Estimator.cpp:4785; the
 * factors: Estimator.cpp:2164-2176, PriorFactor.h:10-40): residual w o (x - target) on the speed/bias of slots 0 .. n_slots-1, w = (8, 8, 1, ..., 1), no
 * loss.  target: [n_slots][9], copied.  n_slots <= W-1 (the reference uses W-1); 0 removes them.  They take part in glio_solve, glio_linearize,
 * glio_time_solve and glio_marginalize*, with or without a marginalization prior beside them, and leave the solver on the path it takes without them.
 * Each is evaluated together with the IMU edge that leaves its slot, so that edge has to be set when the problem is evaluated (GLIO_E_ARG otherwise).
 * glio_marginalize_keep(_async) removes them (the reference's marg = true, Estimator.cpp:2517): the prior it installs carries them on. */
int glio_set_speed_bias_priors(glio_ctx* ctx, int n_slots, const double* target);
/* Replaces addDDPsrResFactor (Estimator.cpp:1893-1897) and the tcdopplerFactor blocks
 * (Estimator.cpp:2329-2337); para_yaw_enu_local / para_anc_ecef are the constant blocks. */
int glio_set_gnss(glio_ctx* ctx, const glio_gnss_frame* frame, int n_dd, const glio_dd_psr* dd,
                  int n_dop, const glio_doppler* dop);

/* ---- the solve.  Replaces ceres::Solve(options, &problem, &summary) (Estimator.cpp:2424-2433):
 * state in = tmpTrans/tmpQuat/tmpSpeedBias(/para_rcv_ddt) before, out = after. */
int glio_solve(glio_ctx* ctx, glio_state* state_inout, glio_summary* summary);
/* One linearisation at `state`: dense H = J^T J (n x n row-major, n = 15 W + state->n_ddt),
 * g = J^T r, cost; after loss correction and local parameterisation, unscaled.  H/g may be NULL.
 * Exposed so that parity can be checked per linearisation (SURVEY.md section 7 "hard parts"). */
int glio_linearize(glio_ctx* ctx, const glio_state* state, double* H, double* g, double* cost);

/* ---- marginalization of the oldest keyframe.  Replaces the MarginalizationInfo block of
 * Estimator.cpp:2462-2607 (addResidualBlockInfo x {prior, IMU(0,1), every LidarPlaneNormFactor with Huber},
 * preMarginalize, marginalize, getParameterBlocks(addr_shift)) on the factors currently set in the context,
 * evaluated at `state` (the solution of glio_solve).  Outputs, caller-allocated for n = 6 (W-1) + 9 and
 * nb = 2 (W-1) + 1 (glio_marginalize_size in the windows after a loop closure): lin_jac [n][n] row-major, lin_res [n], blocks (slot already shifted s -> s-1, kind, first
 * column, x0[9]) -- exactly the fields of glio_prior for the NEXT window.  lin_jac^T lin_jac and
 * lin_jac^T lin_res equal the reference's (it factors the Schur complement by eigen-decomposition, this
 * library by Cholesky: a different square root of the same matrix).  GLIO_E_NUMERIC if the Schur
 * complement is not positive definite. */
int glio_marginalize(glio_ctx* ctx, const glio_state* state, double* lin_jac, double* lin_res,
                     int32_t* blk_slot, int32_t* blk_kind, int32_t* blk_idx, double* blk_x0,
                     int32_t* out_n, int32_t* out_n_blocks);
/* What the next glio_marginalize will write: n and n_blocks.  6 (W-1) + 9 and 2 (W-1) + 1 unless speed-bias priors are set or the installed prior
 * already carries speed-bias blocks of several keyframes (the windows after a loop closure): the reference re-creates the speed-bias priors at the state
 * being marginalized (Estimator.cpp:2483-2518) and KEEPS the blocks of slots 1 .. W-2.  Kept layout: the standard columns at their usual offsets, then the
 * speed/bias of every slot s >= 2 that has such a prior or a speed-bias block in the installed prior, in ascending slot order at 6 (W-1) + 9 + 9 j, named
 * s-1.  The following windows shrink it by one block per keyframe. */
int glio_marginalize_size(glio_ctx* ctx, int32_t* out_n, int32_t* out_n_blocks);

/* The same, but the result is installed as THIS context's prior for the next window without leaving the device
 * (= glio_marginalize + glio_set_prior of its output, minus the two PCIe trips of the n x n matrix).  The caller then
 * slides its state arrays / scans / IMU edges by one keyframe as the reference does (Estimator.cpp:2584-2607, 4300ff). */
int glio_marginalize_keep(glio_ctx* ctx, const glio_state* state);
/* the same in two halves: _async enqueues everything and returns (the host is free, e.g. for glio_set_scan_ahead, while the GPU marginalizes); _finish waits and
 * reports GLIO_E_NUMERIC if the Schur complement was not positive definite (the context is then left without a prior).  Every entry point that reads the prior
 * finishes a pending marginalization by itself. */
int glio_marginalize_keep_async(glio_ctx* ctx, const glio_state* state);
int glio_marginalize_keep_finish(glio_ctx* ctx);

/* ---- single-factor evaluators with the exact Evaluate() pointer convention, computed on the GPU.
 * A ceres::CostFunction shim is a five-line wrapper around these. */
/* LidarPlaneNormFactor (LidarKeyframeFactor.h:73-122): parameters = {t[3], q[4]} */
int glio_eval_lidar_plane(glio_ctx* ctx, const float cp[4], const float plane[4], double score,
                          double const* const* parameters, double* residuals, double** jacobians);
/* ImuFactor::Evaluate (ImuFactor.h:21-171): parameters = {Pi,Qi,SBi,Pj,Qj,SBj} */
int glio_eval_imu(glio_ctx* ctx, const glio_preint* pre, double const* const* parameters,
                  double* residuals, double** jacobians);

/* dd_psr_factor_20::Evaluate (dd_psr_factor.hpp:25-171): parameters = {Pi[3], Pj[3], yaw[1], anc[3]}, 19 residuals
 * (rows >= n_sat-1 zero), jacobians[0..1] 19x3 row-major; jacobians[2..3] are not written (the reference leaves them) */
int glio_eval_dd_psr(glio_ctx* ctx, const glio_dd_psr* f, double const* const* parameters, double* residuals,
                     double** jacobians);
/* tcdopplerFactor (dopp_factor.hpp:24-75): parameters = {Pi[3], SBi[9], Pj[3], SBj[9], rcv_ddt[>epoch], yaw[1], anc[3]},
 * 1 residual; jacobians[0..3] 1x3 / 1x9 / 1x3 / 1x9, jacobians[4] receives d r / d rcv_ddt[epoch] as ONE double */
int glio_eval_doppler(glio_ctx* ctx, const glio_doppler* f, double const* const* parameters, double* residuals,
                      double** jacobians);
/* MarginalizationFactor::Evaluate (MarginalizationFactor.cpp:233-287): parameters[b] = kept block b (3, 4 or 9 doubles),
 * prior->n residuals, jacobians[b] n x size_b row-major */
int glio_eval_marginalization(glio_ctx* ctx, const glio_prior* prior, double const* const* parameters,
                              double* residuals, double** jacobians);
/* BinaryLidarPlaneNormFactor (LidarKeyframeFactor.h:124-164): parameters = {t1[3], q1[4], t2[3], q2[4]}, 1 residual */
int glio_eval_binary_plane(glio_ctx* ctx, const float cp[4], const double norm_cent[6], double score,
                           double const* const* parameters, double* residuals, double** jacobians);

/* ---- measurement hooks (bench.py): time `reps` launches of one kernel with HIP events on the
 * context's stream; returns average milliseconds per launch in *ms_out. */
enum { GLIO_KERNEL_LIDAR_LINEARIZE = 0, GLIO_KERNEL_FULL_LINEARIZE = 1, GLIO_KERNEL_TR_STEP = 2,
       GLIO_KERNEL_ASSOCIATE = 3, GLIO_KERNEL_MAP_BUILD = 4, GLIO_KERNEL_MARGINALIZE = 5,
       GLIO_KERNEL_STREAM_READ = 6 /* same bytes as LIDAR_LINEARIZE, no arithmetic: the practical ceiling */,
       GLIO_KERNEL_LINEARIZE_ALL = 7 /* the launch glio_solve uses: K3 workgroups beside the small-factor workgroups */,
       GLIO_KERNEL_TR_STEP_STEADY = 8 /* a LATER step of a solve (an accepted candidate pending, scale in place: call after a solve): what iterations 2.. cost;
                                         GLIO_KERNEL_TR_STEP is the first step of a solve (no candidate yet, the helpers' speculative build does not apply) */ };
int glio_time_kernel(glio_ctx* ctx, int which, int reps, float* ms_out);
/* time `reps` complete solves from the same initial state with HIP events (state is not modified) */
int glio_time_solve(glio_ctx* ctx, const glio_state* state, int reps, float* ms_out, glio_summary* last);


/* ================================================================================================
 * Batch stage (scan-to-multiscan), the one piece that shards over GPUs.
 * Replaces, inside Estimator::optimizeBatchWithLandMark (Estimator.cpp:2739-3410), the evaluation of all
 * BinaryLidarPlaneNormFactor residual blocks (LidarKeyframeFactor.h:124-164, built at Estimator.cpp:3004-3076,
 * no loss function :2768) and their J^T J / J^T r build.  Unknowns: K keyframe poses (t, q), local size 6 K;
 * H is block banded: block (k, k+d), d = 0..band, stored at Hg[(k*(band+1)+d)*36 ...] (row-major 6x6),
 * followed by g [K][6] and the cost (1 double): Hg has glio_batch_hg_size(K, band) doubles.
 * Each rank loads only ITS constraints.  Damped Gauss-Newton path (glio_batch_linearize_dev / _step_dev): the ranks' Hg buffers are
 * summed with one RCCL all-reduce by the caller, then every rank runs the same banded solve.  Trust-region path
 * (glio_batch_solve_tr2, below): everything is sharded, see there.
 * Pointers named *_dev are DEVICE pointers (e.g. torch tensors); the others are host memory. */
typedef struct glio_batch glio_batch;
int64_t glio_batch_hg_size(int K, int band);
int glio_batch_create(int device, int K, int band, int64_t max_constraints, glio_batch** out);
void glio_batch_destroy(glio_batch* b);
int glio_batch_set_stream(glio_batch* b, void* hip_stream);
/* constraints sorted by (ci, cj); cp [n][4] float (point in frame ci), norm_cent [n][6] double (plane normal and
 * centroid in frame cj), score [n]; |ci-cj| in 1..band */
int glio_batch_set_constraints(glio_batch* b, int64_t n, const int32_t* ci, const int32_t* cj, const float* cp,
                               const double* norm_cent, const double* score);
int glio_batch_set_constraints_dev(glio_batch* b, int64_t n, const int32_t* ci_host, const int32_t* cj_host,
                                   const float* cp_dev, const double* norm_cent_dev, const double* score_dev);
/* the same from a pair list (the output of glio_bassoc_run): pair p = (pair_ci[p], pair_cj[p]) owns pair_count[p]
 * consecutive records of the device arrays; pairs sorted by (ci, cj) */
int glio_batch_set_constraints_pairs_dev(glio_batch* b, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj,
                                         const int64_t* pair_count, const float* cp_dev, const double* norm_cent_dev,
                                         const double* score_dev);
/* (every *_dev entry point BORROWS device buffers and reads them on the library's own non-blocking stream: the caller's stream must have finished
 * producing them before the call)
 * the same for a constraint set that differs from the previous one only in the pairs marked in pair_changed (one byte per input pair; NULL = all):
 * the outer rounds of optimizeBatch re-search the first / last search_range keyframes and keep the stored interior constraints
 * (Estimator.cpp:3018-3030); the next solve then reads the constraints of the marked pairs only (glio_batch_solve_tr2). */
int glio_batch_update_constraints_pairs_dev(glio_batch* b, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj, const int64_t* pair_count,
                                            const float* cp_dev, const double* nc_dev, const double* score_dev, const uint8_t* pair_changed);
/* the same with every pair's record range given explicitly: [pair_offset[p], pair_offset[p] + pair_count[p]) (NULL = the pairs follow each other).  The caller
 * of the outer rounds keeps the stored interior constraints where they are and rewrites only the regions of the re-searched end keyframes. */
int glio_batch_update_constraints_pairs_at_dev(glio_batch* b, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj, const int64_t* pair_count,
                                               const int64_t* pair_offset, const float* cp_dev, const double* nc_dev, const double* score_dev, const uint8_t* pair_changed);
/* poses [K][7] = (t, q) host; Hg_dev device buffer of glio_batch_hg_size doubles (overwritten) */
int glio_batch_linearize_dev(glio_batch* b, const double* poses, double* Hg_dev);
/* damped Gauss-Newton step from a (reduced) Hg: solves (H + lambda diag(H)) d = -g with a block-banded Cholesky on
 * the device and returns poses (+) d; *model_decrease = -(g.d + d^T H d / 2).  poses_out may alias poses_in. */
int glio_batch_step_dev(glio_batch* b, const double* Hg_dev, double lambda, const double* poses_in, double* poses_out,
                        double* model_decrease);
/* ---- the rest of the batch problem and its trust-region solve (Estimator.cpp:2739-3410, sms_fusion_level 1).
 * glio_batch_set_small_factors: delta_q_factor_auto attitude constraints (Estimator.cpp:2831-2891; dq_const [n_dq][4] = const_diff,
 *   blocks q[dq_i], q[dq_j]) and dd_psr_factor_20 per GNSS epoch (Estimator.cpp:3197-3271; slot_i / slot_j = leftKey / rightKey,
 *   identity weight and the station position as addDDPsrResFactor_gl passes them, :1899-1911; `threshold` = DDpsr_threshold of the
 *   current outer round, :2764-2767).  Given whole on every rank; a rank keeps the factors whose first keyframe it owns.
 * glio_batch_set_imu: the ImuFactor chain between consecutive keyframes (Estimator.cpp:2990-3001; gl_tmpSpeedBias blocks :2809-2819):
 *   edges[k] = the pre-integration between keyframes k and k + 1 (the caller decides which interval that is),
 *   n_edges = K - 1, or 0 for the pose-only problem.  With the chain every keyframe has 15 unknowns (band <= 12: the reference's +-12 end windows).
 * glio_batch_set_shard / glio_batch_shard_range: this object is rank `rank` of `world`; it owns a contiguous range of whole
 *   super-blocks of keyframes (6, or 12 for bands > 6).  The constraints handed to glio_batch_set_constraints* must have their source
 *   keyframe (ci) in that range.  Call before glio_batch_set_small_factors.
 * glio_batch_solve_tr2: ceres::Solve of Estimator.cpp:3275-3284 (DOGLEG, opts->dogleg_type = SUBSPACE_DOGLEG, non-monotonic steps,
 *   max_num_iter), device resident -- the host feeds kernel groups and synchronises once per solve.  Returns, as Ceres does, the
 *   iterate of least cost (poses [K][7] in/out, speed_bias [K][9] in/out with the IMU chain) and that cost as final_cost.
 *   `allreduce` (NULL = one rank) is called with a device buffer, its length in doubles, the HIP stream it is produced and consumed on
 *   and `user`; it must leave the sum over the ranks in place ORDERED ON THAT STREAM (ncclAllReduce on it in C++;
 *   torch.distributed.all_reduce with that stream current in Python) -- the host does not wait for it.  Per trust-region iteration:
 *   the assembly buffer (band rows next to the range boundaries + diagonal + gradient + cost), the separator system of the block
 *   cyclic reduction, the Gauss-Newton step, and two 64-byte buffers of curvature sums; every rank the same sequence.
 *   The plane constraints are READ ONCE per call: BinaryLidarPlaneNormFactor's residual is linear in (R_b^T R_a, R_b^T (t_a - t_b)) and
 *   carries no loss function, so the first linearisation takes 12-dimensional moments per keyframe pair (centred at the call's poses) and
 *   every later one evaluates them -- the same sums, exact (GLIO_BATCH_MOMENTS=0 in the environment streams the constraints every time).
 *   A caller that changes the constraint set calls again (every outer round of optimizeBatch does, Estimator.cpp:3018-3030).
 * glio_batch_linearize_full: one linearisation through the same path (parity hook): diag(H) [n], g [n], cost, n = (6 | 15) K. */
typedef void (*glio_allreduce_fn)(double* dev, int64_t count, void* hip_stream, void* user);
int glio_batch_shard_range(int K, int band, int rank, int world, int32_t* lo, int32_t* hi);
int glio_batch_set_shard(glio_batch* b, int rank, int world);
int glio_batch_set_small_factors(glio_batch* b, const glio_gnss_frame* frame, int n_dq, const int32_t* dq_i, const int32_t* dq_j,
                                 const double* dq_const, int n_dd, const glio_dd_psr* dd);
/* LidarPoseFactorBatchRelativeAutoDiff (GLIO/include/factors/LidarPoseFactor.h:55-97), the relative-pose factors that ARE the scan-to-multiscan
 * constraints when sms_fusion_level == 0 (Estimator.cpp:2897-2955; the released default, config_urban_hk.yaml:63): blocks (P, Q) of keyframes rp_i[f]
 * and rp_j[f], rp_const [n_rp][7] = (delta_q w,x,y,z, delta_p) from the odometry poses.  Call BEFORE glio_batch_set_small_factors, which builds the
 * factor table (n_dq = n_dd = 0 is fine there). */
int glio_batch_set_relative_pose_factors(glio_batch* b, int n_rp, const int32_t* rp_i, const int32_t* rp_j, const double* rp_const);
int glio_batch_set_dd_threshold(glio_batch* b, double threshold);   /* the next round's DDpsr_threshold, factors stay on the device */
int glio_batch_set_imu(glio_batch* b, int n_edges, const glio_preint* edges, double gravity);
int glio_batch_add_small_dev(glio_batch* b, const double* poses, double* Hg_dev);      /* damped Gauss-Newton path, one rank */
int glio_batch_linearize_full(glio_batch* b, const double* poses, const double* speed_bias, glio_allreduce_fn allreduce, void* user,
                              double* diag, double* grad, double* cost);
int glio_batch_solve_tr2(glio_batch* b, double* poses, double* speed_bias, const glio_batch_tr_opts* opts, glio_allreduce_fn allreduce,
                         void* user, glio_summary* summary);
/* the pose-only problem (no IMU chain set) */
int glio_batch_solve_tr(glio_batch* b, double* poses, const glio_batch_tr_opts* opts, glio_allreduce_fn allreduce, void* user, glio_summary* summary);
/* hook calls, doubles handed to the hook, trust-region groups enqueued, elimination levels since the last call (reset on read) */
int glio_batch_debug_counters(glio_batch* b, int64_t* out4);
/* trust-region groups glio_batch_solve_tr2 keeps in flight: group g is enqueued when group g - lead has decided that the solve goes on; the groups behind the
 * deciding one exit at once on the device.  Every rank enqueues the same number of groups (a function of the device's decisions, not of host timing), so
 * the collective sequences match.  1 = wait for every group's decision before enqueuing the next (the round-4 loop); 0 = default (2). */
int glio_batch_debug_set_enqueue_lead(glio_batch* b, int lead);

/* For a C++ host that never includes HIP headers (glio_amd/host/glio_batch_backend.hpp): the reduced buffer
 * [H band | g | cost] as a device allocation, the batch stream to hand to ncclAllReduce between glio_batch_linearize_dev and
 * glio_batch_step_dev, a read-back of a few of its doubles (the cost is the last one), a stream synchronisation. */
int glio_batch_hg_alloc_dev(glio_batch* b, double** out_dev);
int glio_batch_hg_free_dev(glio_batch* b, double* dev);
int glio_batch_get_stream(glio_batch* b, void** out_hip_stream);
int glio_batch_read_dev(glio_batch* b, const double* dev, int64_t first, int64_t n, double* out_host);
int glio_batch_synchronize(glio_batch* b);
/* 0 = the sequential banded Cholesky (one workgroup), 1 = block cyclic reduction (default where the band permits) */
int glio_batch_debug_set_solver(glio_batch* b, int mode);
/* timing hook: average ms of `reps` banded solves (H + lambda diag H) x = g (HIP events on the batch stream) */
int glio_batch_time_solve(glio_batch* b, const double* Hg_dev, double lambda, int reps, float* ms_out);
/* timing hook: average ms of `reps` linearisation launches (HIP events on the batch stream) */
int glio_batch_time_linearize(glio_batch* b, const double* poses, double* Hg_dev, int reps, float* ms_out);


/* ================================================================================================
 * Batch association.  Replaces findGlobalCorrespondingSurfFeaturesAdd_Batch(idx, search_idx_start)
 * (Estimator.cpp:3808-3892; its twin findGlobalCorrespondingSurfFeatures_Batch :3711-3806 is the same arithmetic)
 * for a list of keyframe pairs: per pair (ci, cj) the points of surf_frames[ci] are matched against surf_frames[cj],
 * both placed with pose_info_keyframe (poses [K][7] = t, q): exact 5-NN (sqd[4] < 1.5), plane fit in global and in
 * cj-local coordinates, 0.18 validity, float pd / weight, weight > 0.3.  Output per kept point, appended pair after
 * pair in the caller's order (device resident, the layout glio_batch_set_constraints_pairs_dev takes):
 *   cp [4] float (the point in ci's frame), norm_cent [6] (unit normal and 5-point centroid in cj's frame),
 *   score = 2.5 weight.   The caller applies the search-window rule of Estimator.cpp:3009-3017 to make the pair list
 * (glio_amd/batch.py: search_window). */
typedef struct glio_bassoc glio_bassoc;
int glio_bassoc_create(int device, int K, int max_points_per_frame, int64_t max_constraints, glio_bassoc** out);
void glio_bassoc_destroy(glio_bassoc* b);
/* surf_frames[k]: PointXYZI[n] as 4 floats, keyframe-local; stays resident */
int glio_bassoc_set_frame(glio_bassoc* b, int k, const float* scan_xyzi, int n);
int glio_bassoc_set_frame_strided(glio_bassoc* b, int k, const void* scan_points, int n, int stride_bytes, int intensity_offset);
int glio_bassoc_run(glio_bassoc* b, const double* poses, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj,
                    int64_t* pair_count_out, int64_t* total_out);
/* batchFeatureAssociation() (Estimator.cpp:3413-3432), the call that ENDS every optimizeSlidingWindowWithLandMark (:2733): the keyframe
 * idx = size - search_range - 1 is matched against its 2 search_range neighbours and the records are ADDED to gl_vec_surf_* -- here: appended behind
 * what the object already holds (pair_count_out: the pairs of this call; total_out: everything held).  _async enqueues on the object's stream and
 * returns (the inputs are staged in pinned memory); glio_bassoc_finish waits and hands the counts over.  glio_bassoc_reset forgets the records.
 * Any other entry point of the object may be called in between (each waits for the run as far as it must): the run's counts -- and its
 * overflow error, if it produced more than max_constraints records -- are kept for glio_bassoc_finish and reported there ONCE; a second run
 * started before glio_bassoc_finish replaces the first run's counts, but returns its overflow error instead of starting. */
int glio_bassoc_run_append(glio_bassoc* b, const double* poses, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj,
                           int64_t* pair_count_out, int64_t* total_out);
int glio_bassoc_run_append_async(glio_bassoc* b, const double* poses, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj);
int glio_bassoc_finish(glio_bassoc* b, int64_t* pair_count_out, int64_t* total_out);
int glio_bassoc_reset(glio_bassoc* b);
/* globalFeatureSelectionAdd_Batch (Estimator.cpp:4057-4116) for the pairs of the asynchronous run in flight, ON ITS STREAM (call it right after
 * glio_bassoc_run_append_async, before glio_bassoc_finish): no host round trip between the searches and the selection.  The draws stay the caller's:
 * raws = res_num (<= 64) 64-bit numbers per pair of that run, drawn before the counts exist.  A pair with at most res_num records keeps them all; else it
 * keeps the first res_num of a uniform shuffle of its records but the last (random_generator.hpp:79-93 never draws it): step i swaps position i with
 * position i + raws[p * res_num + i] mod (count - 1 - i).  glio_bassoc_finish then reports the per-pair counts FOUND and the total HELD after the selection. */
int glio_bassoc_select_tail_draws_async(glio_bassoc* b, int res_num, const uint64_t* raws);
/* Optional, ahead of a run whose pairs are known before its poses (batchFeatureAssociation inside a keyframe call: the pairs follow from the keyframe count,
 * the poses from the solve): sends the build descriptors of the run's search frames and clears their hash tables now; the run that follows with the same
 * search frames skips both.  Anything else in between only makes the run do them itself.  Whether a preparation applies follows from what was prepared
 * (same search frames, same cloud sizes) and from nothing else -- not from how long ago it was made. */
int glio_bassoc_prepare_async(glio_bassoc* b, int n_pairs, const int32_t* pair_ci, const int32_t* pair_cj);
/* surf_frames[k] <- the scan resident in window slot `slot` of a sliding-window context on the same device, minus the LiDAR offset (a device copy:
 * the keyframe that just entered the window is not uploaded a second time).  The copy runs on the association's stream; the context's next
 * glio_set_scan and glio_destroy are ordered behind it on the device (no host wait). */
int glio_bassoc_set_frame_from_scan(glio_bassoc* b, int k, glio_ctx* ctx, int slot, const float lidar_offset[3]);
/* ---- the local map rebuilt from resident keyframes.  buildLocalMapWithLandMark's rebuild branch (Estimator.cpp:3545-3579) + downSampleCloud + setInputCloud
 * (:3618-3631, :2056): whenever recent_surf_keyframes holds fewer than local_map_width clouds -- during the first local_map_width keyframes of every run, and on
 * EVERY keyframe call after the first loop closure (correctPoses clears the deque, :4660, and the loop's guard at :3550 then refills it with local_map_width - 1
 * clouds only) -- the reference throws the deque away and re-transforms surf_frames[idx] of the last keyframes at their current pose_info_keyframe poses.
 * The ring becomes exactly the n_frames keyframes frame_idx[0..n) (oldest first = concatenation order) of `frames`' resident own-frame clouds
 * (glio_bassoc_set_frame*: scan - lidar_offset, the floats glio_localmap_push_scan forms), each moved by transformCloud at poses[f] = t[3], q[4] (w first; the
 * layout of glio_loop_build_submap; q, t = q_po * q_bl, q_po * t_bl + t_po as for glio_localmap_push), then voxel grid + K1 as glio_localmap_build does.
 * *out_points = the map's size.  Bit for bit what a fresh ring gives that got glio_localmap_push(cloud frame_idx[f], pose f) for f = 0..n-1 and then
 * glio_localmap_build, in both accumulation modes, and later pushes / evictions / builds go on as if those pushes had happened -- in two launches plus the
 * build's chain instead of three to four launches and one upload per frame.  Runs on the context's stream behind the association's pending frame copies (an
 * event, no host wait; the association's next write to a cloud is ordered behind the rebuild the same way) and behind a scan / map sent ahead, whose map it
 * supersedes (the scan sent ahead stays for the next glio_slide_window).  One host wait in its middle, as glio_localmap_build.
 * GLIO_E_STATE without glio_localmap_config; GLIO_E_ARG (ring untouched): n_frames outside [1, width], a frame index outside [0, K), a frame that was never
 * set (or holds no point), a frame with more points than the ring's max_points_per_keyframe, a non-finite pose, an association on another device. */
int glio_localmap_rebuild_from_frames(glio_ctx* ctx, glio_bassoc* frames, int n_frames, const int32_t* frame_idx, const double* poses /* [n_frames][7] */, int* out_points);
/* device time of the last rebuild's own two launches (table clear + the multi-frame kernel), ms; only in a process started with GLIO_LM_REBUILD_TIMING=1
 * (GLIO_E_STATE otherwise: the timing events are not recorded by default) */
int glio_localmap_last_rebuild_device_ms(glio_ctx* ctx, float* ms);
int glio_bassoc_results_dev(glio_bassoc* b, const float** cp_dev, const double** norm_cent_dev, const double** score_dev);
/* globalFeatureSelectionAdd_Batch / globalFeatureSelection_Batch (Estimator.cpp:4057-4116, 3994-4055; batch_feature_res_num: 25):
 * keep records src_index[0..n_keep) of the current n_current records, in that order (pair after pair; the caller updates its
 * per-pair counts).  The random draws stay with the caller (the reference seeds from std::random_device); the gather runs on
 * the device, in place.  glio_amd/batch.py::batch_selection_draws restates the draw rules. */
int glio_bassoc_select(glio_bassoc* b, int64_t n_keep, const int64_t* src_index, int64_t n_current);
/* the same over the tail [first, n_current) only -- what one keyframe's batchFeatureAssociation appended: src_index holds absolute indices >= first;
 * afterwards the object holds first + n_keep records.  Both calls copy src_index before they return and ENQUEUE the gather (no host wait);
 * glio_bassoc_read and glio_bassoc_results_dev wait for it, later runs and selections are ordered behind it. */
int glio_bassoc_select_range(glio_bassoc* b, int64_t first, int64_t n_keep, const int64_t* src_index, int64_t n_current);
int glio_bassoc_read(glio_bassoc* b, int64_t first, int64_t n, float* cp, double* norm_cent, double* score);

/* ---- LiDAR features from the raw scan: Preprocessing::cloudHandler (GLIO/src/Preprocessing.cpp:353-681) on the device.
 * The IMU rotation of the sweep (processIMU / solveRotation, :202-259) stays with the caller (glio_amd/features.py::ScanRotation,
 * glio::ScanRotation): q_imu is the qIMU the reference holds when the scan is handled, after the NaN guard (:415-417). */
void glio_feat_opts_default(glio_feat_opts* o);
/* sizeof() of glio_feat_opts, glio_feat_counts; returns how many there are (2) */
int glio_feat_struct_sizes(int32_t* out, int n);
/* allocates the extraction's buffers for opts->max_raw_points raw points (a context that never calls it allocates nothing for it);
 * GLIO_E_ARG for n_scans not in {16, 32, 64}, ds_rate < 1, ds_leaf <= 0 or max_raw_points outside [1, GLIO_FEAT_MAX_RAW_POINTS] */
int glio_features_config(glio_ctx* ctx, const glio_feat_opts* opts);
/* removeNaNFromPointCloud + removeClosedPointCloud (:144-168, :396-397), startOri / endOri (:401-410), ring, orientation, relTime and
 * undistortion(point, qIMU) per point (:176-200, :424-515), the stable ring bucketing (:517-526), the curvature (:529-538), the six sectors
 * of every ring with their edge / flat picks and the less-flat points (:540-646), the per-ring VoxelGrid at ds_leaf (:648-654).
 * Records of stride_bytes (a multiple of 4, >= 16: x y z floats at 0, the intensity float at intensity_offset; the intensity is not read).
 * Returns when the caller's buffer has been read and the counts are known.  n > max_raw_points: GLIO_E_ARG, nothing written; before
 * glio_features_config: GLIO_E_STATE.  A scan without survivors gives zero counts and GLIO_OK (the reference would read points[0] of
 * an empty cloud at :401). */
int glio_features_extract_strided(glio_ctx* ctx, const void* raw, int n, int stride_bytes, int intensity_offset, const double q_imu[4], glio_feat_counts* counts);
int glio_features_extract(glio_ctx* ctx, const float* xyzi, int n, const double q_imu[4], glio_feat_counts* counts);
/* one output of the last extraction (GLIO_FEAT_*), [n][4] x y z intensity; *n = its size (out may be null to ask for it); capacity too small: GLIO_E_ARG */
int glio_features_read(glio_ctx* ctx, int which, float* out_xyzi, int capacity, int* n);
/* LidarOdometry's downSampleCloud (LidarOdometry.cpp:306-314): the surf features of the last extraction, voxel-filtered at `leaf` on the device
 * (pcl::VoxelGrid, one segment; leaf <= 0: as they are), written into window slot `slot` as glio_set_scan would and presorted -- no host round trip.
 * *n = the points written; more than max_points_per_scan: GLIO_E_ARG, the slot untouched. */
int glio_features_to_scan(glio_ctx* ctx, int slot, float leaf, int* n);
/* device time of the last extraction's kernels (HIP events around them, after the raw upload), ms */
int glio_features_last_device_ms(glio_ctx* ctx, float* ms);

/* ---- The keyframe cloud: the hand-over of a keyframe's UNFILTERED surf cloud from the front end to the sliding window, on the device.
 * Replaces LidarOdometry::publishCloudLast's undistortion(surf_features, trans, quat) (GLIO/src/LidarOdometry.cpp:180-201, :619-627; only with
 * if_to_deskew) and Estimator::downSampleCloud's ds_filter_surf (Estimator.cpp:3628-3630: pcl::VoxelGrid at surfDSRange, 0.9 m in the released yaml)
 * together with the glio_set_scan of the filtered cloud: de-skew per point (line = (int)intensity, ratio = (intensity - line) / 0.1 capped at 1 and
 * not clamped below, q_si = Identity.slerp(ratio, quat), t_si = ratio * trans, pt = q_si * pt + t_si stored as float, intensity unchanged), then
 * pcl::VoxelGrid at `leaf` (all four fields averaged, float sums in input order, PCL's output order; a box of more than INT32_MAX cells passes the
 * cloud through; leaf <= 0 copies it), then the slot's row and its presort as glio_set_scan / glio_set_scan_ahead leave them.
 *   deskew_trans  [3], NULL = if_to_deskew false (no de-skew at all)
 *   deskew_quat   [4] w first, NULL = the identity (the reference's only call)
 *   *n_out        the points the slot holds afterwards
 * One host wait per call, for the output count, on the stream that carries the work (the context's for the slot forms, the upload stream for the
 * _ahead forms, which do not wait for the context's stream); when it returns a host source has been read.
 * Errors leave the slot and its count untouched: GLIO_E_ARG for a bad slot or point layout, n > max_input_points, contexts on different devices, a
 * non-finite motion, or more outputs than max_points_per_scan (*n_out still tells the count); GLIO_E_STATE before glio_scan_filter_config, or for a
 * front end without an extraction.  n == 0 gives an empty slot and GLIO_OK.
 * The full cloud's de-skew (:626), fullDS (Estimator.cpp:3623-3626) and pub_full_cloud_map are the dense store of include/glio_dense.h (glio_dense_*), which runs
 * this same de-skew and VoxelGrid.  Not built: the de-skew of edge_features (:625). */
/* allocates the stage's buffers: staging for max_input_points (1 .. GLIO_FEAT_MAX_RAW_POINTS) input points and the voxel table (a context that
 * never calls it allocates nothing for it) */
int glio_scan_filter_config(glio_ctx* ctx, int max_input_points);
/* (a) host source: records of stride_bytes as glio_set_scan_strided takes them, or a packed [n][4] array */
int glio_set_scan_filtered_strided(glio_ctx* ctx, int slot, const void* points, int n, int stride_bytes, int intensity_offset, float leaf,
                                   const double* deskew_trans, const double* deskew_quat, int* n_out);
int glio_set_scan_filtered(glio_ctx* ctx, int slot, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
/* ... into the row that is slot W - 1 after the next glio_slide_window (see glio_set_scan_ahead), on the upload stream */
int glio_set_scan_filtered_ahead_strided(glio_ctx* ctx, const void* points, int n, int stride_bytes, int intensity_offset, float leaf,
                                         const double* deskew_trans, const double* deskew_quat, int* n_out);
int glio_set_scan_filtered_ahead(glio_ctx* ctx, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
/* (b) resident source: the surf features of `frontend`'s last glio_features_extract*, read where they lie (GLIO_FEAT_SURF of the front end stays what
 * it was: the de-skew is out of place).  The work runs on ctx's stream (its upload stream for _ahead) behind an event recorded on frontend's stream;
 * frontend's next glio_features_extract*, its glio_features_config and its glio_destroy are ordered behind the read on the device -- no host wait
 * is added on frontend.  frontend == ctx is allowed. */
int glio_set_scan_from_features(glio_ctx* ctx, int slot, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
int glio_set_scan_from_features_ahead(glio_ctx* ctx, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
/* (c) what window slot `slot` holds, in the caller's order: [n][4] x y z intensity; *n = its size (out may be null to ask for it); capacity too
 * small: GLIO_E_ARG.  Waits for the context's stream. */
int glio_get_scan(glio_ctx* ctx, int slot, float* out_xyzi, int capacity, int* n);
/* device time of the last non-empty keyframe-cloud call, ms: [0] de-skew + bounding box, [1] the VoxelGrid and the copy into the row, [2] the presort --
 * only when GLIO_KFCLOUD_TIMING=1 was set at glio_scan_filter_config (the events are not recorded otherwise); GLIO_E_STATE without */
int glio_scan_filter_last_device_ms(glio_ctx* ctx, float ms[3]);

/* ---- IMU pre-integration from raw samples: class Preintegration (GLIO/include/factors/Preintegration.h:29-194) on the device.
 * A glio_imu is the reference's pre_integrations vector (Estimator.cpp:1582-1600) kept on the device: edge e is built from its start values and
 * its run of samples (one wavefront per edge, any number of edges per call), digested there into the form the ImuFactor kernels read
 * (sqrt_info = LLT(covariance^-1).L^T, ImuFactor.h:44-45), and handed to a sliding-window context or a batch stage on the same device without
 * crossing PCIe again.  A store owns one HIP stream and is not thread-safe.  An edge whose samples hold a non-finite number, or whose covariance
 * does not invert, is flagged on the device: glio_imu_read of a range that holds it returns GLIO_E_NUMERIC (glio_last_error names the edge; the
 * other edges of the range are delivered), and so does a glio_*_from_store call that is given an edge already known to be flagged. */
typedef struct glio_imu glio_imu;
/* config_urban_hk.yaml:7-10 */
void glio_imu_noise_default(glio_imu_noise* n);
/* sizeof() of glio_imu_noise, glio_imu_sample; returns how many there are (2) */
int glio_imu_struct_sizes(int32_t* out, int n);
int glio_imu_create(int device, int max_edges, int max_samples_per_edge, const glio_imu_noise* noise, glio_imu** out);
void glio_imu_destroy(glio_imu* s);
/* Preintegration(acc0, gyr0, linearized_ba, linearized_bg) + one push_back per sample, in order (Estimator::processIMU, Estimator.cpp:1581-1604),
 * for edges [first_edge, first_edge + n_edges): edge first_edge + e owns samples[sample_offset[e] .. sample_offset[e + 1]) (sample_offset has
 * n_edges + 1 non-decreasing entries; an edge without samples is the constructor's state) and start[e] = acc0[3], gyr0[3], linearized_ba[3],
 * linearized_bg[3].  Returns when the caller's buffers have been copied; the kernels run on the store's stream.  GLIO_E_ARG (nothing launched) for
 * an edge outside [0, max_edges), more than max_samples_per_edge samples in an edge, negative counts or a missing pointer. */
int glio_imu_integrate(glio_imu* s, int first_edge, int n_edges, const int32_t* sample_offset, const glio_imu_sample* samples,
                       const double* start /* [n_edges][12] */);
/* the host view of edges [first_edge, first_edge + n_edges) (waits for the store's stream) */
int glio_imu_read(glio_imu* s, int first_edge, int n_edges, glio_preint* out);
/* device time of the last glio_imu_integrate's kernel (HIP events around it, after the upload), ms; waits */
int glio_imu_last_device_ms(glio_imu* s, float* ms);
/* glio_set_imu (Estimator.cpp:2182-2192) with the edges taken from the store: edge[k] links slots slot_i[k] and slot_i[k] + 1.  The context's
 * stream waits for the store's through an event, not the host; afterwards the context is as after glio_set_imu with the same edges. */
int glio_set_imu_from_store(glio_ctx* ctx, glio_imu* s, int n_edges, const int32_t* edge, const int32_t* slot_i);
/* glio_batch_set_imu (Estimator.cpp:2990-3001) with store edges first_edge .. first_edge + K - 2 as the chain */
int glio_batch_set_imu_from_store(glio_batch* b, glio_imu* s, int first_edge, double gravity);

/* ---- loop closure: detectLoopClosure's submaps and performLoopClosure's ICP (Estimator.cpp:5101-5273) on the device.
 * A glio_loop is created on a glio_bassoc, whose resident keyframe clouds (glio_bassoc_set_frame*) it reads; it lives on the same device, owns one HIP
 * stream, and every call orders itself behind the association's pending frame copies with an event -- never behind the host.  It changes nothing the
 * association holds.  Not thread-safe by itself; meant for the reference's 1 Hz loop thread beside the keyframe cycle.
 *
 * The registration restates pcl::IterativeClosestPoint of PCL 1.8.1 (the version of the reference's docker image).  PCL is not part of the reference
 * tree, so these rules are UNPINNED: restated from the published source, never run against PCL here.  With cur = source,
 * final = I, prev_mse = DBL_MAX every round
 *   1. finds for every point of cur its exact nearest target point: float d2 = dx*dx + dy*dy + dz*dz without contraction, ties to the lowest target
 *      index; the pair is kept when (double) d2 <= max_corr_dist^2;
 *   2. stops with converged = 0, NO_CORRESPONDENCES when fewer than min_correspondences pairs are kept;
 *   3. fits the rigid transform of the kept pairs (Umeyama without scale: means, Sigma = 1/n sum (t - mu_t)(s - mu_s)^T, SVD,
 *      R = U diag(1, 1, det U det V) V^T, t = mu_t - R mu_s) and rounds it to a float 4x4.  DELIBERATE DEVIATION: PCL accumulates in float; here the sums
 *      are fp64 in a fixed order (bit-identical from run to run) and the SVD is fp64;
 *   4. cur <- T cur and final <- T final in float (((a*x + b*y) + c*z) + d per row, no contraction), iterations += 1;
 *   5. tests, in this order: iterations >= max_iterations (ITERATIONS); 0.5 (trace R - 1) >= 1 - transformation_eps and |t|^2 <= transformation_eps
 *      (TRANSFORM); mse = mean of the kept d2 in double: |mse - prev_mse| < abs_mse_eps (ABS_MSE); |mse - prev_mse| / prev_mse < fitness_eps (REL_MSE);
 *      otherwise prev_mse = mse and the next round;
 *   6. fitness = the mean over ALL final cur points of the float squared 1-NN distance, summed in double (getFitnessScore's cap defaults to DBL_MAX).
 * Pairs that are collinear (Sigma of rank < 2) determine no rotation: the round changes nothing, the alignment ends NOT_CONVERGED with rank_deficient = 1.
 * setRANSACIterations(5) (:5194) has no effect in the reference: no correspondence rejector is installed. */
typedef struct glio_loop glio_loop;
void glio_loop_opts_default(glio_loop_opts* o);
/* sizeof() of glio_loop_opts, glio_loop_result, glio_loop_step_result; returns how many there are (3) */
int glio_loop_struct_sizes(int32_t* out, int n);
int glio_loop_create(glio_bassoc* b, const glio_loop_opts* opts, glio_loop** out);
void glio_loop_destroy(glio_loop* lp);
/* one submap (which = GLIO_LOOP_SOURCE / GLIO_LOOP_TARGET) from resident keyframes: cloud frame_idx[f] moved by transformCloud with poses[f] = t[3], q[4]
 * (as glio_bassoc_run takes them; Estimator.cpp:1548-1568), concatenated in list order, pcl::VoxelGrid at opts.leaf with PCL's float sums in
 * concatenation order and PCL's output order (the arithmetic of glio_localmap_set_accumulation(ctx, 1)).  The result stays on the device;
 * *n_points = its size.  GLIO_E_ARG: n_frames outside [1, max_frames_per_submap], a frame index outside [0, K), a frame that was never set (or holds no
 * point), more voxels than the submap's capacity. */
int glio_loop_build_submap(glio_loop* lp, int which, int n_frames, const int32_t* frame_idx, const double* poses /* [n_frames][7] */, int* n_points);
/* a ready cloud [n][4] as a submap; GLIO_E_ARG for n < 1 or n above the capacity */
int glio_loop_set_submap(glio_loop* lp, int which, const float* xyzi, int n);
/* *n = the submap's size (out may be null to ask for it); capacity too small: GLIO_E_ARG */
int glio_loop_read_submap(glio_loop* lp, int which, float* out_xyzi, int capacity, int* n);
/* the whole alignment from "source as set".  Every round is enqueued ahead and turns into a no-op once the device has decided convergence; the call
 * then BLOCKS on one event behind the result's copy into pinned memory (no spinning: it runs on a 1 Hz thread and must not take a core from the keyframe
 * cycle).  GLIO_E_STATE before both submaps exist. */
int glio_loop_align(glio_loop* lp, glio_loop_result* result);
/* one round from the object's current state (the same kernels glio_loop_align enqueues); glio_loop_reset_current returns to "source as set" */
int glio_loop_reset_current(glio_loop* lp);
int glio_loop_step(glio_loop* lp, glio_loop_step_result* step);
/* the last search's answer per source point: target index (-1 beyond max_corr_dist) and float squared distance to the NEAREST target point */
int glio_loop_read_correspondences(glio_loop* lp, int32_t* idx_out, float* d2_out);
/* the current cloud (source moved by the rounds so far), [n_source][4] */
int glio_loop_read_current(glio_loop* lp, float* out_xyzi, int capacity, int* n);
/* per round of the last glio_loop_align: the queries the brute-force scan answered ([0, iterations) and one more entry for the fitness search);
 * *n = entries written */
int glio_loop_read_fallbacks(glio_loop* lp, int32_t* out, int capacity, int* n);
/* device time of the last glio_loop_align (HIP events around its kernels), ms */
int glio_loop_last_device_ms(glio_loop* lp, float* ms);

/* ---- the global map on the device.  Replaces the live part of mapVisualizationThread (Estimator.cpp:5315-5350: every mapping_interval-th keyframe's surf cloud
 * through transformCloud at its final pose, :5339-5341, the concatenation through ds_filter_global_map, :5342-5343) and the same computation of
 * publishCompleteMap (:5275-5313, poses composed at :5287-5288) over the surf clouds.  publishCompleteMap as written -- over full_clouds_ds, the FULL cloud of
 * every keyframe, whose push at :3626 the released source comments out -- is glio_gmap_create_on_dense (include/glio_dense.h).  Writing the .pcd stays
 * with the caller.
 * A glio_gmap is created on a glio_bassoc exactly like a glio_loop: same device, its own HIP stream, every call ordered behind the association's pending frame
 * copies by an event; it changes nothing the association holds.  glio_gmap_add_frames returns when its kernels are done, so the association's next write to a cloud
 * is behind the call.  Not thread-safe by itself.
 *
 * The map is, at any time, pcl::VoxelGrid(leaf) of the concatenation of every cloud added since the last clear, in the order they were added:
 *   voxel coordinates floorf(p * (1.0f / leaf)) per axis, in float; per voxel the four channels summed IN FLOAT IN CONCATENATION ORDER and divided by the float
 *   count; output by ascending PCL linear voxel index ix + iy dx + iz dx dy -- which is the order of (iz, iy, ix) whatever the bounding box.
 * Adding in several calls gives the same bytes as one call, and as a clear followed by one call: a call's points continue each voxel's stored float sum one at a time.
 * There is no removal (float sums cannot be undone): after a loop closure or a batch solve the caller clears and adds again.
 * DEVIATIONS, both stated: (1) Estimator.cpp:5340 applies Tbl and then the pose -- two float roundings per point; here ONE composed pose (q_po * q_bl,
 * q_po * t_bl + t_po, as publishCompleteMap :5287-5288 and the local map do) moves the resident scan - lidar_offset cloud.  (2) A bounding box of more than
 * INT32_MAX cells: see glio_gmap_info.pcl_index_overflow. */
typedef struct glio_gmap glio_gmap;
void glio_gmap_opts_default(glio_gmap_opts* o);
/* sizeof() of glio_gmap_opts, glio_gmap_info; returns how many there are (2) */
int glio_gmap_struct_sizes(int32_t* out, int n);
int glio_gmap_create(glio_bassoc* b, const glio_gmap_opts* opts, glio_gmap** out);
void glio_gmap_destroy(glio_gmap* gm);
/* global_map->clear() (:5348): the map is empty again */
int glio_gmap_clear(glio_gmap* gm);
/* cloud frame_idx[f] of the association moved by transformCloud (Estimator.cpp:1517-1546: double, products kept separate, stored as float) with
 * poses[f] = t[3], q[4] (w first; the layout of glio_loop_build_submap), appended in list order behind everything added since the last clear (:5339-5341); the
 * map afterwards is the VoxelGrid of the whole concatenation (:5342-5343).  Repeated frame indices are allowed.  info may be null.
 * GLIO_E_ARG, and THE MAP STAYS EXACTLY AS IT WAS (size, bytes, device pointer): n_frames < 1 (or above 65535), a frame index outside [0, K), a frame that was
 * never set or holds no point, a pose that is not finite, more points than max_points_per_add, more voxels than max_voxels, a voxel coordinate outside
 * [-2^20, 2^20). */
int glio_gmap_add_frames(glio_gmap* gm, int n_frames, const int32_t* frame_idx, const double* poses /* [n_frames][7] */, glio_gmap_info* info);
int glio_gmap_size(glio_gmap* gm, int* n_voxels);
/* voxels [first, first + n) of the map into out_xyzi [n][4] (ranges: a map can be gigabytes); GLIO_E_ARG for a range outside the map */
int glio_gmap_read(glio_gmap* gm, int first, int n, float* out_xyzi);
/* the map as a device pointer ([n_voxels] float4 on the association's device), valid until the next successful glio_gmap_add_frames; n_voxels may be null */
int glio_gmap_points_dev(glio_gmap* gm, const void** points_dev, int* n_voxels);
/* device time of the last glio_gmap_add_frames (HIP events around its kernels), ms; _stage_ms: the same by stage, ms4 = transform, sort, runs + sums, merge */
int glio_gmap_last_device_ms(glio_gmap* gm, float* ms);
int glio_gmap_last_stage_ms(glio_gmap* gm, float* ms4);

/* ---- the pose graph on the device: what the reference keeps in one gtsam::ISAM2 -- the GLOBAL graph (Estimator.cpp:4586-4652: one node per frame, a
 * PriorFactor<Pose3> on node 0, a BetweenFactor<Pose3> with odom_noise between consecutive frames, one BetweenFactor per loop closure, :5251-5256;
 * global_estimated = isam->calculateEstimate() feeds correctPoses) and the LOCAL graph (:4561-4581, addLIOFactor :1999-2043, addGNSSFactor :1915-1997: one
 * node per keyframe that left the window, gtsam::GPSFactor every >= 5 m, poseCovariance = isam->marginalCovariance(last)).  One object serves either.
 * GTSAM is not part of the reference tree: every GTSAM-side rule below is UNPINNED -- restated from its published behaviour, never
 * run against GTSAM here.  The host's share (which factor when: the gates of addGNSSFactor, the per-frame insertion) is glio_amd/posegraph.py and
 * host/glio_posegraph_backend.hpp.
 *
 * State: a pose x = (R, t), handed over as t[3], q[4] (w first), the layout of glio_loop_build_submap / glio_gmap_add_frames / glio_localmap_rebuild_from_frames.
 * Retraction: x [+] d = (R Exp(d_r), t + R d_t), d = (d_r, d_t): ROTATION FIRST, as gtsam::Pose3's tangent and the variance vectors of :864-865, :5246.
 *   between (i, j; R_m, t_m; var[6]):  r = [Log(R_m^T R_i^T R_j) ; R_m^T (R_i^T (t_j - t_i) - t_m)], every row divided by sqrt(var)
 *   prior   (i; R_p, t_p; var[6]):     r = [Log(R_p^T R) ; R_p^T (t - t_p)]
 *   GPS     (i; p; var[3]):            r = t - p
 * Log is the SO(3) logarithm (taken from the unit quaternion with w >= 0: phi = 2 atan2(|v|, w) v / |v|; for |v| < 1e-3 the series
 * 2 / w (1 - u^2 / 3 + u^4 / 5), u = |v| / w).  The rotational Jacobians use the inverse right Jacobian I + 1/2 [phi]x + c [phi]x^2,
 * c = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta), and for theta < 1e-2 the series c = 1/12 + theta^2 / 720 + theta^4 / 30240.
 * DEVIATION 1: a GTSAM 4.0 build without GTSAM_ROT3_EXPMAP uses the Cayley chart for Rot3; it differs from Log at third order in the residual angle.
 * DEVIATION 2: iSAM2 with relinearizeThreshold 0.1 is an incremental approximation of the maximum-a-posteriori estimate; here every glio_pgraph_solve is the
 * BATCH Gauss-Newton estimate of the whole graph, started from the current estimate, all in fp64.
 * Gauss-Newton (no damping) with gtsam::GaussNewtonParams' termination, decided ON THE DEVICE on the total error E = 1/2 |r|^2: after every iteration
 * stop CONVERGED when E_new <= 0, or (E - E_new) / E <= relative_error_tol, or E - E_new <= absolute_error_tol; stop ITERATION_LIMIT at max_iterations.
 * Never on a step norm: with the reference's prior (translation variance 1e8 against odometry information 1e4) the absolute translation is numerically a gauge.
 * A NEGATIVE decrease passes both tests: an iteration that RAISES the error ends the solve CONVERGED with that worse estimate kept in the pose table
 * (final_error > initial_error; a long drive with accumulated drift does this on its first full step).  glio_pgraph_solve_damped (include/glio_pgraph_lm.h, below)
 * is the solve that never leaves a worse estimate: use it after a loop closure over a long drive.
 * Every iteration solves the normal equations by ONE exact Cholesky in a fixed order (nested dissection: node 0, the last node, every loop endpoint and evenly
 * spaced nodes are separators; the chain between two separators is eliminated by one wavefront per segment; the separator system is factored as a band plus the
 * full rows of loop endpoints).  No atomic takes part in a sum: two runs give the same bits.  A non-positive pivot ends the solve with termination
 * NONPOSITIVE_PIVOT and the estimate the solve STARTED from is put back.  The iteration loop is enqueued ahead (the first 12 iterations, then, for a solve that needs more, the rest): the host waits once, or twice.
 * A glio_pgraph owns one HIP stream and is not thread-safe.  Every refusal is GLIO_E_ARG and changes nothing. */
typedef struct glio_pgraph glio_pgraph;
void glio_pgraph_opts_default(glio_pgraph_opts* o);
/* sizeof() of glio_pgraph_opts, glio_pgraph_info; returns how many there are (2) */
int glio_pgraph_struct_sizes(int32_t* out, int n);
/* GLIO_E_ARG: max_nodes outside [1, 2^24], max_loops outside [0, 1024], max_unary < 0, segment_nodes < 0, a tolerance or default variance that is not finite */
int glio_pgraph_create(int device, const glio_pgraph_opts* opts, glio_pgraph** out);
void glio_pgraph_destroy(glio_pgraph* pg);
/* an empty graph again: no node, no factor, no prior (new gtsam::ISAM2, Estimator.cpp:864) */
int glio_pgraph_clear(glio_pgraph* pg);
/* PriorFactor<Pose3>(0, pose, prior_noise) (Estimator.cpp:4592-4594, :4565-4567): the prior of node 0; a second call replaces it.  var null: opts.prior_var */
int glio_pgraph_set_prior(glio_pgraph* pg, const double pose[7], const double var[6]);
/* n nodes at the end with poses[k] as their initial estimates, and per new node one BetweenFactor(previous, this, between(previous given pose, this given
 * pose), odom_noise) (Estimator.cpp:4613-4633, addLIOFactor :2020-2040).  prev_pose is what the caller holds for the current last node (pose_each_frame[i-1]);
 * null: its current estimate.  The first node of an empty graph gets no between factor (prev_pose is not read).  var null: opts.odom_var.
 * Quaternions are normalised; a zero quaternion is refused. */
int glio_pgraph_append(glio_pgraph* pg, int n, const double* poses /* [n][7] */, const double* prev_pose /* [7] or null */, const double* var /* [6] or null */);
/* BetweenFactor<Pose3>(i, j, rel, Variances(var)) for a loop closure (Estimator.cpp:5251-5254: rel = poseFrom.between(poseTo) of glio::loopConstraint /
 * loop.loop_constraint, var = six times icp.getFitnessScore()); i != j, in either order */
int glio_pgraph_add_between(glio_pgraph* pg, int i, int j, const double rel[7], const double var[6]);
/* gtsam::GPSFactor(i, xyz, Variances(max(var, gps_var_floor))) (Estimator.cpp:1985-1989) */
int glio_pgraph_add_gps(glio_pgraph* pg, int i, const double xyz[3], const double var[3]);
/* isam->update() + calculateEstimate() (Estimator.cpp:4572-4580, :4641-4650), as the batch estimate stated above.  info may be null.  GLIO_E_ARG before a
 * node exists and before a prior or a GPS factor exists.  A NONPOSITIVE_PIVOT termination is reported in info with GLIO_OK. */
int glio_pgraph_solve(glio_pgraph* pg, glio_pgraph_info* info);
int glio_pgraph_size(glio_pgraph* pg, int* n_nodes);
/* the current estimates of nodes [first, first + n): unit quaternions with w >= 0 */
int glio_pgraph_read_poses(glio_pgraph* pg, int first, int n, double* out /* [n][7] */);
/* isam->marginalCovariance(node) (Estimator.cpp:4578): the node's 6x6 block of the inverse of the normal matrix at the current estimate, row major, in the
 * tangent frame stated above (rotation first; entries (3,3), (4,4) gate addGNSSFactor, :1938); symmetric to the bit.  GLIO_E_NUMERIC on a non-positive pivot. */
int glio_pgraph_marginal_covariance(glio_pgraph* pg, int node, double* out /* [36] */);
/* the total error 1/2 |r|^2 of the current estimate */
int glio_pgraph_error(glio_pgraph* pg, double* error);
/* the pose table on the device ([n_nodes][7] doubles t, q), valid until the next successful glio_pgraph_solve / glio_pgraph_append / glio_pgraph_clear */
int glio_pgraph_poses_dev(glio_pgraph* pg, const double** poses_dev, int* n_nodes);
/* the damped (Levenberg-Marquardt) solve on the same object: its entry points and its contract (final_error <= initial_error, always) */
#include "glio_pgraph_lm.h"

#ifdef __cplusplus
}
#endif
#endif /* GLIO_HIP_H_ */

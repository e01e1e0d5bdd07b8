/* glio_traj.h -- the every-frame trajectory on the device: the part of Estimator::saveKeyFramesAndFactors that produces pose_each_frame
 * (GLIO/src/Estimator.cpp:4273-4557) with optimizeLocalGraph (:3452-3527) and its factors (LidarPoseFactor.h:11-52, 128-221).
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * A GAP is the stretch between the keyframe that left the window (a) and the window's oldest keyframe (b): N = keyframe_id_in_frame[b] -
 * keyframe_id_in_frame[a] - 1 in-between frames (the reference's numPara of optimizeLocalGraph) and N + 1 SEGMENTS of IMU samples, frame to frame and the
 * last one on to b's stamp.  The host decides which samples make a segment (glio::frameImuSamples / trajectory.frame_samples); everything else is ONE
 * launch of one wavefront per gap on the object's own stream, fp64, products not contracted:
 *   (a) dead reckoning (:4279-4493)  per sample row  un_acc_0 = R a0 - g, un_gyr = (gy0 + gy1) / 2, R *= deltaQ(un_gyr dt).toRotationMatrix() with
 *       deltaQ = (1, un_gyr dt / 2) NOT normalised (R drifts off orthonormal, as in the reference), un_acc_1 = R a1 - g, P += dt V + dt dt / 2 un_acc,
 *       V += dt un_acc; Ba = Bg = 0.  The first row of a segment only sets a0, gy0 (the sample interpolated at the segment's first stamp; its dt is ignored).
 *       At the end of segment i the pose row i is (P, Quaterniond(R)): Eigen 3.3's trace branch and three diagonal branches, not normalised.
 *   (b) measurements (:4494-4555)    row i relates pose row i - 1 (row -1 = prev_row, pose_each_frame[keyframe_id_in_frame[a]]) to pose row i:
 *       dq = q_{i-1}^-1 q_i, dp = q_{i-1}^-1 (p_i - p_{i-1}), inverse() = conjugate / |q|^2 and Eigen's q * v on the quaternion as it is.
 *       DEVIATION: the reference keeps the positions of pose_each_frame in a PointXYZI (float); the rows here are doubles throughout.
 *   (c) local graph (:3452-3527)     N poses between the two fixed anchors, started from the dead-reckoned rows 0 .. N - 1.  One left factor (measurement 0),
 *       N - 1 between factors, one right factor (measurement N); every row weighted 0.2, no loss, Ceres' QuaternionParameterization.  AS WRITTEN in the
 *       reference the between factor of poses i, i + 1 takes measurement i (paraEach[2 i], :3490-3491), not i + 1: measurement 0 is used twice and, for
 *       N >= 2, measurement N - 1 not at all.  Kept.  The loop is Ceres 1.14's trust-region minimiser (traditional DOGLEG, Jacobi scaling, mu from 1e-8,
 *       the tolerance tests before the acceptance test, monotonic), max_iterations iterations at most, entirely inside the launch.  N == 0: the
 *       reference's early return (:3457), termination GLIO_TRAJ_NOT_SOLVED.
 * THE START STATE QUIRK: the reference reads the start state P, V, R at Ps.size() - slide_window_width (:4281-4283) while the IMU index and the first frame
 * belong to keyframe size - slide_window_width - 1 (:4279, :4287) -- two different keyframes.  glio_traj_push_gap therefore takes the start state
 * explicitly; the host mirrors pass what the reference passes.
 * Every sum is formed in a fixed order and no atomic takes part: equal inputs give equal bits, alone or in a batch.
 * Pose rows are t[3], q[4] (w first), the layout glio_pgraph_append takes; measurement rows are dq[4] (w first), dp[3].
 * A glio_traj owns its streams and is not thread-safe; it touches no window context. */
#ifndef GLIO_TRAJ_H_
#define GLIO_TRAJ_H_
#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the ceiling of max_frames_per_gap: the two block-tridiagonal systems (6 x 6 blocks) of 32 poses, the vectors and the factor rows take 60 936 of the
 * 65 536 bytes of LDS a workgroup may declare statically */
#define GLIO_TRAJ_MAX_FRAMES 32

enum { GLIO_TRAJ_NO_CONVERGENCE = 0, GLIO_TRAJ_FUNCTION_TOLERANCE = 1, GLIO_TRAJ_PARAMETER_TOLERANCE = 2, GLIO_TRAJ_GRADIENT_TOLERANCE = 3,
       GLIO_TRAJ_MIN_RADIUS = 4, GLIO_TRAJ_FAILURE = 5, GLIO_TRAJ_NOT_SOLVED = 6 /* no in-between frame */ };

typedef struct glio_traj_opts {
    int32_t max_gaps;               /* 1 .. 2^20 */
    int32_t max_frames_per_gap;     /* in-between frames N of one gap, 0 .. GLIO_TRAJ_MAX_FRAMES */
    int32_t max_samples_per_gap;    /* sample rows of one gap, all segments together */
    int32_t max_iterations;         /* 15 (:3509) */
} glio_traj_opts;

typedef struct glio_traj_summary {
    int32_t termination;            /* GLIO_TRAJ_* */
    int32_t iterations;
    int32_t successful_steps;
    int32_t n_frames;               /* N */
    uint32_t accepted_mask;         /* bit k: iteration k + 1 ended with an accepted step */
    int32_t flag;                   /* 1: a non-finite value arose on the device */
    double initial_cost;
    double final_cost;
} glio_traj_summary;

typedef struct glio_traj glio_traj;

void glio_traj_opts_default(glio_traj_opts* o);       /* 4096 gaps, 32 frames, 4096 samples, 15 iterations */
/* sizeof() of glio_traj_opts, glio_traj_summary; returns how many there are (2) */
int glio_traj_struct_sizes(int32_t* out, int n);
int glio_traj_create(int device, const glio_traj_opts* opts /* null: the defaults */, glio_traj** out);
void glio_traj_destroy(glio_traj* t);

/* One gap, from raw sample rows to the solved poses.  seg_offset [n_frames + 2]: segment i is rows seg_offset[i] .. seg_offset[i + 1] - 1 of `samples`, its
 * first row the start row; start_state [15] = P[3], V[3], R[9] row major; gravity [3] (the vector g of the recurrence); prev_row, anchor_left, anchor_right
 * [7] = t, q.  Returns once the inputs are copied (pinned staging); the launch runs on the object's stream.
 * GLIO_E_ARG, and every stored gap stays as it was: gap outside [0, max_gaps), n_frames outside [0, max_frames_per_gap], more rows than
 * max_samples_per_gap, offsets that decrease or a segment without its start row, a non-finite input, a zero quaternion, dt < 0. */
int glio_traj_push_gap(glio_traj* t, int gap, int n_frames, const int32_t* seg_offset, const glio_imu_sample* samples, const double* start_state,
                       const double* gravity, const double* prev_row, const double* anchor_left, const double* anchor_right);
/* Every stored gap first_gap .. first_gap + n_gaps - 1 solved again between new anchors, n_gaps wavefronts in one launch: keyframe_poses [n_gaps + 1][7],
 * rows k and k + 1 anchor gap first_gap + k.  The reference has no such call; the initial chain is THIS LIBRARY'S CHOICE: pose 0 = left anchor (+)
 * measurement 0, pose i + 1 = pose i (+) measurement i -- the measurements the left and between factors themselves use, so that they start at zero residual.
 * The dead-reckoned rows and the measurements stay; the solved rows and the summaries are replaced.  summaries (may be null) [n_gaps]: waits for the
 * launch; a gap that ends NO_CONVERGENCE is visible there.  GLIO_E_ARG (nothing changes): a bad range, a non-finite pose, a zero quaternion.
 * GLIO_E_STATE (nothing changes): a gap of the range was never pushed. */
int glio_traj_resolve(glio_traj* t, int first_gap, int n_gaps, const double* keyframe_poses, glio_traj_summary* summaries);
/* Waits for THAT gap's last launch only.  Any output may be null: dead_reckoned [(N + 1)][7] (the last row at b's stamp), measurements [(N + 1)][7],
 * solved [N][7].  GLIO_E_STATE: never pushed.  GLIO_E_NUMERIC: the gap is flagged (glio_last_error names it; the outputs are delivered all the same);
 * pushing it again clears the flag. */
int glio_traj_read(glio_traj* t, int gap, glio_traj_summary* summary, double* dead_reckoned, double* measurements, double* solved);
/* device time of the last launch (HIP events around the kernel), ms */
int glio_traj_last_device_ms(glio_traj* t, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_TRAJ_H_ */

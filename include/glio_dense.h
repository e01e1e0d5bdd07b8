/* glio_dense.h -- the dense map on the device: the reference's full_clouds_ds (one FULL cloud per keyframe) and publishCompleteMap over it.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * WHAT IT REPLACES.  publishCompleteMap (GLIO/src/Estimator.cpp:5275-5313) maps full_clouds_ds[i]: the full cloud of keyframe i, de-skewed by the front end
 * (LidarOdometry.cpp:626), filtered by ds_filter_surf_map at 0.4 m (Estimator.cpp:854, :3623-3625), moved by q_po * q_bl, q_po * t_bl + t_po (:5287-5299) and
 * passed through ds_filter_global_map at 0.2 m (:5302-5303).  The released source comments out the push_back at :3626, so the function has nothing to read; this
 * is the function as written, with that line restored.
 *
 * A glio_dense is an object of its own, like a glio_loop or a glio_gmap: one device, its own HIP stream, its own one-slot VoxelGrid and raw staging for
 * max_input_points (1 .. GLIO_FEAT_MAX_RAW_POINTS) points.  The store is [K][max_points_per_frame] x y z intensity plus host counts.  The keyframe cycle's stream
 * is never touched: the dense work runs beside the keyframe call.  Not thread-safe by itself.
 *
 * A FRAME is pcl::VoxelGrid(leaf) of undistortion(cloud, trans, quat) -- exactly what glio_set_scan_filtered* puts into a window slot (include/glio_hip.h, "the
 * keyframe cloud": the de-skew rules, deskew_trans == NULL = no de-skew, deskew_quat == NULL = the identity, float sums in input order, PCL's output order, a
 * box of more than INT32_MAX cells passes the cloud through, leaf <= 0 copies).  There is no lidar offset: the cloud stays in the LiDAR frame, as full_clouds_ds
 * does.  One host wait per call, for the count; when the call returns a host source has been read.
 *
 * REFUSALS leave frame k, its count and the whole store exactly as they were.  GLIO_E_ARG: k outside [0, K), a bad point layout, n > max_input_points, a
 * non-finite motion, a front end on another device, more outputs than max_points_per_frame (*n_out still tells the count).  GLIO_E_STATE: a front end without an
 * extraction; glio_dense_world_cloud before any glio_dense_set_frame*.  n == 0 gives an empty frame and GLIO_OK.
 *
 * Not built: writing .pcd files, pub_map, the de-skew of edge_features, removal of frames from a map (the points of moving objects are dropped frame by frame
 * by a static store on top of this one, include/glio_static.h, and the map is built again from it). */
#ifndef GLIO_DENSE_H
#define GLIO_DENSE_H

#include "glio_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct glio_dense glio_dense;

int glio_dense_create(int device, int K, int max_points_per_frame, int max_input_points, glio_dense** out);
void glio_dense_destroy(glio_dense* d);
/* (a) host source: records of stride_bytes as glio_set_scan_strided takes them, or a packed [n][4] array */
int glio_dense_set_frame_strided(glio_dense* d, int k, const void* points, int n, int stride_bytes, int intensity_offset, float leaf, const double* deskew_trans,
                                 const double* deskew_quat, int* n_out);
int glio_dense_set_frame(glio_dense* d, int k, const float* xyzi, int n, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
/* (b) resident source: the CUT cloud (GLIO_FEAT_CUT_CLOUD: intensity = ring + 0.1 relTime, what the reference's undistortion reads) of `frontend`'s last
 * glio_features_extract*, read where it lies.  The work runs on the store's stream behind an event recorded on frontend's stream; frontend's next
 * glio_features_extract*, its glio_features_config and its glio_destroy are ordered behind the read on the device -- no host wait is added on frontend.  A
 * glio_set_scan_from_features* that reads the same front end's surf features at the same time keeps its own event: the front end comes behind both. */
int glio_dense_set_frame_from_features(glio_dense* d, int k, glio_ctx* frontend, float leaf, const double* deskew_trans, const double* deskew_quat, int* n_out);
/* frame k: [n][4] x y z intensity; *n = its size (out may be null to ask for it); capacity too small: GLIO_E_ARG.  Waits for the store's stream. */
int glio_dense_read_frame(glio_dense* d, int k, float* out_xyzi, int capacity, int* n);
int glio_dense_frame_count(glio_dense* d, int k, int* n);
/* device time of the last non-empty glio_dense_set_frame*, ms: [0] de-skew + bounding box, [1] the VoxelGrid, [2] the copy into the store -- only when
 * GLIO_DENSE_TIMING=1 was set at glio_dense_create (the events are not recorded otherwise); GLIO_E_STATE without */
int glio_dense_last_device_ms(glio_dense* d, float ms[3]);
/* pub_full_cloud_map (LidarOdometry.cpp:645-658): the last glio_dense_set_frame*'s de-skewed, UNFILTERED cloud moved by transformCloud at pose_qt = t[3], q[4]
 * (w first), stored as float: [n][4]; *n = its size (out may be null to ask for it).  The cloud is kept in the stage's staging buffer: valid until the next
 * glio_dense_set_frame*. */
int glio_dense_world_cloud(glio_dense* d, const double* pose_qt, float* out_xyzi, int capacity, int* n);

/* a global map (include/glio_hip.h, glio_gmap_*) over the store's frames instead of a batch association's: the rules of glio_gmap_create; glio_gmap_add_frames reads
 * frame frame_idx[f] of the store.  The map is ordered behind the store's pending writes by an event, and the store's next write to a frame comes behind the map's
 * read.  With poses q_po * q_bl, q_po * t_bl + t_po and leaf 0.2 this is publishCompleteMap. */
int glio_gmap_create_on_dense(glio_dense* d, const glio_gmap_opts* opts, glio_gmap** out);

#ifdef __cplusplus
}
#endif
#endif

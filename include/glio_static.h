/* glio_static.h -- the static map on the device: every point of every resident frame is tested against the range images of other frames, the points that a
 * later or earlier scan SAW THROUGH (moving objects: the trail a vehicle beside the sensor leaves in the dense map) are dropped, and the remaining points of each
 * frame are kept in a store of their own that glio_gmap_create_on_static maps exactly as rows k / p map the keyframe clouds and the dense store.  A visibility
 * rule in the manner of Removert's "remove" stage (Kim & Kim, IROS 2020); neither it nor anything like it is part of the reference tree, which maps
 * full_clouds_ds as it comes: every rule below is the library's own, UNPINNED, and restated in numpy by tests/static_map_restated.py.  Opt-in: no other entry
 * point changes, and no byte of an existing one.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * OBJECT.  A glio_static is created on a glio_bassoc (the resident keyframe clouds) or on a glio_dense (full clouds), on the owner's device with a stream of its
 * own.  Every read of the owner's clouds comes behind the owner's pending writes (an event, no host wait) and the owner's next write to a frame comes behind the
 * read (glio_bassoc_external_read / glio_dense_external_read).  It changes nothing the owner holds; the owner must outlive it.  Its own store is
 * [K][cap] x y z intensity, K and cap the owner's.  Not thread-safe.
 *
 * A CALL (glio_static_classify) names n frames f = 0 .. n-1 (indices into the owner's store), their LiDAR poses t[3], q[4] (w first) laid out as
 * glio_gmap_add_frames takes them, and per frame a list of VIEWS: call-local indices of other frames of the same call, views[view_offsets[f] .. view_offsets[f+1]).
 *
 * 1. RELATIVE POSE.  T(v, f) = pose_v^-1 o pose_f: with R the rotation matrix of q / |q|, Rrel = R_v^T R_f and trel = R_v^T (t_f - t_v), all formed in double
 *    on the host (the difference of the positions is taken in double: poses 1e6 m from the origin work) and rounded to a float 3 x 4, row major
 *    [R00 R01 R02 t0 | R10 .. | R20 ..].  ONE host function, glio_static_relative_pose, which needs no device.
 *
 * 2. RANGE IMAGE of a view v: rows x cols cells, cols = 4 cols_per_quadrant, over v's OWN points (x, y, z, .).  All arithmetic is float32, every product and
 *    sum rounded on its own (no contraction); there is no atan2f and no sqrtf.
 *      r2 = (x x + y y) + z z,  rho2 = x x + y y.  The point is SKIPPED when a coordinate is not finite, rho2 == 0, r2 < min2 or r2 >= max2
 *      (min2 = (float)(min_range^2), max2 = (float)(max_range^2), squares formed in double).
 *      row     a = z |z| (the signed square of z).  s2[k], k = 0 .. rows: with e_k = elev_min_deg + (elev_max_deg - elev_min_deg) k / rows degrees and
 *              t = tan(e_k pi / 180), s2[k] = (float)(t |t|), formed in double.  The point is out of the field of view (skipped) unless
 *              s2[0] rho2 <= a  and  a < s2[rows] rho2.  Then   lo = 0, hi = rows;  while hi - lo > 1 { mid = (lo + hi) >> 1;
 *              if (s2[mid] rho2 <= a) lo = mid; else hi = mid; }   row = lo.  (A procedure, not a count: float rounding need not be monotone.)
 *      column  quadrant q: x > 0, y >= 0 -> 0; x <= 0, y > 0 -> 1; x < 0, y <= 0 -> 2; x >= 0, y < 0 -> 3 (as glio_place.h).  dir[s] =
 *              ((float)cos, (float)sin) of 2 pi s / cols, s = 0 .. cols - 1.  lo = 0, hi = cols_per_quadrant;  while hi - lo > 1 { mid = (lo + hi) >> 1;
 *              d = dir[q cols_per_quadrant + mid]; if ((d.x y) - (d.y x) >= 0) lo = mid; else hi = mid; }   column = q cols_per_quadrant + lo.
 *      cell    the MINIMUM r2 of its points (an integer atomic min over the float's bits: all values are positive and the minimum does not depend on the
 *              order, so the bytes are reproducible).  An empty cell is +0.
 *    s2 and dir come from ONE host function, glio_static_tables, which needs no device.
 *
 * 3. FLOOR IMAGE.  F[r][c] = the minimum of the raw image over rows r - nb .. r + nb and columns c - nb .. c + nb (columns wrap), nb = neighbourhood in {0, 1}.
 *    A neighbour row outside the table, or an empty neighbour cell, makes F[r][c] = 0.  nb = 0: F is the raw image.
 *
 * 4. VOTE.  Point p = (x, y, z) of frame f against view v with T = T(v, f):  x' = ((T00 x + T01 y) + T02 z) + T03, y' and z' alike, binned by rule 2 with
 *    r2' its squared range.  When it is not skipped and F[row][column] > 0 the point is TESTED by v; when additionally F > (g2 r2') + m2 (strict), with
 *    g2 = (float)(range_gain^2) and m2 = (float)(range_margin^2) formed in double, it was SEEN THROUGH: v measured something farther in every nearby
 *    direction, so p was not there at v's time.  (r_s^2 > g^2 r_p^2 + m^2 needs no square root.)
 *
 * 5. DECISION.  through(p) and tested(p) are integer counts over the frame's views; p is DYNAMIC iff through >= min_votes.  No atomic takes part in a sum that
 *    is not an integer.
 *
 * 6. STATIC FRAME of f: its points that are not dynamic, in their original order, all four channels copied bit for bit (an order-preserving compaction with a
 *    prefix sum), into frame frame_idx[f] of the object's store, replacing what was there.  A point with a coordinate that is not finite is never tested and so
 *    is kept.  A frame without a view is copied whole.
 *
 * KERNELS.  The image of a view is built and floored in ONE workgroup's LDS when  4 rows cols + 4 (rows + 1 + 2 cols) <= 163840 bytes (the 160 KiB of a gfx950
 * compute unit; the default 44 x 360 takes 66 KB) -- no global atomic, each image written out once, raw and floored.  Above that limit (or with
 * image_path = GLIO_STATIC_PATH_GLOBAL) the cells are taken with integer atomic mins in global memory and floored by a second kernel: the same bytes.
 * The votes are one thread per point looping over its views.  One compaction launch for all frames of the call.
 * ONE host wait per glio_static_classify, at the end, for the counts (through pinned memory).
 *
 * REFUSALS are GLIO_E_ARG and leave the object's store, counts and votes exactly as they were.
 *
 * NOT BUILT: Removert's "revert" stage at finer resolutions; removing a voxel from an existing glio_gmap (the caller clears it and adds from the static store);
 * intensity-based or learned rules; range images kept across calls (glio_static_read_image holds the last call's only). */
#ifndef GLIO_STATIC_H_
#define GLIO_STATIC_H_
#include "glio_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLIO_STATIC_MAX_VIEWS 32
#define GLIO_STATIC_MAX_ROWS 256
#define GLIO_STATIC_MAX_COLS_PER_QUADRANT 512
#define GLIO_STATIC_LDS_LIMIT 163840          /* bytes: 4 rows cols + 4 (rows + 1 + 2 cols) at most for the LDS path */
#define GLIO_STATIC_PATH_AUTO 0
#define GLIO_STATIC_PATH_GLOBAL 1

typedef struct glio_static glio_static;

typedef struct glio_static_opts {
    int32_t rows;                      /* 1 .. GLIO_STATIC_MAX_ROWS; default 44 */
    int32_t cols_per_quadrant;         /* 1 .. GLIO_STATIC_MAX_COLS_PER_QUADRANT; default 90 (1 degree) */
    int32_t neighbourhood;             /* 0 or 1; default 1 */
    int32_t min_votes;                 /* 1 .. max_views; default 2 */
    int32_t max_views;                 /* views per frame, 1 .. GLIO_STATIC_MAX_VIEWS; default 16 */
    int32_t image_path;                /* GLIO_STATIC_PATH_AUTO (LDS where it fits) or GLIO_STATIC_PATH_GLOBAL; default AUTO */
    float   elev_min_deg;              /* default -31 */
    float   elev_max_deg;              /* default 13; -89 <= elev_min_deg < elev_max_deg <= 89 */
    float   min_range;                 /* m, > 0; default 1 */
    float   max_range;                 /* m, > min_range; default 80 */
    float   range_gain;                /* >= 0; default 1.05 */
    float   range_margin;              /* m, >= 0; default 0.3 */
} glio_static_opts;

typedef struct glio_static_info {
    int64_t n_points;                  /* points of the call's frames */
    int64_t n_tested;                  /* of them tested by at least one view */
    int64_t n_dynamic;                 /* of them dropped */
    int32_t n_frames;
    int32_t lds_path;                  /* 1: the images were built in LDS */
} glio_static_info;

void glio_static_opts_default(glio_static_opts* o);
/* sizeof() of glio_static_opts, glio_static_info; returns how many there are (2) */
int glio_static_struct_sizes(int32_t* out, int n);
/* s2 [rows + 1] and dir [4 cols_per_quadrant][2] of rule 2 for the options' rows, cols_per_quadrant, elev_min_deg, elev_max_deg; no device needed.
 * GLIO_E_ARG: options out of range, a null pointer */
int glio_static_tables(const glio_static_opts* opts, float* s2, float* dir);
/* T(v, f) of rule 1 from pose_v[7], pose_f[7] (t, q w first) into T[12]; no device needed.  GLIO_E_ARG: a pose that is not finite, a zero quaternion, null */
int glio_static_relative_pose(const double* pose_v, const double* pose_f, float* T);

/* GLIO_E_ARG: bad options, a null pointer */
int glio_static_create(glio_bassoc* b, const glio_static_opts* opts, glio_static** out);
int glio_static_create_on_dense(glio_dense* d, const glio_static_opts* opts, glio_static** out);
void glio_static_destroy(glio_static* st);

/* rules 1 - 6 for the owner's frames frame_idx[0 .. n): poses [n][7], view_offsets [n + 1] (view_offsets[0] = 0, ascending), views [view_offsets[n]] call-local.
 * info may be null.  GLIO_E_ARG (store, counts and votes stay as they were): n outside [1, K], a frame index out of range, a frame never set or empty, a pose
 * that is not finite or has a zero quaternion, offsets that do not start at 0 or descend, more than max_views views of a frame, a view out of [0, n) or the
 * frame itself, a frame index repeated in the call, a null pointer (views may be null only when view_offsets[n] == 0) */
int glio_static_classify(glio_static* st, int n, const int32_t* frame_idx, const double* poses, const int32_t* view_offsets, const int32_t* views,
                         glio_static_info* info);
/* static frame k: [n][4]; *n = its size (out may be null to ask for it); capacity too small: GLIO_E_ARG.  A frame never classified has size 0. */
int glio_static_read_frame(glio_static* st, int k, float* out_xyzi, int capacity, int* n);
int glio_static_frame_count(glio_static* st, int k, int* n);
/* the counts of frame k's last classification, one byte per point of the OWNER's frame at that time ([*n], capacity as above); either output may be null */
int glio_static_read_votes(glio_static* st, int k, uint8_t* through, uint8_t* tested, int capacity, int* n);
/* the last call's images of its call-local frame `view`: raw [rows][cols], floor [rows][cols]; either may be null.  GLIO_E_STATE before the first call */
int glio_static_read_image(glio_static* st, int view, float* raw, float* floor);
/* device time of the last call (HIP events), ms: [0] images (the LDS path floors in the same launch), [1] the floor kernel (0 on the LDS path), [2] votes,
 * [3] compaction; GLIO_E_STATE before the first call */
int glio_static_last_device_ms(glio_static* st, float ms[4]);

/* a global map (include/glio_hip.h, glio_gmap_*) over the STATIC store: the rules of glio_gmap_create; glio_gmap_add_frames reads static frame frame_idx[f].  A
 * frame never classified (or left without a point) reads as never set.  The map is ordered behind the store's pending writes by an event, and the next
 * glio_static_classify comes behind the map's read. */
int glio_gmap_create_on_static(glio_static* st, const glio_gmap_opts* opts, glio_gmap** out);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_STATIC_H_ */

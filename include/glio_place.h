/* glio_place.h -- place recognition on the device: a Scan Context descriptor (Kim & Kim, IROS 2018) of every resident keyframe cloud, and the EXACT
 * scan-context distance of a query place to every stored place (all 60 column shifts, every candidate, no ring-key or sector-key shortcut).  The loop
 * thread's position rule (loop.detect_candidate, Estimator.cpp:5113-5123) proposes a loop only while the drift stays below lc_search_radius; this one
 * looks at what the scans show.  Scan Context is not part of the reference tree: every rule below is the library's own, UNPINNED, and restated in numpy by
 * tests/place_restated.py.  Opt-in: no other entry point changes.
 * (A header of its own because the entry points and structs that glio_hip.h / glio_types.h declare are pinned by the existing ABI tests.)
 *
 * OBJECT.  A glio_place is created on a glio_bassoc (the resident keyframe clouds) or on a glio_dense (full clouds), on the owner's device with a stream
 * of its own.  Every read of the owner's clouds comes behind the owner's pending copies (an event, no host wait) and the owner's next write to a frame
 * comes behind the read (the owner keeps one event for all its external readers: a reader that records while another's read is pending first waits for
 * it on the device, so the owner's wait on the last record covers every reader).  It changes nothing the owner holds; the owner must outlive it.  Not thread-safe.
 *
 * DESCRIPTOR.  GLIO_PLACE_RINGS x GLIO_PLACE_SECTORS cells over the sensor's xy plane, out to max_radius.  All arithmetic below is float32, every product
 * and sum rounded on its own (no contraction), so a float32 restatement repeats it bit for bit; there is no atan2f and no sqrtf in the binning.
 *   point (x, y, z, .) of the frame; skipped when a coordinate is not finite.
 *   levelling  R = the rotation matrix of level_q (unit-normalised, formed in double on the host, stored as float; the identity for a null level_q):
 *              x' = (R00 x + R01 y) + R02 z, y' and z' alike.  The caller passes the keyframe's attitude with its yaw removed.
 *   ring       r2 = (x' x') + (y' y'); the point is skipped unless 0 < r2 < rb2[20]; ring = #{k in 1..19 : rb2[k] <= r2},
 *              rb2[k] = (float)((k max_radius / 20)^2) formed in double.
 *   sector     quadrant q: x' > 0, y' >= 0 -> 0; x' <= 0, y' > 0 -> 1; x' < 0, y' <= 0 -> 2; x' >= 0, y' < 0 -> 3;
 *              sector = 15 q + #{k in 1..14 : (d.x y') - (d.y x') >= 0 for d = dir[15 q + k]}, dir[s] = ((float)cos(2 pi s / 60), (float)sin(2 pi s / 60)).
 *   value      v = z' + lidar_height (one float add); a v that is not finite skips the point; v == 0 is stored as +0.
 *   cell       the maximum v over the cell's points (an integer atomic max over the order-preserving image of the float: the maximum does not depend on the
 *              order, so the bytes are reproducible).  A cell without a point is exactly +0.  No atomic takes part in any sum.
 *   mask       bit s of the 60-bit column mask is set when sector s holds at least one point.
 * rb2 and dir come from ONE host function, glio_place_tables, which needs no device.
 *
 * UNIT COLUMNS.  Behind the maxima the same launch forms what the query reads: per column the norm (an fp64 sum of squares over ascending ring, its square root
 * in fp64, rounded to float) and the column divided by it in float.  A column is PRESENT when its mask bit is set and its norm is positive and finite; an absent
 * column is stored as zeros.
 *
 * DISTANCE of query Q to candidate C at shift s:  1 - (sum_j cos(Q_j, C_((j + s) mod 60))) / cnt(s)  over the columns j present in Q whose partner is present
 * in C; cos is the 20-term dot product of the two unit columns, formed by five v_mfma_f32_16x16x4_f32 issues over ascending ring (the order and rounding inside
 * an issue are the instruction's own: the restatement rounds every product and sum separately and the two are held to a gate, not to the bit), the sum runs
 * over ascending j in float, cnt(s) comes from the two masks, the division and the subtraction are float.  cnt(s) = 0 gives exactly 1: no evidence is no match.  The pair's answer
 * is the smallest distance over ALL 60 shifts, the LOWEST shift on a tie.
 * SHIFT AND YAW.  yaw = shift * 2 pi / 60 (double product, rounded to float).  Shift s says: the candidate's cloud is the query's cloud turned by +yaw
 * about the sensor's z axis (counter-clockwise seen from above), p_candidate = Rz(yaw) p_query -- the query's sensor heading is the candidate's plus yaw.
 * A pair's (distance, shift) bits depend on the two descriptors only: not on what else is stored, on top_k, or on which of the two query calls asked.
 *
 * CANDIDATES of a query: every valid place other than the query itself with |time - time_query| > min_time_gap (lc_time_thres, Estimator.cpp:5119); with
 * earlier_only additionally time < time_query.  The top_k by ascending (distance, place index) are returned.
 *
 * ONE host wait per query call, at the end (the result comes through pinned memory).  glio_place_add_frames waits for nothing but the upload of the previous
 * call's argument array.  REFUSALS are GLIO_E_ARG and leave the store exactly as it was.
 *
 * NOT BUILT: a ring-key prefilter (the search is exhaustive), descriptors of other sizes, removal of a place other than by overwriting it or
 * glio_place_clear, intensity or semantic variants. */
#ifndef GLIO_PLACE_H_
#define GLIO_PLACE_H_
#include "glio_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLIO_PLACE_RINGS 20
#define GLIO_PLACE_SECTORS 60
#define GLIO_PLACE_TOP_K_MAX 8

typedef struct glio_place glio_place;

typedef struct glio_place_opts {
    int32_t max_places;                /* 1 .. 2^17; default 4096 */
    int32_t top_k_max;                 /* 1 .. GLIO_PLACE_TOP_K_MAX; default 8 */
    float   max_radius;                /* m; default 80 */
    float   lidar_height;              /* m, added to z'; default 2.0 */
} glio_place_opts;

typedef struct glio_place_match {
    int32_t place;
    int32_t shift;                     /* 0 .. 59 */
    float   distance;
    float   yaw;                       /* shift * 2 pi / 60 */
} glio_place_match;

void glio_place_opts_default(glio_place_opts* o);
/* sizeof() of glio_place_opts, glio_place_match; returns how many there are (2) */
int glio_place_struct_sizes(int32_t* out, int n);
/* rb2 [21] (rb2[0] = 0) and dir [60][2] for a max_radius; no device needed.  GLIO_E_ARG: max_radius not positive and finite, a null pointer */
int glio_place_tables(float max_radius, float* rb2, float* dir);

/* GLIO_E_ARG: bad options, a null pointer */
int glio_place_create(glio_bassoc* b, const glio_place_opts* opts, glio_place** out);
int glio_place_create_on_dense(glio_dense* d, const glio_place_opts* opts, glio_place** out);
void glio_place_destroy(glio_place* pl);

/* the descriptor of the owner's frame frame_idx[f] into place place_idx[f] with time times[f], replacing what was there; ONE launch for all n frames, one
 * workgroup per frame.  level_q [n][4] (w first) or null.  GLIO_E_ARG (the store stays as it was): n outside [1, max_places], an index out of range, a frame
 * never set or empty, a quaternion that is not finite (or zero), a time that is not finite, a place_idx repeated in the call, a null pointer */
int glio_place_add_frames(glio_place* pl, int n, const int32_t* frame_idx, const int32_t* place_idx, const double* level_q, const double* times);
/* heights [20][60] (ring major), the column mask, the time, valid (0 / 1); any output may be null.  An invalid place reads as zeros. */
int glio_place_read_descriptor(glio_place* pl, int place, float* heights, uint64_t* mask, double* time, int32_t* valid);
/* a host descriptor into a place, through the same normalisation as glio_place_add_frames.  GLIO_E_ARG (the store stays): place out of range, a height or
 * the time not finite, a mask bit above 59, a null pointer */
int glio_place_set_descriptor(glio_place* pl, int place, const float* heights, uint64_t mask, double time);
/* every place invalid */
int glio_place_clear(glio_place* pl);

/* the top_k candidates of `place` into matches [top_k]; *n_found of them are written (the rest of `matches` is untouched).
 * GLIO_E_ARG: place out of range or not valid, top_k outside [1, top_k_max], min_time_gap negative or not finite, a null pointer */
int glio_place_query(glio_place* pl, int place, double min_time_gap, int top_k, glio_place_match* matches, int32_t* n_found);
/* the same for the places first .. first + n - 1 in one call: matches [n][top_k], n_found [n].  A place of the range that is not valid finds nothing. */
int glio_place_query_many(glio_place* pl, int first, int n, double min_time_gap, int earlier_only, int top_k, glio_place_match* matches, int32_t* n_found);
/* device time of the last add_frames / query call (HIP events), ms; GLIO_E_STATE before the first */
int glio_place_last_device_ms(glio_place* pl, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* GLIO_PLACE_H_ */

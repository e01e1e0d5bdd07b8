"""Place recognition: the device object (glio_place_*, include/glio_place.h, csrc/place_kernels.hip: a Scan Context descriptor of every resident keyframe
cloud and the exact scan-context distance of a query to every stored place) and the host's share -- the attitude with its yaw removed that levels a cloud
(leveling_quaternion), the candidate rule that stands beside loop.detect_candidate in the loop thread (detect_candidate_by_appearance) and the pose the source
submap is built at so that the ICP starts from the yaw the descriptor found (initial_guess, rebase_poses).  `glio::PlaceRecognition`,
`glio::levelingQuaternion`, `glio::detectCandidateByAppearance` and `glio::placeInitialGuess` (host/glio_place_backend.hpp) are the C++ twins: the same scalar
arithmetic in the same order.  There is no CPU fallback for the descriptor or the search."""
import ctypes as C
import math

import numpy as np

from . import capi
from . import ctypes_types as T
from .loop import LOOP_TIME_GATE

RINGS, SECTORS, TOP_K_MAX = T.PLACE_RINGS, T.PLACE_SECTORS, T.PLACE_TOP_K_MAX
MATCH_DTYPE = np.dtype([("place", "<i4"), ("shift", "<i4"), ("distance", "<f4"), ("yaw", "<f4")])
DISTANCE_THRESHOLD = 0.2                # the yaml-style threshold detect_candidate_by_appearance defaults to

default_opts = capi.place_opts


class PlaceRecognition:
    """One glio_place on a batch.BatchAssociation or a mapping.DenseClouds (which owns the resident clouds and must outlive this object).  The caller keeps
    keyframe i at place i, so a match's `place` is the keyframe index loop.submap_frames takes."""

    def __init__(self, owner, opts=None, **kw):
        from .mapping import DenseClouds
        lib = capi.load()
        self.opts = default_opts(**kw) if opts is None else opts
        self._owner = owner
        self._h = C.c_void_p()
        create = lib.glio_place_create_on_dense if isinstance(owner, DenseClouds) else lib.glio_place_create
        capi._check(create(owner._h, C.byref(self.opts), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_place_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_frames(self, frames, places, times, level_q=None):
        """the descriptors of the owner's frames `frames` into the places `places` with `times`, one launch.  level_q [n][4] (w first) or None.  A refusal
        (GlioError) leaves the store exactly as it was."""
        frames, places = np.ascontiguousarray(frames, np.int32).reshape(-1), np.ascontiguousarray(places, np.int32).reshape(-1)
        times = np.ascontiguousarray(times, np.float64).reshape(-1)
        assert len(frames) == len(places) == len(times)
        lq = None
        if level_q is not None:
            lq = np.ascontiguousarray(level_q, np.float64).reshape(-1, 4)
            assert len(lq) == len(frames)
        n = len(frames)
        capi._check(capi.load().glio_place_add_frames(self._h, n, T.iptr(frames) if n else None, T.iptr(places) if n else None,
                                                      T.dptr(lq) if lq is not None and n else None, T.dptr(times) if n else None))

    def read_descriptor(self, place):
        """(heights [20][60] float32, mask, time, valid)"""
        h = np.zeros((RINGS, SECTORS), np.float32)
        mask, t, valid = C.c_uint64(0), C.c_double(0), C.c_int32(0)
        capi._check(capi.load().glio_place_read_descriptor(self._h, int(place), T.fptr(h), C.byref(mask), C.byref(t), C.byref(valid)))
        return h, int(mask.value), float(t.value), bool(valid.value)

    def set_descriptor(self, place, heights, mask, time):
        h = np.ascontiguousarray(heights, np.float32).reshape(RINGS, SECTORS)
        capi._check(capi.load().glio_place_set_descriptor(self._h, int(place), T.fptr(h), int(mask), float(time)))

    def clear(self):
        capi._check(capi.load().glio_place_clear(self._h))

    def query(self, place, min_time_gap, top_k=1):
        """the top_k candidates of `place` by ascending (distance, place): a MATCH_DTYPE array of the matches found"""
        m = (T.GlioPlaceMatch * int(top_k))()
        n = C.c_int32(0)
        capi._check(capi.load().glio_place_query(self._h, int(place), float(min_time_gap), int(top_k), m, C.byref(n)))
        return np.frombuffer(bytes(m), MATCH_DTYPE)[:n.value].copy()

    def query_many(self, first, n, min_time_gap, earlier_only=False, top_k=1):
        """places first .. first + n - 1 in one call: (MATCH_DTYPE [n][top_k], n_found [n]); rows beyond n_found are zero"""
        n, top_k = int(n), int(top_k)
        m = (T.GlioPlaceMatch * (n * top_k))()
        nf = np.zeros(n, np.int32)
        capi._check(capi.load().glio_place_query_many(self._h, int(first), n, float(min_time_gap), 1 if earlier_only else 0, top_k, m, T.iptr(nf)))
        return np.frombuffer(bytes(m), MATCH_DTYPE).reshape(n, top_k).copy(), nf

    def last_device_ms(self):
        ms = C.c_float(0)
        capi._check(capi.load().glio_place_last_device_ms(self._h, C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------ the host's share (scalar arithmetic, mirrored in glio_place_backend.hpp)
def _qmul(a, b):
    """Eigen's quaternion product, (w, x, y, z) (place_detail::qmul)"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def _qinv(q):
    """conjugate / squaredNorm"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2]


def _qrot(q, v):
    """Eigen's quaternion * vector: v + w (2 u x v) + u x (2 u x v)"""
    w, x, y, z = q
    uv = [y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    uuv = [y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]]
    return [v[0] + w * uv[0] + uuv[0], v[1] + w * uv[1] + uuv[1], v[2] + w * uv[2] + uuv[2]]


def _yaw_of(q):
    """the yaw of the ZYX Euler angles of q (w, x, y, z)"""
    w, x, y, z = [float(v) for v in q]
    return math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def _qz(yaw):
    return [math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw)]


def leveling_quaternion(q):
    """the attitude q (w, x, y, z) with its yaw removed, qz(-yaw(q)) * q: what glio_place_add_frames takes as level_q -- roll and pitch are taken out of the
    cloud, the heading stays what the descriptor's column shift measures"""
    q = [float(v) for v in q]
    return np.array(_qmul(_qz(-_yaw_of(q)), q))


def detect_candidate_by_appearance(pr, query_place, time_thres, time_new_odom, time_last_loop, dist_thres=DISTANCE_THRESHOLD):
    """The appearance rule beside loop.detect_candidate: the stored place closest to `query_place` in scan-context distance among those more than time_thres
    away in time (Estimator.cpp:5119), taken when its distance is below dist_thres.  Returns (closest, yaw, distance); closest = -1 (yaw 0) when there is no
    such place or |time_last_loop - time_new_odom| < 0.2 (:5127).  closest is the place index = the keyframe index loop.submap_frames takes."""
    m = pr.query(query_place, time_thres, 1)
    if len(m) == 0 or not float(m[0]["distance"]) < float(dist_thres):
        return -1, 0.0, float(m[0]["distance"]) if len(m) else float("inf")
    if abs(float(time_last_loop) - float(time_new_odom)) < LOOP_TIME_GATE:
        return -1, 0.0, float(m[0]["distance"])
    return int(m[0]["place"]), float(m[0]["yaw"]), float(m[0]["distance"])


def initial_guess(pose_closest, yaw, q_query=None):
    """The pose (t[3], q[4] w first) to build the query keyframe's cloud at so that it lies on the closest keyframe's: the closest keyframe's position, and the
    heading the match found -- p_closest = Rz(yaw) p_query between the levelled clouds.  Without q_query both attitudes are taken as level: q = q_closest * qz(yaw).
    With q_query (the query keyframe's attitude, whose level_q was leveling_quaternion(q_query)): q = qz(yaw(q_closest) + yaw) * leveling_quaternion(q_query)."""
    pc = [float(v) for v in pose_closest]
    if q_query is None:
        q = _qmul(pc[3:], _qz(float(yaw)))
    else:
        q = _qmul(_qz(_yaw_of(pc[3:]) + float(yaw)), [float(v) for v in leveling_quaternion(q_query)])
    return np.array(pc[:3] + q)


def rebase_poses(poses, pose_from, pose_to):
    """poses [n][7] (t, q) moved by the rigid motion that takes pose_from to pose_to: the source submap's other keyframes keep their place relative to the query
    keyframe when that one is put at initial_guess.  q' = (q_to * q_from^-1) * q, t' = (q_to * q_from^-1) (t - t_from) + t_to."""
    pf, pt = [float(v) for v in pose_from], [float(v) for v in pose_to]
    dq = _qmul(pt[3:], _qinv(pf[3:]))
    out = []
    for p in np.asarray(poses, np.float64).reshape(-1, 7):
        p = [float(v) for v in p]
        r = _qrot(dq, [p[0] - pf[0], p[1] - pf[1], p[2] - pf[2]])
        out.append([r[0] + pt[0], r[1] + pt[1], r[2] + pt[2]] + _qmul(dq, p[3:]))
    return np.array(out)

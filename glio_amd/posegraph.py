"""The pose graph: the device object (glio_pgraph_*, csrc/posegraph_kernels.hip -- what the reference keeps in one gtsam::ISAM2: the global graph of
Estimator.cpp:4586-4652, :5251-5256 and the local graph of :4561-4581) and the host's share of it, restated as plain arithmetic the way loop.py restates the
loop thread: which frames enter the global graph at a keyframe call (:4610-4611), the loop edge between frame ids (:5251-5252), addLIOFactor's node per
keyframe that left the window (:1999-2043) and every gate of addGNSSFactor (:1915-1997).  `glio::PoseGraph`, `glio::globalGraphFrames`, `glio::GnssGate`
(host/glio_posegraph_backend.hpp) are the C++ twins.  The factor definitions, the two stated deviations from GTSAM / iSAM2 and the termination are in
include/glio_hip.h.  PoseGraph.read_poses() hands back rows t[3], q[4] -- what loop.correct_window_poses (after its q, t reordering), Context.
localmap_rebuild_from_frames, loop.LoopClosure.build_submap and mapping.GlobalMap.add take (through loop.frame_poses where the LiDAR offset applies).
There is no CPU fallback."""
import ctypes as C
import math

import numpy as np

from . import capi
from . import ctypes_types as T

GNSS_SPACING = 5.0                      # Estimator.cpp:1932, :1980
GNSS_TIME_WINDOW = 0.2                  # :1950-1954
GNSS_COV_THRESHOLD = 200.0              # :237
POSE_COV_THRESHOLD = 1.0                # :238


def default_opts(**kw):
    """glio_pgraph_opts: the reference's noise variances (Estimator.cpp:864-865, :1986), GaussNewtonParams' termination, capacities; keywords override fields"""
    lib = capi.load()
    lib.glio_pgraph_opts_default.restype = None
    o = T.GlioPgraphOpts()
    lib.glio_pgraph_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def fixed_iterations(n, **kw):
    """options under which a solve runs exactly n iterations: no relative test, and an absolute threshold no decrease reaches"""
    return default_opts(max_iterations=int(n), relative_error_tol=0.0, absolute_error_tol=-1e300, **kw)


class SolveInfo:
    def __init__(self, r):
        self.iterations, self.termination = int(r.iterations), int(r.termination)
        self.initial_error, self.final_error = float(r.initial_error), float(r.final_error)
        self.separators, self.segments = int(r.separators), int(r.segments)
        self.device_ms, self.stage_ms = float(r.device_ms), [float(x) for x in r.stage_ms]

    @property
    def termination_name(self):
        return T.PGRAPH_LM_TERMINATION_NAMES[self.termination]

    def as_dict(self):
        return dict(iterations=self.iterations, termination=self.termination_name, initial_error=self.initial_error, final_error=self.final_error,
                    separators=self.separators, segments=self.segments, device_ms=self.device_ms, stage_ms=self.stage_ms)


def default_lm_opts(**kw):
    """glio_pgraph_lm_opts: Ceres 1.14's LevenbergMarquardtStrategy defaults; keywords override fields"""
    lib = capi.load()
    lib.glio_pgraph_lm_opts_default.restype = None
    o = T.GlioPgraphLmOpts()
    lib.glio_pgraph_lm_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class DampedSolveInfo(SolveInfo):
    """SolveInfo (iterations = trials) with glio_pgraph_lm_info and the per-trial history [trials][4]: E tried, the radius used, the model decrease,
    1 accepted / 0 rejected / -1 invalid"""

    def __init__(self, r, lm, history):
        SolveInfo.__init__(self, r)
        self.final_radius = float(lm.final_radius)
        self.accepted, self.rejected, self.invalid, self.trials = int(lm.accepted), int(lm.rejected), int(lm.invalid), int(lm.trials)
        self.history = history

    def as_dict(self):
        return dict(SolveInfo.as_dict(self), final_radius=self.final_radius, accepted=self.accepted, rejected=self.rejected, invalid=self.invalid, trials=self.trials,
                    verdicts=[int(v) for v in self.history[:, 3]])


def _p7(a):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    assert a.size == 7
    return a


class PoseGraph:
    """One glio_pgraph.  Poses are rows t[3], q[4] (w first); variances are in the tangent order of the header: rotation first."""

    def __init__(self, opts=None, device=0):
        lib = capi.load()
        lib.glio_pgraph_destroy.restype = None
        self.opts = default_opts() if opts is None else opts
        self._h = C.c_void_p()
        capi._check(lib.glio_pgraph_create(int(device), C.byref(self.opts), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_pgraph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        capi._check(capi.load().glio_pgraph_clear(self._h))

    def set_prior(self, pose, var=None):
        v = None if var is None else np.ascontiguousarray(var, np.float64).reshape(6)
        capi._check(capi.load().glio_pgraph_set_prior(self._h, T.dptr(_p7(pose)), None if v is None else T.dptr(v)))

    def append(self, poses, prev_pose=None, var=None):
        """nodes at the end with `poses` as initial estimates, one between factor each (the first node of an empty graph none); prev_pose: the caller's pose of the
        current last node (None: its current estimate)"""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        v = None if var is None else np.ascontiguousarray(var, np.float64).reshape(6)
        capi._check(capi.load().glio_pgraph_append(self._h, len(poses), T.dptr(poses) if len(poses) else None, None if prev_pose is None else T.dptr(_p7(prev_pose)),
                                                   None if v is None else T.dptr(v)))

    def add_between(self, i, j, rel, var):
        capi._check(capi.load().glio_pgraph_add_between(self._h, int(i), int(j), T.dptr(_p7(rel)), T.dptr(np.ascontiguousarray(var, np.float64).reshape(6))))

    def add_gps(self, i, xyz, var):
        capi._check(capi.load().glio_pgraph_add_gps(self._h, int(i), T.dptr(np.ascontiguousarray(xyz, np.float64).reshape(3)),
                                                    T.dptr(np.ascontiguousarray(var, np.float64).reshape(3))))

    def solve(self):
        r = T.GlioPgraphInfo()
        capi._check(capi.load().glio_pgraph_solve(self._h, C.byref(r)))
        return SolveInfo(r)

    def solve_damped(self, lm_opts=None):
        """glio_pgraph_solve_damped: the solve that never leaves a worse estimate (lm_opts None: the defaults); returns DampedSolveInfo"""
        lib = capi.load()
        r, lm = T.GlioPgraphInfo(), T.GlioPgraphLmInfo()
        capi._check(lib.glio_pgraph_solve_damped(self._h, None if lm_opts is None else C.byref(lm_opts), C.byref(r), C.byref(lm)))
        hist = np.zeros((lm.trials, 4))
        capi._check(lib.glio_pgraph_lm_history(self._h, 0, int(lm.trials), T.dptr(hist) if lm.trials else None))
        return DampedSolveInfo(r, lm, hist)

    def size(self):
        n = C.c_int(0)
        capi._check(capi.load().glio_pgraph_size(self._h, C.byref(n)))
        return n.value

    def read_poses(self, first=0, n=None):
        n = self.size() - int(first) if n is None else int(n)
        out = np.zeros((max(n, 0), 7))
        capi._check(capi.load().glio_pgraph_read_poses(self._h, int(first), n, T.dptr(out) if n > 0 else None))
        return out

    def marginal_covariance(self, node):
        out = np.zeros((6, 6))
        capi._check(capi.load().glio_pgraph_marginal_covariance(self._h, int(node), T.dptr(out)))
        return out

    def marginal_covariances(self, next=False, with_info=False):
        """glio_pgraph_covariance_all (include/glio_pgraph_cov.h): block (i, i) of (J^T J)^-1 for EVERY node from one factorisation, [N][6][6] in the tangent
        frame of the retraction (rotation first); next=True: also the blocks (i, i + 1), [N - 1][6][6]; with_info: also the glio_pgraph_cov_info as a dict.
        A pivot that is not positive and finite raises GlioError with code E_NUMERIC and `info` (bad_node names the node)."""
        n = self.size()
        diag = np.zeros((max(n, 1), 6, 6))[:n]           # (an empty graph still hands over an address: the refusal is the library's)
        nxt = np.zeros((max(n, 2) - 1, 6, 6))[:max(n - 1, 0)] if next else None
        info = T.GlioPgraphCovInfo()
        rc = capi.load().glio_pgraph_covariance_all(self._h, T.dptr(diag), T.dptr(nxt) if next else None, C.byref(info))
        if rc != 0:
            e = capi.GlioError(f"libglio_hip error {rc}: {capi.load().glio_last_error().decode()}")
            e.code, e.info = rc, info.as_dict()
            raise e
        out = (diag, nxt) if next else (diag,)
        out = out + (info.as_dict(),) if with_info else out
        return out[0] if len(out) == 1 else out

    def marginal_covariances_dev(self):
        """(device address of diag [n][36], device address of next [n - 1][36], n): valid until the next call that changes the graph or asks again"""
        d, x, n = C.c_void_p(), C.c_void_p(), C.c_int(0)
        capi._check(capi.load().glio_pgraph_covariance_all_dev(self._h, C.byref(d), C.byref(x), C.byref(n)))
        return d.value, x.value, n.value

    def marginal_covariances_ms(self):
        """(device ms of the last marginal_covariances call, its five stages: linearise, segments + separator factor, separator inversion, down-sweep, copy)"""
        ms, st = C.c_float(0), (C.c_float * 5)()
        capi._check(capi.load().glio_pgraph_covariance_all_last_device_ms(self._h, C.byref(ms)))
        capi._check(capi.load().glio_pgraph_covariance_all_last_stage_ms(self._h, st))
        return float(ms.value), [float(v) for v in st]

    def error(self):
        e = C.c_double(0)
        capi._check(capi.load().glio_pgraph_error(self._h, C.byref(e)))
        return e.value

    def poses_dev(self):
        """(device address of the [n][7] float64 pose table, n): valid until the next successful solve / append / clear"""
        p, n = C.c_void_p(), C.c_int(0)
        capi._check(capi.load().glio_pgraph_poses_dev(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value


# ---------------------------------------------------------------------------------------------------------------- the host's share: the global graph
def global_graph_frames(keyframe_id_in_frame, n_keyframes, W):
    """Estimator.cpp:4589-4611: the frame ids that enter the global graph at the keyframe call that sees n_keyframes keyframes (W = slide_window_width).
    n_keyframes < W: none.  == W: frame 0 alone (with the prior, :4592-4594).  > W: keyframe_id_in_frame[n - W - 1] + 1 .. keyframe_id_in_frame[n - W]."""
    n, W = int(n_keyframes), int(W)
    if n < W:
        return []
    if n == W:
        return [0]
    return list(range(int(keyframe_id_in_frame[n - W - 1]) + 1, int(keyframe_id_in_frame[n - W]) + 1))


def loop_edge_frames(keyframe_id_in_frame, latest_keyframe, closest_keyframe):
    """Estimator.cpp:5251-5252: the loop's between factor joins FRAME ids"""
    return int(keyframe_id_in_frame[int(latest_keyframe)]), int(keyframe_id_in_frame[int(closest_keyframe)])


class GlobalGraph:
    """The global graph's bookkeeping on a PoseGraph: one node per frame, fed per keyframe call (:4586-4652)."""

    def __init__(self, graph, W):
        self.graph, self.W = graph, int(W)

    def keyframe_call(self, pose_each_frame, keyframe_id_in_frame, n_keyframes):
        """pose_each_frame [F][7] = t, q of every frame so far.  Adds what :4589-4637 adds; returns the frame ids added."""
        ids = global_graph_frames(keyframe_id_in_frame, n_keyframes, self.W)
        if not ids:
            return ids
        P = np.asarray(pose_each_frame, np.float64).reshape(-1, 7)
        if ids == [0] and self.graph.size() == 0:
            self.graph.set_prior(P[0])
            self.graph.append(P[0:1])
            return ids
        assert ids[0] == self.graph.size(), (ids[0], self.graph.size())
        self.graph.append(P[ids[0]:ids[-1] + 1], prev_pose=P[ids[0] - 1])
        return ids

    def loop_closed(self, keyframe_id_in_frame, latest_keyframe, closest_keyframe, constraint, damped=False):
        """constraint = loop.loop_constraint(...) = (rel [7], var [6]); adds the edge (:5251-5254), solves (:5255-5261); returns SolveInfo.
        damped: PoseGraph.solve_damped instead (DampedSolveInfo) -- the call for a loop over a long drive, where the undamped step can raise the error"""
        i, j = loop_edge_frames(keyframe_id_in_frame, latest_keyframe, closest_keyframe)
        self.graph.add_between(i, j, constraint[0], constraint[1])
        return self.graph.solve_damped() if damped else self.graph.solve()

    def keyframe_poses(self, keyframe_id_in_frame, n):
        """pose_each_frame[keyframe_id_in_frame[i]] of the corrected estimate for keyframes 0 .. n - 1 (correctPoses, :4702-4713): rows t, q"""
        ids = np.asarray(keyframe_id_in_frame[:int(n)], np.int64)
        return self.graph.read_poses()[ids]


# ---------------------------------------------------------------------------------------------------------------- the host's share: the local graph
def _f32(x):
    return np.float32(x)


def point_distance_f32(a, b):
    """pointDistance(PointType, PointType) (:1570-1573): float differences, products and sum, the square root in double"""
    a, b = [np.float32(v) for v in a], [np.float32(v) for v in b]
    d = [a[k] - b[k] for k in range(3)]
    s = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])
    return math.sqrt(float(np.float32(s)))


def point_distance_f64(a, b):
    """pointDistance(PointPoseInfo, PointPoseInfo) (:1575-1578)"""
    return math.sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]))


class GnssGate:
    """addGNSSFactor (:1915-1997) without GTSAM: decides whether the keyframe that just left the window gets a GPS factor, and which.
    The queue holds (stamp, xyz[3], cov[3]) oldest first (nav_msgs::Odometry: pose.pose.position, pose.covariance[0..2]) and is consumed as the reference does."""

    def __init__(self, timeshift=0.0, gnss_cov_threshold=GNSS_COV_THRESHOLD, pose_cov_threshold=POSE_COV_THRESHOLD):
        self.timeshift, self.gnss_cov_threshold, self.pose_cov_threshold = float(timeshift), float(gnss_cov_threshold), float(pose_cov_threshold)
        self.last_add_pos = (0.0, 0.0, 0.0)              # last_GNSS_add_pos (:499-501)
        self.last_gps_point = (0.0, 0.0, 0.0)            # static PointType lastGPSPoint (:1943)
        self.queue = []

    def push(self, stamp, xyz, cov):
        self.queue.append((float(stamp), tuple(float(v) for v in xyz), tuple(float(v) for v in cov)))

    def select(self, n_keyframes, W, keyframe_xyz, keyframe_time, pose_cov):
        """keyframe_xyz / keyframe_time: pose_info_keyframe[proc_kf_idx] of proc_kf_idx = n_keyframes - W; pose_cov: the 6x6 poseCovariance.  Returns None or
        (proc_kf_idx, xyz [3], variances [3]) -- what PoseGraph.add_gps takes; max(noise, 1) is applied here as at :1986 (and again, idempotently, by the library)."""
        n, W = int(n_keyframes), int(W)
        if n <= W:                                                                      # :1918
            return None
        idx = n - W
        if not self.queue:                                                              # :1922
            return None
        if point_distance_f64(self.last_add_pos, keyframe_xyz) < GNSS_SPACING:          # :1932
            return None
        pc = np.asarray(pose_cov, np.float64).reshape(6, 6)
        if pc[3, 3] < self.pose_cov_threshold and pc[4, 4] < self.pose_cov_threshold:   # :1938
            return None
        t = float(keyframe_time) + self.timeshift                                       # :1946
        while self.queue:
            stamp, xyz, cov = self.queue[0]
            if stamp < t - GNSS_TIME_WINDOW:                                            # :1950
                self.queue.pop(0)
            elif stamp > t + GNSS_TIME_WINDOW:                                          # :1954
                break
            else:
                self.queue.pop(0)
                nx, ny, nz = _f32(cov[0]), _f32(cov[1]), _f32(cov[2])                    # float noise_x ... (:1964-1966)
                if float(nx) > self.gnss_cov_threshold or float(ny) > self.gnss_cov_threshold:     # :1967
                    continue
                g = tuple(float(_f32(v)) for v in xyz)                                   # float gps_x ... (:1971-1973)
                if point_distance_f32(g, self.last_gps_point) < GNSS_SPACING:           # :1980
                    continue
                self.last_gps_point = g
                var = [float(max(v, _f32(1.0))) for v in (nx, ny, nz)]                   # :1986
                self.last_add_pos = tuple(float(v) for v in keyframe_xyz)               # :1992
                return idx, list(g), var
        return None


class LocalGraph:
    """The local graph's bookkeeping on a PoseGraph: one node per keyframe that left the window (addLIOFactor, :1999-2043), GPS factors through a GnssGate,
    the solve and poseCovariance of :4572-4579."""

    def __init__(self, graph, W, gate=None):
        self.graph, self.W, self.gate = graph, int(W), gate if gate is not None else GnssGate()
        self.pose_cov = np.zeros((6, 6))                 # Eigen::MatrixXd poseCovariance before the first solve: the covariance gate is closed

    def keyframe_call(self, pose_info_keyframe, keyframe_time, n_keyframes):
        """pose_info_keyframe [n][7] = t, q.  Returns (node added or None, GPS factor added or None, SolveInfo or None)."""
        n = int(n_keyframes)
        if n < self.W:                                                                   # :4563
            return None, None, None
        P = np.asarray(pose_info_keyframe, np.float64).reshape(-1, 7)
        idx = n - self.W
        if n == self.W:                                                                  # :2003-2015
            self.graph.set_prior(P[0])
            self.graph.append(P[0:1])
        else:                                                                            # :2018-2041
            assert idx == self.graph.size(), (idx, self.graph.size())
            self.graph.append(P[idx:idx + 1], prev_pose=P[idx - 1])
        gps = self.gate.select(n, self.W, P[idx, :3], keyframe_time[idx], self.pose_cov)
        if gps is not None:
            self.graph.add_gps(*gps)
        info = self.graph.solve()                                                        # :4566-4577
        self.pose_cov = self.graph.marginal_covariance(self.graph.size() - 1)            # :4578
        return idx, gps, info

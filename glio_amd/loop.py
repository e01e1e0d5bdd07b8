"""Loop closure: the device object (glio_loop_*, csrc/loop_kernels.hip: detectLoopClosure's submaps from the resident keyframe clouds of a
batch association and performLoopClosure's ICP, Estimator.cpp:5101-5273) and the host's share of the same thread -- which keyframe closes the
loop (:5113-5128), which keyframes make the two submaps (:5133-5175), their poses (:5147-5148), and the relative pose handed to the pose graph
(:5210-5247).  `glio::LoopClosure`, `glio::detectLoopCandidate`, `glio::loopSubmapFrames`, `glio::loopFramePoses` and `glio::loopConstraint`
(host/glio_loop_backend.hpp) are the C++ twins: the same scalar arithmetic in the same order, so the two hosts agree bit for bit
(tests/test_loop_host_cpu.py).  Of correctPoses (:4658-4787) the window's share is here too -- correct_window_poses / glio::correctWindowPoses: the
relative poses inside the sliding window taken before the correction, the older keyframes set to the caller's corrected poses, the window chained back on,
Rs / Ps -- and its recent_surf_keyframes.clear() is sliding.ReferenceMapSchedule.loop_closed() (the next call rebuilds the local map from the resident
keyframes at the corrected poses, glio_localmap_rebuild_from_frames).  The corrected poses themselves come from posegraph.GlobalGraph (glio_pgraph_*: the pose graph
on the device; a caller may keep GTSAM / iSAM2 instead); pose_each_frame and the prior reset
(:5249-5269, :4785 marg = false: glio_set_prior(NULL)) stay with the caller.  There is no CPU fallback for the submaps or the registration."""
import ctypes as C
import math

import numpy as np

from . import capi
from . import ctypes_types as T

SOURCE, TARGET = T.LOOP_SOURCE, T.LOOP_TARGET
LATEST_FRAMES = 6                       # Estimator.cpp:5135
LOOP_TIME_GATE = 0.2                    # :5127


def default_opts(**kw):
    """glio_loop_opts of Estimator.cpp:855, :5197-5200 and PCL 1.8.1's defaults; keyword arguments override fields"""
    lib = capi.load()
    lib.glio_loop_opts_default.restype = None
    o = T.GlioLoopOpts()
    lib.glio_loop_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


class LoopResult:
    def __init__(self, r):
        self.converged, self.state, self.iterations = bool(r.converged), int(r.state), int(r.iterations)
        self.fitness, self.last_mse, self.last_n_corr, self.rank_deficient = float(r.fitness), float(r.last_mse), int(r.last_n_corr), bool(r.rank_deficient)
        self.transform = np.array(r.transform, np.float32).reshape(4, 4)

    @property
    def state_name(self):
        return T.LOOP_STATE_NAMES[self.state]

    def as_dict(self):
        return dict(converged=self.converged, state=self.state_name, iterations=self.iterations, fitness=self.fitness, last_mse=self.last_mse,
                    last_n_corr=self.last_n_corr, rank_deficient=self.rank_deficient, transform=self.transform.tolist())


class LoopStep:
    def __init__(self, r):
        self.n_corr, self.mse, self.state, self.n_fallback, self.rank_deficient = int(r.n_corr), float(r.mse), int(r.state), int(r.n_fallback), bool(r.rank_deficient)
        self.transform = np.array(r.transform, np.float32).reshape(4, 4)


class LoopClosure:
    """One glio_loop on a batch.BatchAssociation (which owns the resident keyframe clouds)."""

    def __init__(self, assoc, opts=None):
        lib = capi.load()
        lib.glio_loop_destroy.restype = None
        self.opts = default_opts() if opts is None else opts
        self._assoc = assoc             # (the association must outlive the loop object)
        self._h = C.c_void_p()
        capi._check(lib.glio_loop_create(assoc._h, C.byref(self.opts), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_loop_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_submap(self, which, frames, poses):
        """frames: resident keyframe indices in list order; poses [n][7] = t, q (frame_poses).  Returns the filtered submap's size."""
        frames = np.ascontiguousarray(frames, np.int32)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        assert len(poses) == len(frames)
        n = C.c_int(0)
        capi._check(capi.load().glio_loop_build_submap(self._h, int(which), len(frames), T.iptr(frames) if len(frames) else None,
                                                       T.dptr(poses) if len(frames) else None, C.byref(n)))
        return n.value

    def set_submap(self, which, xyzi):
        xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        capi._check(capi.load().glio_loop_set_submap(self._h, int(which), T.fptr(xyzi) if len(xyzi) else None, len(xyzi)))

    def read_submap(self, which):
        n = C.c_int(0)
        capi._check(capi.load().glio_loop_read_submap(self._h, int(which), None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            capi._check(capi.load().glio_loop_read_submap(self._h, int(which), T.fptr(out), n.value, C.byref(n)))
        return out

    def align(self):
        r = T.GlioLoopResult()
        capi._check(capi.load().glio_loop_align(self._h, C.byref(r)))
        return LoopResult(r)

    def reset_current(self):
        capi._check(capi.load().glio_loop_reset_current(self._h))

    def step(self):
        r = T.GlioLoopStepResult()
        capi._check(capi.load().glio_loop_step(self._h, C.byref(r)))
        return LoopStep(r)

    def read_correspondences(self, n_source):
        idx, d2 = np.zeros(n_source, np.int32), np.zeros(n_source, np.float32)
        capi._check(capi.load().glio_loop_read_correspondences(self._h, T.iptr(idx), T.fptr(d2)))
        return idx, d2

    def read_current(self):
        n = C.c_int(0)
        capi._check(capi.load().glio_loop_read_current(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.float32)
        if n.value:
            capi._check(capi.load().glio_loop_read_current(self._h, T.fptr(out), n.value, C.byref(n)))
        return out

    def fallbacks(self):
        """queries the brute-force scan answered, per round of the last align, then for the fitness search"""
        n = C.c_int(0)
        capi._check(capi.load().glio_loop_read_fallbacks(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int32)
        if n.value:
            capi._check(capi.load().glio_loop_read_fallbacks(self._h, T.iptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def last_device_ms(self):
        ms = C.c_float(0)
        capi._check(capi.load().glio_loop_last_device_ms(self._h, C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------ the host's share (scalar arithmetic, mirrored in glio_loop_backend.hpp)
def _qmul(a, b):
    """Eigen's quaternion product, (w, x, y, z)"""
    return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]


def _qrot(q, v):
    """Eigen's quaternion * vector: v + w (2 u x v) + u x (2 u x v)"""
    w, x, y, z = q
    uv = [y * v[2] - z * v[1], z * v[0] - x * v[2], x * v[1] - y * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    uuv = [y * uv[2] - z * uv[1], z * uv[0] - x * uv[2], x * uv[1] - y * uv[0]]
    return [v[0] + w * uv[0] + uuv[0], v[1] + w * uv[1] + uuv[1], v[2] + w * uv[2] + uuv[2]]


def eigen_R2q(R):
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), (w, x, y, z).  synth.R2q is the same rule
    followed by a flip to w >= 0 and a normalisation, which Eigen does not do; this one stops where Eigen stops."""
    m = [[float(R[r][c]) for c in range(3)] for r in range(3)]
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2][1] - m[1][2]) * t
        q[2] = (m[0][2] - m[2][0]) * t
        q[3] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k][j] - m[j][k]) * t
        q[1 + j] = (m[j][i] + m[i][j]) * t
        q[1 + k] = (m[k][i] + m[i][k]) * t
    return q


def detect_candidate(positions_f32, times, select_pose, time_new_odom, time_last_loop, radius, time_thres):
    """Estimator.cpp:5113-5128: the keyframes within `radius` of select_pose (float squared distance ((dx dx + dy dy) + dz dz), counted when
    (double) d2 < radius^2), by ascending squared distance, ties by index (PCL's radius search sorts; the tie rule is unpinned); the first
    whose |time - time_new_odom| > time_thres.  -1: no such keyframe, or |time_last_loop - time_new_odom| < 0.2."""
    pos = np.ascontiguousarray(positions_f32, np.float32).reshape(-1, 3)
    sp = np.asarray(select_pose, np.float32)
    d = pos - sp[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2 = float(radius) * float(radius)
    cand = [(float(d2[i]), i) for i in range(len(pos)) if float(d2[i]) < r2]
    cand.sort()
    closest = -1
    for _, i in cand:
        if abs(float(times[i]) - float(time_new_odom)) > float(time_thres):
            closest = i
            break
    if closest == -1:
        return -1
    if abs(float(time_last_loop) - float(time_new_odom)) < LOOP_TIME_GATE:
        return -1
    return closest


def submap_frames(n_keyframes, slide_window_width, closest, lc_map_width):
    """Estimator.cpp:5133-5175: (latest, source list, target list).  latest = n - W; source: latest - j for j = 0..5 where >= 0, in that order;
    target: closest + j for j = -w..w where 0 <= closest + j <= latest, ascending."""
    latest = int(n_keyframes) - int(slide_window_width)
    src = [latest - j for j in range(LATEST_FRAMES) if latest - j >= 0]
    tgt = [closest + j for j in range(-int(lc_map_width), int(lc_map_width) + 1) if 0 <= closest + j <= latest]
    return latest, src, tgt


def frame_poses(pose_info, q_bl, t_bl):
    """Estimator.cpp:5147-5148 for every row of pose_info [n][7] = t_po, q_po (w first): rows t, q with q = q_po * q_bl, t = q_po * t_bl + t_po --
    what glio_loop_build_submap takes."""
    pose_info = np.asarray(pose_info, np.float64).reshape(-1, 7)
    qb, tb = [float(x) for x in q_bl], [float(x) for x in t_bl]
    out = np.zeros((len(pose_info), 7))
    for k, p in enumerate(pose_info):
        tp, qp = [float(x) for x in p[:3]], [float(x) for x in p[3:]]
        q = _qmul(qp, qb)
        r = _qrot(qp, tb)
        out[k, :3] = [r[0] + tp[0], r[1] + tp[1], r[2] + tp[2]]
        out[k, 3:] = q
    return out


def loop_constraint(result, pose_latest, pose_closest, icp_thres):
    """Estimator.cpp:5210-5247.  None when !converged or fitness > icp_thres (:5210).  Otherwise qIncre = Eigen::Quaterniond(rotation block cast to
    double), poseFrom = (qIncre * q, qIncre * t + tIncre) of pose_latest, poseTo = pose_closest (poses = t[3], q[4]); returns
    (relative [7] = t, q of poseFrom^-1 * poseTo, variances [6] all = fitness).  The two rotations enter the relative pose as UNIT quaternions
    (gtsam::Rot3::Quaternion builds a rotation from them; GTSAM itself is the caller's)."""
    if not result.converged or result.fitness > float(icp_thres):
        return None
    Tm = np.asarray(result.transform, np.float32).reshape(4, 4)
    R = [[float(Tm[r, c]) for c in range(3)] for r in range(3)]
    ti = [float(Tm[r, 3]) for r in range(3)]
    qi = eigen_R2q(R)
    pl, pc = [float(x) for x in pose_latest], [float(x) for x in pose_closest]
    qf = _qmul(qi, pl[3:])
    r = _qrot(qi, pl[:3])
    tf = [r[0] + ti[0], r[1] + ti[1], r[2] + ti[2]]
    nf = math.sqrt(qf[0] * qf[0] + qf[1] * qf[1] + qf[2] * qf[2] + qf[3] * qf[3])
    qf = [qf[0] / nf, qf[1] / nf, qf[2] / nf, qf[3] / nf]
    qt = pc[3:]
    nt = math.sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3])
    qt = [qt[0] / nt, qt[1] / nt, qt[2] / nt, qt[3] / nt]
    qfi = [qf[0], -qf[1], -qf[2], -qf[3]]
    q_rel = _qmul(qfi, qt)
    t_rel = _qrot(qfi, [pc[0] - tf[0], pc[1] - tf[1], pc[2] - tf[2]])
    return np.array(t_rel + q_rel), np.full(6, float(result.fitness))


def _qinv(q):
    """Eigen's Quaterniond::inverse(): conjugate / squaredNorm (zeros for the zero quaternion)"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    if not n2 > 0.0:
        return [0.0, 0.0, 0.0, 0.0]
    return [q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2]


def _q2R(q):
    """Eigen's toRotationMatrix() (no normalisation), row-major [9]"""
    w, x, y, z = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def correct_window_poses(abs_poses, corrected, W):
    """The sliding window's share of correctPoses (Estimator.cpp:4664-4686, :4702-4773).  abs_poses [N][7] = q (w first), t -- the estimator's abs_poses, where
    row i + 1 belongs to keyframe i (row 0 is the start pose); W = slide_window_width; corrected [N - W][7], same layout: the pose-graph poses of the keyframes
    0 .. N - 1 - W (pose_each_frame[keyframe_id_in_frame[i]], :4702-4713: the keyframes up to the window's oldest).
      1. the W - 1 relative poses between rows N - W .. N - 1 are taken BEFORE anything is corrected: q_rel = q_from.inverse() * q_to,
         t_rel = q_from.inverse() * (t_to - t_from) (Eigen's inverse(): conjugate / squaredNorm);
      2. rows 1 .. N - W take the corrected poses;
      3. rows N - W + 1 .. N - 1 are chained back on: t = t_prev + q_prev * t_rel, q = q_prev * q_rel.
    Returns (abs_poses', Rs [N][9] row-major toRotationMatrix() of each rewritten row, Ps [N][3]); row 0 of Rs / Ps is left zero (the reference does not write
    it).  pose_keyframe / pose_info_keyframe[i] are row i + 1 of abs_poses'.  glio::correctWindowPoses is the C++ twin, bit for bit.
    (Eigen's q * v assumes a unit quaternion: with |q| = 1 + e the chained translations are off by ~2 e |t_rel|, in the reference as here.)"""
    a = np.array(abs_poses, np.float64).reshape(-1, 7)
    N, W = len(a), int(W)
    c = np.asarray(corrected, np.float64).reshape(-1, 7)
    if not (1 <= W <= N) or len(c) != N - W:
        raise ValueError(f"correct_window_poses: {N} poses, window {W}, {len(c)} corrected poses (want {N - W})")
    out = [[float(x) for x in row] for row in a]
    rel = []
    for i in range(N - W, N - 1):
        qf, tf, qt, tt = out[i][:4], out[i][4:], out[i + 1][:4], out[i + 1][4:]
        qi = _qinv(qf)
        rel.append((_qmul(qi, qt), _qrot(qi, [tt[0] - tf[0], tt[1] - tf[1], tt[2] - tf[2]])))
    Rs, Ps = np.zeros((N, 9)), np.zeros((N, 3))
    for i in range(N - W):
        out[i + 1] = [float(x) for x in c[i]]
        Rs[i + 1], Ps[i + 1] = _q2R(out[i + 1][:4]), out[i + 1][4:]
    for k, i in enumerate(range(N - W, N - 1)):
        q, t = out[i][:4], out[i][4:]
        r = _qrot(q, rel[k][1])
        t = [t[0] + r[0], t[1] + r[1], t[2] + r[2]]
        q = _qmul(q, rel[k][0])
        out[i + 1] = q + t
        Rs[i + 1], Ps[i + 1] = _q2R(q), t
    return np.array(out), Rs, Ps

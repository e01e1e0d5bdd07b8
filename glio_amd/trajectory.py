"""The every-frame trajectory: the device object (glio_traj_*, csrc/trajectory_kernels.hip, include/glio_traj.h) and the host's share of
`saveKeyFramesAndFactors` (Estimator.cpp:4273-4557): which IMU samples make a frame segment (`frame_samples`) and the bookkeeping of pose_each_frame
(`Trajectory`).  `glio::frameImuSamples`, `glio::TrajectoryStore` and `glio::Trajectory` (host/glio_trajectory_backend.hpp) are the C++ twins: the same
scalar arithmetic in the same order, so the two hosts agree bit for bit (tests/test_trajectory_host_cpu.py).  Pose rows are t[3], q[4] (w first), what
posegraph.GlobalGraph.keyframe_call takes.  There is no CPU fallback for the gap itself."""
import ctypes as C

import numpy as np

from . import capi
from . import ctypes_types as T

ACC_CLAMP = (15.0, 15.0, 18.0)          # Estimator.cpp:4319-4325
MAX_FRAMES = 32                         # GLIO_TRAJ_MAX_FRAMES
TERMINATION_NAMES = ("NO_CONVERGENCE", "FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE", "MIN_RADIUS", "FAILURE", "NOT_SOLVED")
NO_CONVERGENCE, FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, GRADIENT_TOLERANCE, MIN_RADIUS, FAILURE, NOT_SOLVED = range(7)


class GlioTrajOpts(C.Structure):
    _fields_ = [("max_gaps", C.c_int32), ("max_frames_per_gap", C.c_int32), ("max_samples_per_gap", C.c_int32), ("max_iterations", C.c_int32)]


class GlioTrajSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32), ("n_frames", C.c_int32),
                ("accepted_mask", C.c_uint32), ("flag", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        return dict(termination=int(self.termination), iterations=int(self.iterations), successful_steps=int(self.successful_steps), n_frames=int(self.n_frames),
                    accepted_mask=int(self.accepted_mask), flag=int(self.flag), initial_cost=float(self.initial_cost), final_cost=float(self.final_cost))


def default_opts(**kw):
    lib = capi.load()
    lib.glio_traj_opts_default.restype = None
    o = GlioTrajOpts()
    lib.glio_traj_opts_default(C.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


# ------------------------------------------------------------------ the host's share: which samples make a frame segment
def _clamp(v, lim):
    if v > lim:
        v = lim
    if v < -lim:
        v = -lim
    return v


def frame_samples(stamps, acc, gyr, frame_stamps, imu_idx):
    """The sample rows of the gap's segments (Estimator.cpp:4287-4375 for every in-between frame, :4399-4481 for the last segment): frame_stamps are the
    stamps of frames keyframe_id_in_frame[a] .. keyframe_id_in_frame[b], imu_idx = imu_idx_in_kf[a].  Per segment
      * the start row (dt 0): the sample interpolated at the segment's first stamp between imu_idx and imu_idx + 1 -- NOT clamped for an in-between
        segment (:4295-4301), clamped for the last one (:4413-4419);
      * the whole samples with a stamp strictly before (`<`) the next frame stamp, acc clamped to +-15 / +-15 / +-18, dt against the previous stamp;
      * the closing row with dt1, interpolated between the values of the last row taken -- the CLAMPED acc of the last whole sample (:4348), or the start
        row's -- and the next sample, clamped.
    The IMU index steps back by one after an in-between frame (:4375).  Returns (seg_offset [n_segments + 1] int32, samples [.][7], imu_idx after)."""
    ii = int(imu_idx)
    M = len(frame_stamps) - 1
    offs, out = [0], []
    for i in range(1, M + 1):
        last = i == M
        t0, t1 = float(frame_stamps[i - 1]), float(frame_stamps[i])
        dt1 = t0 - float(stamps[ii])
        dt2 = float(stamps[ii + 1]) - t0
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [w1 * float(acc[ii][k]) + w2 * float(acc[ii + 1][k]) for k in range(3)]
        r = [w1 * float(gyr[ii][k]) + w2 * float(gyr[ii + 1][k]) for k in range(3)]
        if last:
            d = [_clamp(d[k], ACC_CLAMP[k]) for k in range(3)]
        out.append([0.0] + d + r)
        ii += 1
        start = t0
        while float(stamps[ii]) < t1:
            t = float(stamps[ii])
            dt = t - start
            start = t
            d = [_clamp(float(acc[ii][k]), ACC_CLAMP[k]) for k in range(3)]
            r = [float(gyr[ii][k]) for k in range(3)]
            out.append([dt] + d + r)
            ii += 1
        dt1 = t1 - float(stamps[ii - 1])
        dt2 = float(stamps[ii]) - t1
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [_clamp(w1 * d[k] + w2 * float(acc[ii][k]), ACC_CLAMP[k]) for k in range(3)]
        r = [w1 * r[k] + w2 * float(gyr[ii][k]) for k in range(3)]
        out.append([dt1] + d + r)
        if not last:
            ii -= 1
        offs.append(len(out))
    return np.array(offs, np.int32), np.array(out, float).reshape(-1, 7), ii


# ------------------------------------------------------------------ the device object
class GapResult:
    def __init__(self, summary, dead_reckoned, measurements, solved):
        self.summary, self.dead_reckoned, self.measurements, self.solved = summary, dead_reckoned, measurements, solved

    @property
    def termination_name(self):
        return TERMINATION_NAMES[self.summary["termination"]]


def _row(a, n):
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


class TrajectoryStore:
    """One glio_traj: every gap's dead-reckoned rows, measurements, solved rows and summary on the device."""

    def __init__(self, opts=None, device=0, **kw):
        lib = capi.load()
        if lib.glio_device_count() < 1:
            raise capi.GlioError("no HIP device visible: the trajectory has no CPU fallback")
        lib.glio_traj_destroy.restype = None
        self.opts = default_opts(**kw) if opts is None else opts
        self._h = C.c_void_p()
        capi._check(lib.glio_traj_create(int(device), C.byref(self.opts), C.byref(self._h)))
        self._n = {}

    def close(self):
        if self._h:
            capi.load().glio_traj_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push_gap(self, gap, n_frames, seg_offset, samples, start_state, gravity, prev_row, anchor_left, anchor_right):
        """Asynchronous: returns once the inputs are copied.  start_state [15] = P, V, R (row major)."""
        seg_offset = np.ascontiguousarray(seg_offset, np.int32)
        samples = np.ascontiguousarray(samples, np.float64).reshape(-1, 7)
        assert len(seg_offset) == int(n_frames) + 2
        capi._check(capi.load().glio_traj_push_gap(self._h, int(gap), int(n_frames), T.iptr(seg_offset), samples.ctypes.data_as(C.c_void_p) if len(samples) else None,
                                                   T.dptr(_row(start_state, 15)), T.dptr(_row(gravity, 3)), T.dptr(_row(prev_row, 7)), T.dptr(_row(anchor_left, 7)),
                                                   T.dptr(_row(anchor_right, 7))))
        self._n[int(gap)] = int(n_frames)

    def push(self, gap, case):
        """a dict with the arguments' names"""
        self.push_gap(gap, case["n_frames"], case["seg_offset"], case["samples"], case["start_state"], case["gravity"], case["prev_row"], case["anchor_left"],
                      case["anchor_right"])

    def resolve(self, first_gap, keyframe_poses, wait=True):
        """keyframe_poses [n_gaps + 1][7]; returns the per-gap summaries (wait) or None"""
        kp = np.ascontiguousarray(keyframe_poses, np.float64).reshape(-1, 7)
        n = len(kp) - 1
        out = (GlioTrajSummary * max(n, 1))() if wait else None
        capi._check(capi.load().glio_traj_resolve(self._h, int(first_gap), n, T.dptr(kp), out))
        return [out[k].as_dict() for k in range(n)] if wait else None

    def read(self, gap, check=True):
        """waits for that gap only; GlioError with code GLIO_E_NUMERIC for a flagged gap (check=False: delivered all the same, summary flag set)"""
        lib = capi.load()
        gap = int(gap)
        N = self._n.get(gap, 0)
        s = GlioTrajSummary()
        dr, ms, sol = np.zeros((N + 1, 7)), np.zeros((N + 1, 7)), np.zeros((N, 7))
        rc = lib.glio_traj_read(self._h, gap, C.byref(s), T.dptr(dr), T.dptr(ms), T.dptr(sol) if N else None)
        if rc != 0 and not (rc == -4 and not check):
            e = capi.GlioError(f"libglio_hip error {rc}: {lib.glio_last_error().decode()}")
            e.code = rc
            raise e
        return GapResult(s.as_dict(), dr, ms, sol)

    def last_device_ms(self):
        ms = C.c_float(0)
        capi._check(capi.load().glio_traj_last_device_ms(self._h, C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------ pose_each_frame / keyframe_id_in_frame for the caller
class Trajectory:
    """pose_each_frame (rows t, q) and keyframe_id_in_frame, fed once per keyframe call (Estimator.cpp:4273-4557).  Gap k lies between keyframes k and k + 1."""

    def __init__(self, store, W, gravity=(0.0, 0.0, 9.805)):
        self.store, self.W, self.gravity = store, int(W), np.asarray(gravity, float)
        self.keyframe_id_in_frame = []
        self._rows = []
        self._pending = []          # (gap, first in-between frame, N) pushed and not read yet

    def keyframe_call(self, keyframe_frame_id, keyframe_poses, frame_stamps, imu_stamps, imu_acc, imu_gyr, imu_idx_in_kf, start_state):
        """keyframe_frame_id: the frame the new keyframe is; keyframe_poses [n][7]: pose_info_keyframe after this call's window solve; frame_stamps: the stamp
        of every frame so far; imu_idx_in_kf [n]; start_state [15] = Ps, Vs, Rs at Ps.size() - W -- the keyframe AFTER the one the IMU index and the first
        frame belong to (:4281-4283 against :4279, :4287; include/glio_traj.h names the quirk).  Returns the gap pushed, or None.  Asynchronous: the
        in-between rows arrive with poses()."""
        self.keyframe_id_in_frame.append(int(keyframe_frame_id))
        n, W = len(self.keyframe_id_in_frame), self.W
        kp = np.asarray(keyframe_poses, float).reshape(-1, 7)
        if n == W:                                          # :4274-4277
            self._rows.append(kp[0].copy())
            return None
        if n < W:
            return None
        a, b = n - W - 1, n - W
        fa, fb = self.keyframe_id_in_frame[a], self.keyframe_id_in_frame[b]
        N = fb - fa - 1
        offs, smp, _ = frame_samples(imu_stamps, imu_acc, imu_gyr, [frame_stamps[i] for i in range(fa, fb + 1)], imu_idx_in_kf[a])
        assert len(self._rows) == fa + 1, "keyframe calls are not contiguous with the trajectory"
        self.store.push_gap(a, N, offs, smp, start_state, self.gravity, self._rows[fa], kp[a], kp[b])
        self._pending.append((a, fa + 1, N))
        self._rows.extend([None] * N)                       # the solved rows, read on demand
        self._rows.append(kp[b].copy())                     # :4397-4398
        return a

    def _flush(self):
        for gap, first, N in self._pending:
            sol = self.store.read(gap).solved
            for k in range(N):
                self._rows[first + k] = sol[k].copy()
        self._pending = []

    def poses(self):
        """pose_each_frame [F][7]: what GlobalGraph.keyframe_call takes (waits for the gaps pushed since the last call)"""
        self._flush()
        return np.array(self._rows, float).reshape(-1, 7)

    def resolve_all(self, keyframe_poses):
        """every in-between row solved again between the rows of keyframe_poses [>= n_gaps + 1][7] (after optimizeBatch or correctPoses): one launch.
        Returns the per-gap summaries."""
        self._flush()
        G = len(self.keyframe_id_in_frame) - self.W
        if G < 1:
            return []
        kp = np.asarray(keyframe_poses, float).reshape(-1, 7)[:G + 1]
        summ = self.store.resolve(0, kp)
        for k in range(G + 1):
            self._rows[self.keyframe_id_in_frame[k]] = kp[k].copy()
        for k in range(G):
            fa, fb = self.keyframe_id_in_frame[k], self.keyframe_id_in_frame[k + 1]
            if fb - fa - 1 > 0:
                sol = self.store.read(k).solved
                for i in range(fb - fa - 1):
                    self._rows[fa + 1 + i] = sol[i].copy()
        return summ


# ------------------------------------------------------------------ a synthetic drive (tests, the demo, the timing script)
def make_drive(n_keyframes=12, W=4, seed=0, imu_rate=200.0, frame_rate=10.0, pose_noise=(0.01, 0.002), correction=(0.05, 0.01)):
    """IMU samples, frame stamps, keyframes every 1-4 frames and the tables the hosts are fed with: keyframe_poses [NK][7] (the truth plus pose_noise: what the
    window solves would leave), start_states [NK][15] (row n - 1 = P, V, R passed at keyframe call n: the true state at the keyframe that left the window),
    corrected [NK][7] (the keyframe table after a correction, for resolve_all).  The truth is the IMU integrated by imu.propagate_state from rest."""
    from . import imu as imu_mod
    rng = np.random.RandomState(seed)
    steps = rng.randint(1, 5, n_keyframes - 1)
    kf_id = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)
    F = int(kf_id[-1]) + 1
    frame_stamps = 1000.0 + 0.013 + np.arange(F) / frame_rate + rng.uniform(-0.002, 0.002, F)
    n_imu = int((F / frame_rate + 0.2) * imu_rate)
    stamps = 1000.0 + np.arange(n_imu) / imu_rate
    g = np.array([0.0, 0.0, 9.805])
    t = stamps - stamps[0]
    gyr = np.stack([0.05 * np.sin(1.3 * t), 0.04 * np.cos(0.9 * t), 0.3 * np.sin(0.5 * t)], 1) + 0.01 * rng.randn(n_imu, 3)
    body = np.stack([0.8 * np.cos(0.7 * t), 0.5 * np.sin(1.1 * t), 0.1 * np.sin(2.0 * t)], 1) + 0.05 * rng.randn(n_imu, 3)
    R, P, V = np.eye(3), np.zeros(3), np.array([2.0, 0.0, 0.0])
    acc = np.zeros((n_imu, 3))
    states = []
    for i in range(n_imu):
        acc[i] = R.T @ g + body[i]
        if i:
            smp = np.concatenate([[stamps[i] - stamps[i - 1]], acc[i], gyr[i]])
            R, P, V, _, _ = imu_mod.propagate_state(R, P, V, np.zeros(3), np.zeros(3), acc[i - 1], gyr[i - 1], smp[None, :], g)
        states.append((P.copy(), V.copy(), R.copy()))
    imu_idx = np.array([int(np.searchsorted(stamps, frame_stamps[f], side="left")) - 1 for f in kf_id], np.int32)

    def quat(Rm):
        w = 0.5 * np.sqrt(max(1e-12, 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2]))
        return np.array([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])

    def disturbed(row, dp, da):
        v = rng.randn(3)
        v = v / np.linalg.norm(v) * da / 2.0
        d = np.array([1.0, v[0], v[1], v[2]])
        q = row[3:7]
        qq = np.array([q[0] * d[0] - q[1] * d[1] - q[2] * d[2] - q[3] * d[3], q[0] * d[1] + q[1] * d[0] + q[2] * d[3] - q[3] * d[2],
                       q[0] * d[2] + q[2] * d[0] + q[3] * d[1] - q[1] * d[3], q[0] * d[3] + q[3] * d[0] + q[1] * d[2] - q[2] * d[1]])
        return np.concatenate([row[0:3] + dp * rng.randn(3), qq / np.linalg.norm(qq)])
    truth = np.array([np.concatenate([states[i][0], quat(states[i][2])]) for i in imu_idx])
    keyframe_poses = np.array([disturbed(r, *pose_noise) for r in truth])
    corrected = np.array([disturbed(r, *correction) for r in keyframe_poses])
    start_states = np.zeros((n_keyframes, 15))
    for n in range(W + 1, n_keyframes + 1):
        Pa, Va, Ra = states[imu_idx[n - W - 1]]
        start_states[n - 1] = np.concatenate([Pa, Va, Ra.reshape(-1)])
    return dict(W=W, imu=np.concatenate([stamps[:, None], acc, gyr], 1), frame_stamps=frame_stamps, keyframe_id_in_frame=kf_id, imu_idx_in_kf=imu_idx,
                keyframe_poses=keyframe_poses, start_states=start_states, corrected=corrected, gravity=g)


def run_drive(drive, store, graph=None):
    """the drive through Trajectory (and GlobalGraph on `graph`, a posegraph.PoseGraph): returns (Trajectory, per-call summaries)"""
    from . import posegraph
    traj = Trajectory(store, drive["W"], drive["gravity"])
    glob = posegraph.GlobalGraph(graph, drive["W"]) if graph is not None else None
    imu_rows, kf = drive["imu"], drive["keyframe_id_in_frame"]
    calls = []
    for n in range(1, len(kf) + 1):
        gap = traj.keyframe_call(kf[n - 1], drive["keyframe_poses"][:n], drive["frame_stamps"][:kf[n - 1] + 1], imu_rows[:, 0], imu_rows[:, 1:4], imu_rows[:, 4:7],
                                 drive["imu_idx_in_kf"], drive["start_states"][n - 1])
        poses = traj.poses()
        if glob is not None:
            glob.keyframe_call(poses, traj.keyframe_id_in_frame, n)
        if gap is not None:
            s = store.read(gap).summary
            calls.append((n, gap, s["n_frames"], s["termination"], s["iterations"]))
    return traj, calls

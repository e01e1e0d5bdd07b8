"""Raw IMU input: the device-resident store of pre-integrations (glio_imu_*, csrc/imu_kernels.hip) and the host's share of
`saveKeyFramesAndFactors` (Estimator.cpp:4162-4229: which samples an edge is made of) and of `processIMU` (:1592-1598: the state
propagation beside the pre-integration).  `glio::ImuStore`, `glio::keyframeImuSamples` and `glio::propagateImuState`
(host/glio_backend.hpp) are the C++ twins: the same scalar arithmetic in the same order, so the two hosts agree bit for bit
(tests/test_imu_host_cpu.py).  There is no CPU fallback for the integration itself."""
import ctypes as C

import numpy as np

from . import capi
from . import ctypes_types as T

ACC_CLAMP = (15.0, 15.0, 18.0)          # Estimator.cpp:4176-4182


def default_noise():
    """glio_imu_noise of config_urban_hk.yaml:7-10"""
    lib = capi.load()
    lib.glio_imu_noise_default.restype = None
    n = T.GlioImuNoise()
    lib.glio_imu_noise_default(C.byref(n))
    return n


def make_noise(acc_n, gyr_n, acc_w, gyr_w):
    return T.GlioImuNoise(acc_n, gyr_n, acc_w, gyr_w)


HEADER_NOISE = (0.00059, 0.000061, 0.000011, 0.000001)          # the defaults of nh.param in Preintegration.h:48-51


def edge_arrays(acc, gyr, dts, ba, bg):
    """The raw form synth.preintegrate takes (acc / gyr [n + 1][3] with the start values in row 0, dts [n]) as (samples [n][7], start [12])."""
    acc, gyr, dts = np.asarray(acc, float), np.asarray(gyr, float), np.asarray(dts, float)
    n = len(dts)
    smp = np.zeros((n, 7))
    smp[:, 0], smp[:, 1:4], smp[:, 4:7] = dts, acc[1:n + 1], gyr[1:n + 1]
    return smp, np.concatenate([acc[0], gyr[0], np.asarray(ba, float), np.asarray(bg, float)])


def preint_dict(p):
    """glio_preint -> the dict synth.preintegrate returns"""
    return dict(delta_p=np.array(p.delta_p), delta_q=np.array(p.delta_q), delta_v=np.array(p.delta_v), linearized_ba=np.array(p.linearized_ba),
                linearized_bg=np.array(p.linearized_bg), sum_dt=float(p.sum_dt), jacobian=np.array(p.jacobian).reshape(15, 15),
                covariance=np.array(p.covariance).reshape(15, 15))


class ImuStore:
    """One glio_imu = the pre_integrations vector (Estimator.cpp:1582-1600) on the device: raw samples in, edges integrated and digested there."""

    def __init__(self, max_edges, max_samples_per_edge, noise=None, device=0):
        lib = capi.load()
        if lib.glio_device_count() < 1:
            raise capi.GlioError("no HIP device visible: the IMU store has no CPU fallback")
        lib.glio_imu_destroy.restype = None
        self.max_edges, self.max_samples, self.device = int(max_edges), int(max_samples_per_edge), device
        self.noise = default_noise() if noise is None else (noise if isinstance(noise, T.GlioImuNoise) else make_noise(*noise))
        self._h = C.c_void_p()
        capi._check(lib.glio_imu_create(device, self.max_edges, self.max_samples, C.byref(self.noise), C.byref(self._h)))

    def close(self):
        if self._h:
            capi.load().glio_imu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def integrate_raw(self, first_edge, offsets, samples, start):
        """offsets [n + 1] int32 into samples [.][7] (dt, acc, gyr); start [n][12] = acc0, gyr0, linearized_ba, linearized_bg.  Asynchronous."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        samples = np.ascontiguousarray(samples, np.float64).reshape(-1, 7)
        start = np.ascontiguousarray(start, np.float64).reshape(-1, 12)
        n = len(offsets) - 1
        assert n >= 0 and len(start) >= n
        capi._check(capi.load().glio_imu_integrate(self._h, int(first_edge), n, T.iptr(offsets), samples.ctypes.data_as(C.c_void_p) if len(samples) else None,
                                                   T.dptr(start) if n else None))

    def integrate(self, first_edge, edges):
        """edges: [(samples [n][7], start [12])] for store edges first_edge .. (edge_arrays makes one from the generators' raw form)"""
        offs = np.zeros(len(edges) + 1, np.int32)
        for k, (smp, _) in enumerate(edges):
            offs[k + 1] = offs[k] + len(smp)
        smp = np.concatenate([np.asarray(e[0], float).reshape(-1, 7) for e in edges]) if edges else np.zeros((0, 7))
        start = np.array([np.asarray(e[1], float) for e in edges]).reshape(-1, 12)
        self.integrate_raw(first_edge, offs, smp, start)

    def read_structs(self, first_edge, n):
        out = T.preint_array(n)
        capi._check(capi.load().glio_imu_read(self._h, int(first_edge), int(n), out))
        return out

    def read(self, first_edge=0, n=None):
        """the host view of n edges (waits): dicts with the fields of glio_preint"""
        n = self.max_edges - first_edge if n is None else n
        arr = self.read_structs(first_edge, n)
        return [preint_dict(arr[k]) for k in range(n)]

    def last_device_ms(self):
        ms = C.c_float(0)
        capi._check(capi.load().glio_imu_last_device_ms(self._h, C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------ the host's share: sample preparation and state propagation
def _clamp(v, lim):
    if v > lim:
        v = lim
    if v < -lim:
        v = -lim
    return v


def keyframe_samples(stamps, acc, gyr, idx_imu, cur_time_imu, kf_time):
    """The (dt, acc, gyr) list `processIMU` is called with for the keyframe at kf_time (Estimator.cpp:4162-4229): the samples of the buffer from
    idx_imu with a stamp strictly before kf_time -- dt against cur_time_imu (0 for the very first sample, cur_time_imu < 0), acc clamped to
    +-15 / +-15 / +-18 -- up to the buffer's end, then the closing sample interpolated between the last one taken and the next
    (w1 = dt2 / (dt1 + dt2), w2 = dt1 / (dt1 + dt2), clamped again) with dt1 = kf_time - cur_time_imu; none when the buffer ended.
    Returns (samples [n][7], idx_imu, cur_time_imu) with the two running values as the reference leaves them (:4243, :4229)."""
    n = len(stamps)
    i = int(idx_imu)
    cur = float(cur_time_imu)
    kf_time = float(kf_time)
    d = [0.0, 0.0, 0.0]
    r = [0.0, 0.0, 0.0]
    out = []
    while i < n and float(stamps[i]) < kf_time:
        t = float(stamps[i])
        if cur < 0:
            cur = t
        dt = t - cur
        cur = t
        d = [_clamp(float(acc[i][k]), ACC_CLAMP[k]) for k in range(3)]
        r = [float(gyr[i][k]) for k in range(3)]
        out.append([dt] + d + r)
        i += 1
        if i >= n:
            break
    if i < n:
        dt1 = kf_time - cur
        dt2 = float(stamps[i]) - kf_time
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [_clamp(w1 * d[k] + w2 * float(acc[i][k]), ACC_CLAMP[k]) for k in range(3)]
        r = [w1 * r[k] + w2 * float(gyr[i][k]) for k in range(3)]
        out.append([dt1] + d + r)
    return np.array(out, float).reshape(-1, 7), i, kf_time


def propagate_state(R, P, V, ba, bg, acc0, gyr0, samples, g):
    """Rs / Ps / Vs of processIMU (Estimator.cpp:1592-1598) over the samples of one edge: midpoint propagation in the world frame with
    deltaQ(un_gyr dt) = (1, un_gyr dt / 2) turned into a matrix by Eigen's toRotationMatrix() WITHOUT normalisation (synth.q2R_eigen's
    formula).  R [3][3], P, V, ba, bg, acc0, gyr0, g (the gravity vector, (0, 0, 9.805...)) [3].  Returns (R, P, V, acc0, gyr0) after the last
    sample.  Plain scalar arithmetic in a fixed order: the C++ twin gives the same doubles."""
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    P, V = [float(v) for v in P], [float(v) for v in V]
    ba, bg, g = [float(v) for v in ba], [float(v) for v in bg], [float(v) for v in g]
    a0, w0 = [float(v) for v in acc0], [float(v) for v in gyr0]
    for s in np.asarray(samples, float).reshape(-1, 7):
        dt = float(s[0])
        a1, w1 = [float(v) for v in s[1:4]], [float(v) for v in s[4:7]]
        e0 = [a0[k] - ba[k] for k in range(3)]
        un0 = [R[i][0] * e0[0] + R[i][1] * e0[1] + R[i][2] * e0[2] - g[i] for i in range(3)]
        ug = [0.5 * (w0[k] + w1[k]) - bg[k] for k in range(3)]
        qw, qx, qy, qz = 1.0, ug[0] * dt / 2.0, ug[1] * dt / 2.0, ug[2] * dt / 2.0
        tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
        twx, twy, twz = tx * qw, ty * qw, tz * qw
        txx, txy, txz = tx * qx, ty * qx, tz * qx
        tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
        D = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
        R = [[R[i][0] * D[0][j] + R[i][1] * D[1][j] + R[i][2] * D[2][j] for j in range(3)] for i in range(3)]
        e1 = [a1[k] - ba[k] for k in range(3)]
        un1 = [R[i][0] * e1[0] + R[i][1] * e1[1] + R[i][2] * e1[2] - g[i] for i in range(3)]
        un = [0.5 * (un0[k] + un1[k]) for k in range(3)]
        P = [P[k] + (dt * V[k] + 0.5 * dt * dt * un[k]) for k in range(3)]
        V = [V[k] + dt * un[k] for k in range(3)]
        a0, w0 = a1, w1
    return np.array(R), np.array(P), np.array(V), np.array(a0), np.array(w0)

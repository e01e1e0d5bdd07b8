"""LiDAR feature extraction from the raw scan (Preprocessing::cloudHandler, reference GLIO/src/Preprocessing.cpp:353-681), host side.

The extraction itself runs on the device (glio_features_*, capi.Context.features_*).  What stays on the host is the rotation of the
sweep that the reference integrates from the gyro (processIMU / solveRotation, :202-259): ScanRotation restates it, and
glio::ScanRotation (host/glio_backend.hpp) is the same class in C++.
"""
import math

import numpy as np

from . import ctypes_types as T

# config_urban_hk.yaml:14-18,90-93 and the node's members
N_SCANS = 32              # line_num
DS_RATE = 1               # ds_rate
EDGE_THRESHOLD = 1.0      # edgeThreshold
SURF_THRESHOLD = 0.1      # surfThreshold
DS_LEAF = 0.4             # Preprocessing::ds_v (:14): a member default, never read from the yaml
MIN_RANGE = 3.0           # removeClosedPointCloud(.., 3.0) (:397)
Q_LB = (1.0, 0.0, 0.0, 0.0)   # ql2b_w/x/y/z


def default_opts(n_scans=N_SCANS, max_raw_points=T.FEAT_MAX_RAW_POINTS, **kw):
    o = T.GlioFeatOpts()
    o.n_scans, o.ds_rate = n_scans, DS_RATE
    o.edge_threshold, o.surf_threshold = EDGE_THRESHOLD, SURF_THRESHOLD
    o.ds_leaf, o.min_range = DS_LEAF, MIN_RANGE
    o.q_lb[:] = Q_LB
    o.max_raw_points = max_raw_points
    for k, v in kw.items():
        if k == "q_lb":
            o.q_lb[:] = v
        else:
            setattr(o, k, v)
    return o


def qmul(a, b):
    """Eigen's quaternion product (w, x, y, z), in the operation order of glio_device.h d_qmul"""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


class ScanRotation:
    """qIMU of Preprocessing: imuHandler (:260-292), processIMU (:223-259) with solveRotation (:202-207) and the NON-normalised
    deltaQ of math_tools.h (w = 1, xyz = theta / 2), the NaN guard (:415-417) and the reset after each cloud (:675).

    add_imu(t, gyro) per IMU message; for_scan(t_scan_next) per cloud -- t_scan_next is the stamp of the NEXT cloud in the queue
    (cloudHandler keeps two clouds queued, :356-371).  Returns qIMU (w, x, y, z) to hand to the extraction, or None where the reference
    returns "Waiting for IMU data" (:373-377) and drops the cloud.  qIMU is reset to the identity after every handled cloud."""

    def __init__(self):
        self.buf = []                      # (t, wx, wy, wz)
        self.idx_imu = 0
        self.current_time_imu = -1.0
        self.gyr_0 = (0.0, 0.0, 0.0)
        self.q = (1.0, 0.0, 0.0, 0.0)
        self.first_imu = False

    def add_imu(self, t, gyro):
        self.buf.append((float(t), float(gyro[0]), float(gyro[1]), float(gyro[2])))
        if self.current_time_imu < 0:              # the first sample's dt is 0
            self.current_time_imu = float(t)
        if not self.first_imu:
            self.first_imu = True
            self.gyr_0 = (float(gyro[0]), float(gyro[1]), float(gyro[2]))

    def _solve(self, dt, w):
        un = tuple(0.5 * (self.gyr_0[k] + w[k]) for k in range(3))
        th = tuple(un[k] * dt for k in range(3))
        dq = (1.0, th[0] / 2.0, th[1] / 2.0, th[2] / 2.0)
        self.q = qmul(self.q, dq)
        self.gyr_0 = (w[0], w[1], w[2])

    def process(self, t_cur):
        buf = self.buf
        rx = ry = rz = 0.0
        i = self.idx_imu
        if i >= len(buf):
            i -= 1
        while buf[i][0] < t_cur:
            t = buf[i][0]
            if self.current_time_imu < 0:
                self.current_time_imu = t
            dt = t - self.current_time_imu
            self.current_time_imu = buf[i][0]
            rx, ry, rz = buf[i][1], buf[i][2], buf[i][3]
            self._solve(dt, (rx, ry, rz))
            i += 1
            if i >= len(buf):
                break
        if i < len(buf):                            # the interpolated last step at t_cur
            dt1 = t_cur - self.current_time_imu
            dt2 = buf[i][0] - t_cur
            w1 = dt2 / (dt1 + dt2)
            w2 = dt1 / (dt1 + dt2)
            rx = w1 * rx + w2 * buf[i][1]
            ry = w1 * ry + w2 * buf[i][2]
            rz = w1 * rz + w2 * buf[i][3]
            self._solve(dt1, (rx, ry, rz))
        self.current_time_imu = t_cur
        self.idx_imu = i

    def for_scan(self, t_scan_next):
        tmp = self.idx_imu - 1 if self.idx_imu > 0 else 0
        if not self.buf or self.buf[tmp][0] > t_scan_next:
            return None
        if self.first_imu:
            self.process(float(t_scan_next))
        if any(math.isnan(v) for v in self.q):
            self.q = (1.0, 0.0, 0.0, 0.0)
        q = np.array(self.q, np.float64)
        self.q = (1.0, 0.0, 0.0, 0.0)
        return q

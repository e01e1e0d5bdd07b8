"""CPU restatement of the keyframe cloud's hand-over (reference GLIO/src/LidarOdometry.cpp:180-201, :619-627 and Estimator.cpp:3628-3630) -- TEST
INFRASTRUCTURE ONLY, the checker of glio_set_scan_filtered* / glio_set_scan_from_features*.  Rounding as preproc_restated.py states it: Python floats are
the reference's doubles, numpy float32 its floats, math.acos / math.sin the slerp's libm, Eigen's operation order for slerp and q * v.

  deskew(pts, trans, quat)      undistortion(cloud, trans, quat): per point line = (int)intensity (truncating), dt_i the FLOAT difference, ratio = dt_i / 0.1
                                capped at 1 and not clamped below, q_si = Identity.slerp(ratio, quat), t_si = ratio * trans, pt = q_si * pt + t_si stored as
                                float, the intensity unchanged
  keyframe_cloud(pts, leaf, trans, quat)   the de-skew (trans None: none) followed by pcl::VoxelGrid at leaf (leaf <= 0: the cloud as it is)

The gate of LidarOdometry.cpp:566-578 (which scans are keyframes) is restated in gate_sequence() for the C++ and Python KeyframeGate tests.
"""
import math

import numpy as np

from preproc_restated import DBL_EPS, F, _qrot, voxel_grid


def ratio_of(inten):
    f = F(inten)
    line = int(f)                                  # (int): toward zero
    t = float(F(f - F(line))) / 0.1
    return 1.0 if t >= 1.0 else t


def slerp_identity(quat, t):
    qw, qx, qy, qz = (float(v) for v in quat)
    d = 0.0 * qx + 0.0 * qy + 0.0 * qz + 1.0 * qw
    ad = abs(d)
    if ad >= 1.0 - DBL_EPS:
        s0, s1 = 1.0 - t, t
    else:
        th = math.acos(ad)
        sth = math.sin(th)
        s0 = math.sin((1.0 - t) * th) / sth
        s1 = math.sin(t * th) / sth
    if d < 0.0:
        s1 = -s1
    return (s0 * 1.0 + s1 * qw, s0 * 0.0 + s1 * qx, s0 * 0.0 + s1 * qy, s0 * 0.0 + s1 * qz)


def deskew(pts, trans, quat=None):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    quat = (1.0, 0.0, 0.0, 0.0) if quat is None else tuple(float(v) for v in quat)
    tr = [float(v) for v in trans]
    out = pts.copy()
    for i in range(len(pts)):
        t = ratio_of(pts[i, 3])
        qs = slerp_identity(quat, t)
        o = _qrot(qs, [float(pts[i, 0]), float(pts[i, 1]), float(pts[i, 2])])
        for k in range(3):
            out[i, k] = F(o[k] + t * tr[k])
    return out


def keyframe_cloud(pts, leaf, trans=None, quat=None):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    moved = pts.copy() if trans is None else deskew(pts, trans, quat)
    if not leaf > 0:
        return moved
    return voxel_grid(moved, leaf)


# ---- the hand-made intensity table: fractions 0, 0.05, 0.0999, 0.1 (3.1 in float leaves a ratio a hair below 1, 1.1 a hair above: 1 by the cap's
# comparison alone), 4.35 (far beyond: the cap), -0.01 (ratio -0.1), 15.0625 (exact: 0.625)
def intensity_table():
    inten = np.array([3.0, 3.05, 3.0999, 3.1, 4.35, -0.01, 0.0, 7.02, 15.0625, 2.5, 1.1], np.float32)
    xyz = np.array([[10.0, 0.5, -1.0], [-7.25, 3.0, 0.25], [4.0, -12.5, 2.0], [0.75, 0.5, 0.25], [-20.0, -20.0, 1.5],
                    [6.0, 6.0, -0.5], [1.0, 2.0, 3.0], [-3.5, 8.0, 0.0], [30.0, -1.0, 4.0], [2.0, 2.0, 2.0], [-5.0, 5.0, -5.0]], np.float32)
    return np.concatenate([xyz, inten[:, None]], 1).astype(np.float32)


# ---- LidarOdometry.cpp:566-578 with the initial values of :71-75: kf = true, kf_num = 0, quat_last_kF the identity, trans_last_kf zero
def gate_sequence(poses, first_size=1):
    """poses: a list of (q (w x y z), t) of consecutive scans; the first is judged with pose_cloud_frame->points.size() == first_size (1: the scan
    after the initialisation frame, :671-675), savePoses adds one per scan and a keyframe sets kf_num to the size after it (:684-685).  Returns the kf
    flag of every scan, restated independently of glio_amd.odometry.KeyframeGate."""
    kf_num = 0
    ql, tl = (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    out = []
    size = first_size
    for q, t in poses:
        dis = math.sqrt((t[0] - tl[0]) ** 2 + (t[1] - tl[1]) ** 2 + (t[2] - tl[2]) ** 2)
        n2 = ql[0] * ql[0] + ql[1] * ql[1] + ql[2] * ql[2] + ql[3] * ql[3]                     # inverse(): conjugate / squaredNorm
        iw, ix, iy, iz = ql[0] / n2, -ql[1] / n2, -ql[2] / n2, -ql[3] / n2
        w = iw * q[0] - ix * q[1] - iy * q[2] - iz * q[3]
        ang = 2.0 * math.acos(w) if -1.0 <= w <= 1.0 else float("nan")                         # acos outside [-1, 1]: NaN, every comparison false
        kf = ((dis > 0.2 or ang > 0.1) and size - kf_num > 1) or size - kf_num > 2 or size <= 1
        if kf:
            ql, tl = tuple(q), tuple(t)
        size += 1                                                                              # savePoses
        if kf:
            kf_num = size
        out.append(bool(kf))
    return out

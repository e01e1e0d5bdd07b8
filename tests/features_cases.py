"""Inputs that take the front end (glio_features_*, csrc/feature_kernels.hip) through every branch of Preprocessing::cloudHandler -- no GPU import.

  * ORIENTATION: 16-line scans of 301 columns, cut and re-joined so that every adjustment of the orientation state machine fires (reference
    Preprocessing.cpp:406, :409, :491, :493, :501, :503), halfPassed is never set, relTime leaves [0, 1];
  * OPTIONS: every glio_feat_opts field away from its default;
  * hand_rings() / zigzag(): exact rows whose picks are known on paper (tests/test_preproc_restated.py), with tied curvatures;
  * q_imu_forms(): the quaternions production hands over (negated, non-unit on either slerp branch, features.ScanRotation's product).

tests/test_features_cases_cpu.py shows that each case reaches what it claims; tests/test_hip_features_branches.py holds the device to the
restatement (tests/preproc_restated.py) on them.

301 columns, not 300: with a column count divisible by 4 one column lies exactly a quarter, a half or three quarters of a turn from the start,
within 1e-7 rad of a threshold, and on a reversed turn the device's atan2f and glibc's may then take different branches."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_restated as pr  # noqa: E402

from glio_amd import ctypes_types as T  # noqa: E402
from glio_amd import features, synth_lidar as sl  # noqa: E402

N_SCANS, N_AZ, SEED = 16, 301, 5
MARGIN = 1e-4             # rad: a condition on the inputs.  atan2f on either side is within a few ulps (< 1e-6 rad near pi) of the true angle
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])
OUTPUTS = [("sharp", T.FEAT_SHARP), ("less_sharp", T.FEAT_EDGE_LESS_SHARP), ("flat", T.FEAT_FLAT), ("surf", T.FEAT_SURF)]


# ------------------------------------------------------------------------------------------------ shared with tests/test_hip_features.py
def _ctx(n_scans, max_raw=T.FEAT_MAX_RAW_POINTS):
    from glio_amd import capi, synth
    ctx = capi.Context(synth.default_opts(1, pts=1 << 16, map_pts=1 << 16))
    ctx.features_config(features.default_opts(n_scans, max_raw_points=max_raw))
    return ctx


def _yaw_q(yaw):
    return np.array([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _intensity_close(a, b):
    """intensity = scanID + 0.1 relTime within 2 float ulps taken at the scale of the ring's value (scanID + 0.1).  glibc's atan2f is not correctly
    rounded and neither is the device's: one ulp of the orientation moves relTime by ~1e-8, which near relTime = 0 on ring 0 is many ulps of the tiny
    intensity itself: the gate is 2 ulps of the ring's value or 2 ulps of an orientation near 4 pi carried through relTime, whichever is larger"""
    scale = np.spacing((np.rint(b.astype(np.float64)) + 0.1).astype(np.float32)).astype(np.float64)
    ori = 0.1 * float(np.spacing(np.float32(4 * math.pi))) / (2 * math.pi)        # one ulp of an orientation near 4 pi, through relTime
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    tol = 2 * np.maximum(scale, ori)
    i = int(np.argmax(err / tol))
    print(f"intensity: max |d| {err.max():.3e}, worst d / tol {err[i] / tol[i]:.3f} at {i} ({b[i]!r})")
    return bool((err <= tol).all())


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ orientation cases
@functools.lru_cache(maxsize=None)
def _turn(start_az):
    """one clean clockwise turn as [column][laser][4]: the lasers of a column fire together (synth_lidar.make_scan is column-major)"""
    t = sl.make_scan(N_SCANS, N_AZ, start_az=start_az, seed=SEED).reshape(N_AZ, N_SCANS, 4)
    t.setflags(write=False)
    return t


def _flat(columns):
    return np.ascontiguousarray(columns, np.float32).reshape(-1, 4)


def _edges_dropped():
    """the baseline with its first and last three columns gone: NaN (removeNaNFromPointCloud) or pulled inside 3 m (removeClosedPointCloud)"""
    t = _turn(0.7).copy()
    for c in (0, 2, N_AZ - 2):
        t[c, :, :3] = np.nan
    for c in (1, N_AZ - 3, N_AZ - 1):
        r = np.linalg.norm(t[c, :, :3].astype(np.float64), axis=1, keepdims=True)
        t[c, :, :3] = (t[c, :, :3] * (2.0 / r)).astype(np.float32)                  # range 2 m (NaN misses stay NaN)
    return t


def _jitter():
    t = _turn(-3.1)
    return np.concatenate([t[5:10], t[0:5], t[10:-10], t[-5:], t[-10:-5]])


# name -> (columns, what the restatement must report: branches with non-zero counts, halfPassed, relTime range)
ORIENTATION = {
    "baseline":       (lambda: _turn(0.7),                                    dict(reach={"n503"}, only=True, rel=(0.0, 1.0))),
    "c_first_plus":   (lambda: _turn(-0.7),                                   dict(reach={"n491"}, rel=(0.0, 1.0))),
    "a_partial":      (lambda: _turn(0.7)[:181],                              dict(reach={"end_minus"}, rel=(0.0, 1.0))),
    "b_never_half":   (lambda: _turn(-0.7)[:120],                             dict(reach={"end_plus"}, half=False, rel=(0.0, 0.29))),
    "a_full":         (lambda: _turn(math.pi),                                dict(reach={"end_minus"}, rel=(0.0, 1.0))),
    "over_full":      (lambda: np.concatenate([_turn(-2.0), _turn(-2.0)[:60]]), dict(reach={"end_plus", "n491", "n501"}, rel=(0.0, 1.0))),
    # 468 degrees: endOri - 3 pi/2 lies beyond startOri + pi, so the point that sets halfPassed would come out a turn later on the second branch
    "over_full_wide": (lambda: np.concatenate([_turn(-2.0), _turn(-2.0)[:90]]), dict(reach={"end_plus", "n491", "n501"}, half_differs=True, rel=(0.0, 1.2))),
    "reversed_1":     (lambda: _turn(2.0)[::-1],                              dict(reach={"n493"}, outside=True, rel=(-0.27, 1.27))),
    "reversed_2":     (lambda: _turn(-3.1)[::-1],                             dict(reach={"n501"}, outside=True, rel=(-0.27, 1.27))),
    "jitter":         (_jitter,                                               dict(reach={"end_minus", "n493"}, outside=True, rel=(-0.05, 1.05))),
    "edges_dropped":  (_edges_dropped,                                        dict(reach={"n503"}, rel=(0.0, 1.0))),
}
ORIENTATION_NAMES = list(ORIENTATION)
ROTATED_NAMES = ORIENTATION_NAMES            # every case also runs with a yaw of 0.1 rad
YAW = 0.1


@functools.lru_cache(maxsize=None)
def orientation_scan(name):
    raw = _flat(ORIENTATION[name][0]())
    raw.setflags(write=False)
    return raw


def orientation_claim(name):
    return ORIENTATION[name][1]


# ------------------------------------------------------------------------------------------------ option cases
def q_lb_tilted():
    """the rotation vector (0.02, -0.03, 0.5) as a unit quaternion"""
    v = np.array([0.02, -0.03, 0.5])
    a = float(np.linalg.norm(v))
    return np.concatenate([[math.cos(a / 2)], math.sin(a / 2) * v / a])


def near_origin_row():
    """one ring-8 row passing 0.25 m from the origin: 13 of its 129 points have a squared norm below 0.25 (:603, :641)"""
    p = np.zeros((129, 4), np.float32)
    p[:, 0] = -4.0 + 0.0625 * np.arange(129)
    p[:, 1] = 0.25
    return p


# selection stage (k_ft_rings): held on the device's own cut cloud
SELECT_OPTIONS = {
    "ds_rate_2": dict(ds_rate=2), "ds_rate_3": dict(ds_rate=3),
    "edge_0.2": dict(edge_threshold=0.2), "edge_50": dict(edge_threshold=50.0),
    "surf_0.01": dict(surf_threshold=0.01), "surf_1.0": dict(surf_threshold=1.0),
    "leaf_0.2": dict(ds_leaf=0.2), "leaf_1.0": dict(ds_leaf=1.0),
}
# projection stage (survivors, de-skew): end to end; name -> (scan, options, q_imu)
NEAR_OPTS = dict(min_range=0.2, ds_leaf=0.01)          # a leaf below the row's spacing: every less-flat point is its own voxel


def project_options():
    base = orientation_scan("baseline")
    return {
        "min_range_10": (base, dict(min_range=10.0), IDENTITY),
        "min_range_0.2_near": (near_origin_row(), NEAR_OPTS, IDENTITY),
        "q_lb_identity_imu": (base, dict(q_lb=tuple(q_lb_tilted())), IDENTITY),
        "q_lb_yaw": (base, dict(q_lb=tuple(q_lb_tilted())), _yaw_q(YAW)),
    }


def device_opts(n_scans, max_raw, **kw):
    """glio_feat_opts for the device from the restatement's keyword names"""
    return features.default_opts(n_scans, max_raw_points=max_raw, **kw)


# ------------------------------------------------------------------------------------------------ hand-made rings through the raw entry
HAND_ROWS = [(125, 16.0, 0.0, 8), (113, 40.0, 2.0, 9), (17, 40.0, -2.0, 6), (16, 40.0, 4.0, 10), (11, 40.0, -4.0, 5)]       # points, x0, z, ring
HAND_LEAF = 0.01


def _row(n, x0, z):
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = x0 + 0.125 * np.arange(n)
    p[:, 2] = z
    return p


def hand_rings(rows=HAND_ROWS):
    """rows x = x0 + 0.125 k, y = 0, constant z (spacing exact in float: every curvature is exactly 0), interleaved round-robin in the raw order so
    that the stable bucketing by ring has work to do.  y = 0 and x > 0: every orientation is -0.0, relTime 0, intensity the ring"""
    ps = [_row(n, x0, z) for n, x0, z, _ in rows]
    out = [p[k] for k in range(max(len(p) for p in ps)) for p in ps if k < len(p)]
    return np.array(out, np.float32)


def small_rings():
    """the rings of 11, 16 and 17 points alone"""
    return hand_rings(HAND_ROWS[2:])


def zigzag():
    """test_edges_break_on_the_eleventh's ring: every point a corner with the same curvature (576), steps far above 0.05 (no marks); ring 8"""
    n = 6 * 30 + 11
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = 20.0 + np.arange(n)
    p[:, 1] = np.where(np.arange(n) % 2 == 0, 2.0, -2.0)
    return p


def check_hand_picks(out):
    """the literal indices of tests/test_preproc_restated.py (equal curvatures rank by index, the 4th flat marks nothing, marks cross sectors)"""
    flat, surf = out["flat"], out["surf"]
    x = lambda x0, idx: [np.float32(x0 + 0.125 * i) for i in idx]
    assert list(flat[flat[:, 2] == 0][:5, 0]) == x(16.0, [5, 11, 17, 23, 24])
    assert list(flat[flat[:, 2] == 2][:6, 0]) == x(40.0, [5, 11, 17, 23, 29, 35])
    assert list(flat[flat[:, 2] == -2][:, 0]) == x(40.0, [5])
    assert list(surf[surf[:, 2] == -2][:, 0]) == x(40.0, [5, 6, 7, 8, 9, 10])
    for z in (4, -4):
        assert not (flat[:, 2] == z).any() and not (surf[:, 2] == z).any()
    assert len(out["sharp"]) == 0 and len(out["less_sharp"]) == 0


def check_zigzag_order(out):
    """ties rank by index: every sector [5 + 30 j, 34 + 30 j] gives its picks from the top index down, 2 sharp and 10 less sharp"""
    assert list(out["sharp"][:, 0]) == [np.float32(20 + 34 + 30 * j - k) for j in range(6) for k in range(2)]
    assert list(out["less_sharp"][:, 0]) == [np.float32(20 + 34 + 30 * j - k) for j in range(6) for k in range(10)]


AXIS_ROW = 40


def axis_rows():
    """two ring-8 rows on the +x and the -y axis: atan2f(0, x) = 0 and atan2f(-y, 0) = -pi/2 are exact special cases of any libm, so the intensities (the
    ring, and the ring + 0.1 * (pi/2) / (pi/2 + 2 pi) in float) are the same bits on the device and in glibc, and every comparison is pi/2 from its
    constant"""
    a, b = _row(AXIS_ROW, 16.0, 0.0), _row(AXIS_ROW, 16.0, 0.0)
    b[:, 1] = -b[:, 0]
    b[:, 0] = 0.0
    return np.vstack([a, b])


def one_ring_60000():
    """tests/test_hip_features.py's 60 000-point ring (32 lines): large enough to leave every buffer of a context full"""
    rng = np.random.default_rng(5)
    n = 60000
    a = 0.4 - 2 * np.pi * np.arange(n) / n
    r = 12.0 / np.maximum(np.abs(np.cos(a)), np.abs(np.sin(a))) ** 0.7 + 0.01 * rng.standard_normal(n)
    raw = np.zeros((n, 4), np.float32)
    raw[:, 0], raw[:, 1] = r * np.cos(a), r * np.sin(a)
    return raw


# ------------------------------------------------------------------------------------------------ q_imu forms
def scan_rotation_q():
    """features.ScanRotation's product of non-normalised deltaQ after a dozen gyro samples of about 0.5 rad/s over a 0.1 s sweep"""
    rot = features.ScanRotation()
    for k in range(12):
        rot.add_imu(0.009 * k, (0.03 + 0.002 * k, -0.05 + 0.001 * k, 0.5 - 0.003 * k))
    q = rot.for_scan(0.1)
    assert q is not None
    return q


def slerp_branch(q):
    """which arm of Eigen's slerp from the identity q takes: linear at |w| >= 1 - epsilon"""
    return "linear" if abs(float(q[0])) >= 1.0 - pr.DBL_EPS else "acos"


def q_imu_forms():
    """name -> (q_imu, slerp branch, unit?)"""
    return {
        "negated_yaw": (-_yaw_q(YAW), "acos", True),
        "non_unit_linear": (np.array([1.0, 0.02, -0.01, 0.03]), "linear", False),
        "non_unit_acos": (np.array([0.999, 0.02, -0.01, 0.03]), "acos", False),
        "scan_rotation": (scan_rotation_q(), "acos", False),
    }


def position_gate(got, want):
    """the gate of test_end_to_end_with_a_sweep_rotation: 2e-6 * range + 1e-6 m.  Returns the worst excess (<= 0 passes)"""
    rng = np.linalg.norm(want[:, :3].astype(np.float64), axis=1)
    err = np.linalg.norm(got[:, :3].astype(np.float64) - want[:, :3], axis=1)
    return float((err - (2e-6 * rng + 1e-6)).max()) if len(want) else -1e-6

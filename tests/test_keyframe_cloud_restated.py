"""The numpy restatement of the keyframe cloud's de-skew (tests/keyframe_cloud_restated.py) against the restatement of the front end's undistortion
(tests/preproc_restated.py: the reference carries the same function body in both files) and against hand-made values."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_cloud_restated as kr  # noqa: E402
import preproc_restated as pr  # noqa: E402

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-80.0, 80.0, (n, 3))
    inten = rng.integers(0, 32, n) + rng.uniform(0.0, 0.12, n)          # ring + 0.1 relTime, some beyond the cap
    return np.concatenate([xyz, inten[:, None]], 1).astype(np.float32)


def test_zero_translation_is_the_front_ends_undistortion_bit_for_bit():
    p = _random_cloud(2000, 1)
    yaw = 0.07
    quat = np.array([np.cos(yaw / 2), 0.01, -0.02, np.sin(yaw / 2)])
    quat /= np.linalg.norm(quat)
    got = kr.deskew(p, (0.0, 0.0, 0.0), quat)
    want = pr.undistort(p[:, :3], p[:, 3], quat, (1.0, 0.0, 0.0, 0.0))
    assert np.array_equal(_bits(got[:, :3]), _bits(want))
    assert np.array_equal(_bits(got[:, 3]), _bits(p[:, 3]))


def test_identity_quat_is_the_point_plus_ratio_times_trans_exactly():
    """slerp's w = (1 - t) + t is not always 1, yet u = 0 makes q * v return v itself: the output is float32(float64(p) + ratio * trans)"""
    p = _random_cloud(2000, 2)
    trans = (0.6, -0.05, 0.02)
    for quat in (None, (1.0, 0.0, 0.0, 0.0)):
        got = kr.deskew(p, trans, quat)
        ratio = np.array([kr.ratio_of(v) for v in p[:, 3]])
        want = (p[:, :3].astype(np.float64) + ratio[:, None] * np.array(trans)[None, :]).astype(np.float32)
        assert np.array_equal(_bits(got[:, :3]), _bits(want))
        assert np.array_equal(_bits(got[:, 3]), _bits(p[:, 3]))


def test_hand_made_intensity_table():
    tab = kr.intensity_table()
    r = [kr.ratio_of(v) for v in tab[:, 3]]
    # fraction 0
    assert r[0] == 0.0 and r[6] == 0.0
    # 0.05 and 0.0999 as float differences of a float near 3: what the reference's float subtraction leaves, promoted, over 0.1
    assert r[1] == float(F(F(3.05) - F(3.0))) / 0.1 and 0.49 < r[1] < 0.51
    assert r[2] == float(F(F(3.0999) - F(3.0))) / 0.1 and 0.998 < r[2] < 1.0
    # float(3.1) - 3 = 0.0999999046...: the quotient by the double 0.1 stays below 1 -- and 15.0625 (exact in float) gives exactly 0.625
    assert r[3] == float(F(F(3.1) - F(3.0))) / 0.1 and r[3] < 1.0
    assert r[8] == 0.625
    # a fraction of 0.1 on ring 0: 0.1 in float is a hair above the double 0.1, the quotient a hair above 1 -- ratio 1 by the comparison alone
    assert kr.ratio_of(F(0.1)) == 1.0 and float(F(0.1)) / 0.1 > 1.0 - 1e-15
    # 4.35: the cap
    assert r[4] == 1.0 and float(F(F(4.35) - F(4.0))) / 0.1 > 3.0
    # -0.01: (int) truncates toward zero, the ratio is negative and stays so
    assert int(F(-0.01)) == 0 and r[5] == float(F(-0.01)) / 0.1 and -0.11 < r[5] < -0.09
    # 2.5: cap; 1.1: float(1.1) - 1 = 0.10000002..., a hair over
    assert r[9] == 1.0 and r[10] == 1.0 and 1.0 < float(F(F(1.1) - F(1.0))) / 0.1 < 1.000001
    trans = (0.6, -0.05, 0.02)
    got = kr.deskew(tab, trans)
    for i in range(len(tab)):
        want = (tab[i, :3].astype(np.float64) + r[i] * np.array(trans)).astype(np.float32)
        assert np.array_equal(_bits(got[i, :3]), _bits(want)), i
    assert got[5, 0] < tab[5, 0]                         # the negative ratio moves the point AGAINST the translation
    # zero motion: bit-identical to the input, with the identity and with no quaternion
    for quat in (None, (1.0, 0.0, 0.0, 0.0)):
        assert np.array_equal(_bits(kr.deskew(tab, (0.0, 0.0, 0.0), quat)), _bits(tab))
    # ... and a general rotation at ratio 1 is the rotation itself, at ratio 0 the identity
    yaw = 0.03
    quat = (np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2))
    g = kr.deskew(tab, (0.0, 0.0, 0.0), quat)
    assert np.array_equal(_bits(g[0]), _bits(tab[0]))
    c, s = np.cos(yaw), np.sin(yaw)
    assert abs(float(g[4, 0]) - (c * -20.0 - s * -20.0)) < 1e-5 and abs(float(g[4, 1]) - (s * -20.0 + c * -20.0)) < 1e-5


def test_keyframe_cloud_is_deskew_then_voxel_grid():
    p = _random_cloud(500, 3)
    p[:, :3] *= F(0.1)
    trans = (0.6, -0.05, 0.02)
    assert np.array_equal(_bits(kr.keyframe_cloud(p, 0.9, trans)), _bits(pr.voxel_grid(kr.deskew(p, trans), 0.9)))
    assert np.array_equal(_bits(kr.keyframe_cloud(p, 0.0, trans)), _bits(kr.deskew(p, trans)))
    assert np.array_equal(_bits(kr.keyframe_cloud(p, 0.9)), _bits(pr.voxel_grid(p, 0.9)))
    assert len(kr.keyframe_cloud(p, 0.9)) < len(p)

"""The CPU restatement of Preprocessing::cloudHandler (tests/preproc_restated.py) on hand-made clouds whose labels are known on paper."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_restated as pr  # noqa: E402


def _line(n, step=0.125, x0=16.0):
    """n points on a line, spacing exact in float: every curvature is exactly 0; squared steps 0.015625 <= 0.05 (neighbours get marked)"""
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = x0 + step * np.arange(n)
    return p


def _one_ring(p, **kw):
    return pr.select(p, np.array([0]), np.array([len(p)]), **kw)


def test_sector_bounds_leave_out_the_point_at_end():
    """size 30: S = 5, E = 24; the six sectors (:550-551) cover [5, 23]: index 24 (= scanEndInd) and beyond belong to no sector"""
    out = _one_ring(_line(30), ds_leaf=0.01)               # a leaf below the spacing: every less-flat point is its own voxel
    assert len(out["surf"]) == 24 - 5
    assert np.array_equal(out["surf"][:, 0], _line(30)[5:24, 0])


def test_small_rings_are_skipped():
    """scanEndInd - scanStartInd < 6 (:542): rings of 11 or 16 points give nothing; 17 points give six one-point sectors [5] .. [10], all less flat;
    the flat 5 marks 6 .. 10, so it is the only flat"""
    for n, nsurf, nflat in ((11, 0, 0), (16, 0, 0), (17, 6, 1)):
        out = _one_ring(_line(n), ds_leaf=0.01)
        assert len(out["surf"]) == nsurf and len(out["flat"]) == nflat, n


def test_ds_rate_2_skips_odd_rings():
    p = np.vstack([_line(40), _line(40, x0=30.0)])
    out = pr.select(p, np.array([0, 40]), np.array([40, 40]), ds_rate=2, ds_leaf=0.01)
    assert len(out["surf"]) and (out["surf"][:, 0] < 30.0).all()
    out1 = pr.select(p, np.array([0, 40]), np.array([40, 40]), ds_rate=1, ds_leaf=0.01)
    assert (out1["surf"][:, 0] >= 30.0).any()


def test_fourth_flat_pick_marks_no_neighbours():
    """size 125: sectors of 19 points, sector 0 = [5, 23].  Equal curvatures (0) rank by index: flats 5, 11, 17 (each marks +-5), then 23 -- the
    4th, which breaks BEFORE marking (:609-613), so sector 1's first flat is 24 (29 had 23 marked its neighbours)"""
    p = _line(125)
    out = _one_ring(p)
    assert list(out["flat"][:5, 0]) == list(p[[5, 11, 17, 23, 24], 0])


def test_neighbour_marks_cross_into_the_next_sector():
    """size 113: sectors of 17 points, sector 0 = [5, 21], sector 1 = [22, 38].  Sector 0's flats 5, 11, 17; 17 marks 18 .. 22 -- 22 is sector 1's
    first point, so sector 1 starts its flats at 23: 23, 29, 35 (the sectors of a ring are sequential)"""
    p = _line(113)
    out = _one_ring(p)
    assert list(out["flat"][:6, 0]) == list(p[[5, 11, 17, 23, 29, 35], 0])


def test_edges_break_on_the_eleventh():
    """every point a corner (a zigzag with steps far above 0.05: no marks): per sector 2 sharp + 8 more less-sharp, the 11th breaks (:568-577)"""
    n = 6 * 30 + 11
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = 20.0 + np.arange(n)
    p[:, 1] = np.where(np.arange(n) % 2 == 0, 2.0, -2.0)
    out = _one_ring(p)
    assert len(out["sharp"]) == 12 and len(out["less_sharp"]) == 60
    assert (out["label"] == 1).sum() == 48 and (out["label"] == 2).sum() == 12


def _pt(angle_deg, r=10.0):
    e = math.radians(angle_deg)
    return np.array([[r * math.cos(e), 0.0, r * math.sin(e)]], np.float32)


def test_32_line_truncation_maps_just_below_the_lowest_bin_to_ring_0():
    """int((angle + 92/3) * 3/4) truncates toward zero: a coordinate in (-1, 0) is ring 0, not rejected"""
    sid, _ = pr.scan_ids(_pt(-92.0 / 3.0 - 0.5), 32)
    assert sid[0] == 0
    sid, _ = pr.scan_ids(_pt(-92.0 / 3.0 - 1.5), 32)
    assert sid[0] == -1


def test_64_line_rejects_rings_above_50():
    sid, _ = pr.scan_ids(_pt(-24.0), 64)                   # 32 + int((-8.83 + 24) * 2 + 0.5) = 62 > 50
    assert sid[0] == -1
    sid, _ = pr.scan_ids(_pt(-16.5), 64)                   # 32 + int(15.34 + 0.5) = 47
    assert sid[0] == 47
    sid, _ = pr.scan_ids(_pt(1.0), 64)                     # int((2 - 1) * 3 + 0.5) = 3
    assert sid[0] == 3
    sid, _ = pr.scan_ids(_pt(2.5), 64)
    assert sid[0] == -1

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


# ------------------------------------------------------------------------------------------------ the orientation state machine on paper
# Hand-placed 16-line scans at range 10 m.  A point at azimuth az has ori = -atan2(y, x) = -az (:489), so below "ori" is minus the azimuth
# written in the test, in degrees.  startOri = ori of the first survivor (:401); endOri = ori of the last survivor + 360 (:402-404), minus 360 if
# endOri - startOri > 540 (:406), plus 360 if it is < 180 (:409).  Before halfPassed (:490-497): ori + 360 if ori < startOri - 90 (:491), ori - 360
# if ori > startOri + 270 (:493), then halfPassed is set if ori - startOri > 180 -- AFTER this point's ori is final.  After it (:499-504): ori + 360,
# then + 360 if that is < endOri - 270 (:501), - 360 if it is > endOri + 90 (:503).  relTime = (ori - startOri) / (endOri - startOri) (:507).
# Every azimuth is at least 5 degrees from every constant it is compared with.  The lasers at +1 deg are ring int((1 + 15) / 2 + 0.5) = 8; an
# elevation of 20 deg gives int((20 + 15) / 2 + 0.5) = 17 > 15: rejected (:443-446).
RING = 8
REL_TOL = 2 * float(np.spacing(np.float32(RING + 0.1))) / 0.1          # two float spacings of the ring's intensity, through intensity = ring + 0.1 relTime: 1.9e-5


def _at(az_deg, elev_deg=1.0, r=10.0):
    a, e = math.radians(az_deg), math.radians(elev_deg)
    return [r * math.cos(e) * math.cos(a), r * math.cos(e) * math.sin(a), r * math.sin(e), 0.0]


def _rel_of(points, want_kept=None):
    """relTime of the valid points in raw order (one ring: the bucketing keeps the order), and the report"""
    raw = np.array(points, np.float32)
    cut, _, size, kept, sid = pr.project(raw, 16)
    rep = pr.orientation_report(raw, 16)
    assert size[RING] == len(cut) == (sid >= 0).sum() and kept == (len(points) if want_kept is None else want_kept)
    rel = (cut[:, 3].astype(np.float64) - RING) / 0.1
    assert np.abs(rel - rep["rel"]).max() <= REL_TOL and rep["margin"] > math.radians(4.9)
    return rel, rep


def _branches(rep):
    return {k for k in ("n491", "n493", "n501", "n503") if rep[k]} | {k for k in ("end_minus", "end_plus") if rep[k]}


def _check(rel, want):
    assert len(rel) == len(want) and np.abs(rel - np.array(want)).max() <= REL_TOL, (rel, want)


def test_orientation_clean_turn_takes_503_only():
    """ori -40, 60, 130, 150, 170, -120, -50.  start -40, end -50 + 360 = 310, span 350: no adjustment.  60: 100 / 350.  130: 170 / 350 (170 < 180:
    not yet half).  150: 190 / 350, and 190 > 180 sets halfPassed.  170: + 360 = 530 > 310 + 90 -> 170 (:503): 210 / 350.  -120: 240, between 40 and
    400: 280 / 350.  -50: 310: 350 / 350"""
    rel, rep = _rel_of([_at(40), _at(-60), _at(-130), _at(-150), _at(-170), _at(120), _at(50)])
    _check(rel, [0.0, 0.2857143, 0.4857143, 0.5428571, 0.6, 0.8, 1.0])
    assert _branches(rep) == {"n503"} and rep["n503"] == 1 and rep["half_passed"] and rep["half"] == 3


def test_orientation_first_half_plus_491():
    """ori 140, 170, -170, -100, -30, 40, 130.  start 140, end 130 + 360 = 490, span 350.  170: 30 / 350.  -170 < 140 - 90 = 50 -> 190 (:491): 50 / 350.
    -100 -> 260 (:491): 120 / 350.  -30 -> 330 (:491): 190 / 350, sets halfPassed.  40: 400, between 220 and 580: 260 / 350.  130: 490: 1"""
    rel, rep = _rel_of([_at(-140), _at(-170), _at(170), _at(100), _at(30), _at(-40), _at(-130)])
    _check(rel, [0.0, 0.0857143, 0.1428571, 0.3428571, 0.5428571, 0.7428571, 1.0])
    assert _branches(rep) == {"n491"} and rep["n491"] == 3 and rep["half"] == 4


def test_orientation_end_minus_406_on_a_partial_turn():
    """ori -100, -40, 50, 85, 100.  start -100, end 100 + 360 = 460, span 560 > 540 -> end 100 (:406), span 200.  -40: 60 / 200.  50: 150 / 200.
    85: 185 / 200, sets halfPassed.  100: 460 > 100 + 90 -> 100 (:503): 1"""
    rel, rep = _rel_of([_at(100), _at(40), _at(-50), _at(-85), _at(-100)])
    _check(rel, [0.0, 0.3, 0.75, 0.925, 1.0])
    assert _branches(rep) == {"end_minus", "n503"} and rep["half"] == 3


def test_orientation_end_plus_409_and_half_never_passed():
    """ori 100, 150, -170, -150: 110 degrees of a turn.  start 100, end -150 + 360 = 210, span 110 < 180 -> end 570 (:409), span 470.  150: 50 / 470.
    -170 < 10 -> 190 (:491): 90 / 470.  -150 -> 210 (:491): 110 / 470.  No ori - start exceeds 180: halfPassed stays false"""
    rel, rep = _rel_of([_at(-100), _at(-150), _at(170), _at(150)])
    _check(rel, [0.0, 0.1063830, 0.1914894, 0.2340426])
    assert _branches(rep) == {"end_plus", "n491"} and not rep["half_passed"] and rep["half"] == 4


def test_orientation_first_half_minus_493_gives_a_negative_reltime():
    """ori -140, 150, -100, 0, 60, 170: the second point lies BEHIND the start.  start -140, end 170 + 360 = 530, span 670 > 540 -> end 170 (:406),
    span 310.  150 > -140 + 270 = 130 -> -210 (:493): -70 / 310.  -100: 40 / 310.  0: 140 / 310.  60: 200 / 310, sets halfPassed.  170: 530 > 260 ->
    170 (:503): 1"""
    rel, rep = _rel_of([_at(140), _at(-150), _at(100), _at(0), _at(-60), _at(-170)])
    _check(rel, [0.0, -0.2258065, 0.1290323, 0.4516129, 0.6451613, 1.0])
    assert _branches(rep) == {"end_minus", "n493", "n503"} and rep["n493"] == 1 and rep["rel_min"] < -0.2


def test_orientation_second_half_plus_501_on_an_over_full_turn():
    """ori 115, 170, -150, -60, 0, 100, -178, -175: 430 degrees.  start 115, end -175 + 360 = 185, span 70 < 180 -> end 545 (:409), span 430.
    170: 55 / 430.  -150 < 25 -> 210 (:491): 95 / 430.  -60 -> 300 (:491): 185 / 430, sets halfPassed.  0: 360, between 275 and 635: 245 / 430.
    100: 460: 345 / 430.  -178: 182 < 545 - 270 = 275 -> 542 (:501): 427 / 430.  -175: 185 -> 545 (:501): 1"""
    rel, rep = _rel_of([_at(-115), _at(-170), _at(150), _at(60), _at(0), _at(-100), _at(178), _at(175)])
    _check(rel, [0.0, 0.1279070, 0.2209302, 0.4302326, 0.5697674, 0.8023256, 0.9930233, 1.0])
    assert _branches(rep) == {"end_plus", "n491", "n501"} and rep["n501"] == 2 and rep["half"] == 3


def test_orientation_the_point_that_sets_half_passed_keeps_its_first_branch_value():
    """ori -100, 0, 100, 105, 40: 500 degrees.  start -100, end 40 + 360 = 400, span 500: no adjustment.  0: 100 / 500.  100: 200 / 500, sets
    halfPassed -- on the second branch it would be 460, between 130 and 490: 560 / 500 = 1.12.  105: 465 < 490: 565 / 500, beyond 1.  40: 400: 1"""
    rel, rep = _rel_of([_at(100), _at(0), _at(-100), _at(-105), _at(-40)])
    _check(rel, [0.0, 0.2, 0.4, 1.13, 1.0])
    assert _branches(rep) == set() and rep["half"] == 2 and rep["rel_max"] > 1.1


def test_orientation_a_rejected_ring_does_not_set_half_passed():
    """as above with a point of elevation 20 deg (rejected, :443-446) at ori 100 before a valid one at ori 90.  The continue comes before :489: the
    rejected point sets nothing.  90: 190 / 500 and sets halfPassed itself; had the rejected point set it, 90 -> 450: 550 / 500 = 1.1"""
    rel, rep = _rel_of([_at(100), _at(-100, 20.0), _at(-90), _at(-105), _at(-40)])
    _check(rel, [0.0, 0.38, 1.13, 1.0])
    assert rep["half"] == 2 and rep["half_passed"]


def test_orientation_rejected_first_and_last_survivors_still_define_start_and_end():
    """the clean turn with its first (ori -40) and last (ori -50) point at elevation 20 deg: rejected rings, but :401-404 read them before any ring
    is computed.  start -40, end 310.  60: 100 / 350.  150: 190 / 350, sets halfPassed.  170 (:503): 210 / 350.  -120: 280 / 350.
    (With start and end from the first and last VALID point, 60 and -120 + 360, the second relTime would be 90 / 180.)"""
    rel, rep = _rel_of([_at(40, 20.0), _at(-60), _at(-150), _at(-170), _at(120), _at(50, 20.0)])
    _check(rel, [0.2857143, 0.5428571, 0.6, 0.8])
    assert _branches(rep) == {"n503"} and rep["half"] == 2


def test_orientation_start_and_end_come_from_the_first_and_last_survivor():
    """the clean turn between leading and trailing NaN points and points inside min_range (1 m and 2 m, at ori 0 and 90): the same relTime"""
    nan = [float("nan"), 1.0, 1.0, 0.0]
    pts = [nan, _at(0, r=1.0), _at(40), _at(-60), _at(-130), _at(-150), _at(-170), _at(120), _at(50), _at(-90, r=2.0), nan]
    rel, rep = _rel_of(pts, want_kept=7)
    _check(rel, [0.0, 0.2857143, 0.4857143, 0.5428571, 0.6, 0.8, 1.0])
    assert _branches(rep) == {"n503"}


def test_orientation_paper_cases_reach_all_six_branches():
    """(a summary of the above, so that dropping a case shows)"""
    scans = [[_at(40), _at(-60), _at(-130), _at(-150), _at(-170), _at(120), _at(50)], [_at(-140), _at(-170), _at(170), _at(100), _at(30), _at(-40), _at(-130)],
             [_at(100), _at(40), _at(-50), _at(-85), _at(-100)], [_at(-100), _at(-150), _at(170), _at(150)],
             [_at(140), _at(-150), _at(100), _at(0), _at(-60), _at(-170)], [_at(-115), _at(-170), _at(150), _at(60), _at(0), _at(-100), _at(178), _at(175)]]
    seen = set()
    for s in scans:
        seen |= _branches(pr.orientation_report(np.array(s, np.float32), 16))
    assert seen == {"end_minus", "end_plus", "n491", "n493", "n501", "n503"}

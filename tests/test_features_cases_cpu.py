"""The cases of tests/features_cases.py do what they claim (CPU only): every orientation case reaches its branches on the restatement with a margin
no atan2f can cross, every option changes the restatement's output, the hand-made rows stay in their rings and give the picks derived on paper
in tests/test_preproc_restated.py, and every q_imu form takes the slerp arm it is named after."""
import math

import numpy as np
import pytest

import features_cases as fc
import preproc_restated as pr

BRANCHES = ("end_minus", "end_plus", "n491", "n493", "n501", "n503")


def _fired(rep):
    return {k for k in BRANCHES if rep[k]}


def _line(name, rep):
    return (f"{name}: :406 {int(rep['end_minus'])} :409 {int(rep['end_plus'])} :491 {rep['n491']} :493 {rep['n493']} :501 {rep['n501']} :503 {rep['n503']} "
            f"half {rep['half_passed']} relTime [{rep['rel_min']:.4f}, {rep['rel_max']:.4f}] margin {rep['margin']:.2e} rad")


# ------------------------------------------------------------------------------------------------ orientation
@pytest.mark.parametrize("name", fc.ORIENTATION_NAMES)
def test_orientation_case_reaches_its_branches(name):
    raw, claim = fc.orientation_scan(name), fc.orientation_claim(name)
    rep = pr.orientation_report(raw, fc.N_SCANS)
    print(_line(name, rep), f"({len(raw)} points)")
    assert 4000 <= len(raw) <= 6300 or name in ("a_partial", "b_never_half")
    assert claim["reach"] <= _fired(rep), (claim["reach"], _fired(rep))
    if claim.get("only"):
        assert _fired(rep) == claim["reach"]
    assert rep["half_passed"] == claim.get("half", True)
    lo, hi = claim["rel"]
    assert lo - 1e-6 <= rep["rel_min"] and rep["rel_max"] <= hi + 1e-6          # (the lasers of the first column differ by an ulp of atan2f: -2e-8)
    if claim.get("outside"):
        assert rep["rel_min"] < 0.0 and rep["rel_max"] > 1.0
    if claim.get("half_differs"):
        # the point that sets halfPassed keeps its first-branch value; the next valid point (the same column) is a whole turn later
        sid = pr.project(raw, fc.N_SCANS)[4]
        k = int((sid[:rep["half"]] >= 0).sum())
        print(f"{name}: relTime {rep['rel'][k]:.4f} at the point that sets halfPassed, {rep['rel'][k + 1]:.4f} at the next")
        assert rep["rel"][k + 1] - rep["rel"][k] > 0.7
    assert rep["margin"] >= fc.MARGIN


def test_orientation_figures_of_the_cases():
    """the figures the case table quotes"""
    rep = {n: pr.orientation_report(fc.orientation_scan(n), fc.N_SCANS) for n in fc.ORIENTATION_NAMES}
    assert 400 <= rep["c_first_plus"]["n491"] <= 650
    assert 0.27 <= rep["b_never_half"]["rel_max"] <= 0.29 and rep["b_never_half"]["half"] == len(pr.survivors(fc.orientation_scan("b_never_half")[:, :3]))
    assert 250 <= rep["reversed_1"]["n493"] <= 400 and rep["reversed_1"]["rel_min"] < -0.2 and rep["reversed_1"]["rel_max"] > 1.2
    assert rep["reversed_2"]["n501"] > 1000 and rep["reversed_2"]["rel_min"] < -0.2 and rep["reversed_2"]["rel_max"] > 1.2
    assert -0.05 < rep["jitter"]["rel_min"] < 0 and 1 < rep["jitter"]["rel_max"] < 1.05


def test_orientation_cases_reach_all_six_branches_together():
    seen = set()
    for n in fc.ORIENTATION_NAMES:
        seen |= _fired(pr.orientation_report(fc.orientation_scan(n), fc.N_SCANS))
    assert seen == set(BRANCHES)


def test_reltime_outside_0_1_reaches_the_negative_ratio_and_the_ring_below():
    """what relTime < 0 leads to (reference :178-181): on ring 0 the intensity is negative, int() truncates toward zero and the ratio is negative; on
    rings >= 1 int(intensity) is the ring below and the ratio is capped at 1"""
    for name in ("reversed_1", "reversed_2", "jitter"):
        cut = pr.project(fc.orientation_scan(name), fc.N_SCANS)[0]
        inten = cut[:, 3]
        ring = np.rint(inten.astype(np.float64)).astype(int)
        neg0 = int(((ring == 0) & (inten < 0)).sum())
        below = int(((ring >= 1) & (inten.astype(int) == ring - 1)).sum())
        print(f"{name}: {neg0} points of ring 0 with a negative intensity, {below} points whose int(intensity) is the ring below")
        assert neg0 > 0 and below > 0


def test_edges_dropped_takes_start_and_end_from_the_first_and_last_survivor():
    raw, base = fc.orientation_scan("edges_dropped"), fc.orientation_scan("baseline")
    keep = pr.survivors(raw[:, :3])
    assert keep[0] >= 3 * fc.N_SCANS and keep[-1] < len(raw) - 3 * fc.N_SCANS
    assert np.isnan(raw[:fc.N_SCANS, 0]).all() and not np.isnan(raw[fc.N_SCANS:2 * fc.N_SCANS, 0]).all(), "both kinds of dropped points"
    rep, rep0 = pr.orientation_report(raw, fc.N_SCANS), pr.orientation_report(base, fc.N_SCANS)
    p0, p1 = raw[keep[0]], raw[keep[-1]]
    assert rep["start"] == float(-pr.atan2f(p0[1], p0[0]))
    assert rep["end"] == float(pr.F(float(-pr.atan2f(p1[1], p1[0])) + 2 * math.pi))
    assert rep["start"] - rep0["start"] > 0.05 and rep0["end"] - rep["end"] > 0.05, "three columns of 2 pi / 301 each"


def test_column_counts_divisible_by_4_sit_on_the_thresholds():
    """why 301: with 300 columns a column lies a half turn from the start, within float rounding of the halfPassed threshold"""
    import glio_amd.synth_lidar as sl
    rep = pr.orientation_report(sl.make_scan(fc.N_SCANS, 300, start_az=2.0, seed=fc.SEED).reshape(300, fc.N_SCANS, 4)[::-1].reshape(-1, 4), fc.N_SCANS)
    print(f"300 columns reversed: margin {rep['margin']:.2e} rad")
    assert rep["margin"] < 1e-6


# ------------------------------------------------------------------------------------------------ options
def _differs(a, b):
    return any(not fc._same(a[k], b[k]) for k in ("cut", "sharp", "less_sharp", "flat", "surf"))


@pytest.fixture(scope="module")
def default_out():
    return pr.extract(fc.orientation_scan("baseline"), fc.N_SCANS)


@pytest.mark.parametrize("name", list(fc.SELECT_OPTIONS))
def test_selection_option_changes_the_output(name, default_out):
    out = pr.extract(fc.orientation_scan("baseline"), fc.N_SCANS, **fc.SELECT_OPTIONS[name])
    assert fc._same(out["cut"], default_out["cut"]), "a selection option leaves the cut cloud alone"
    changed = [k for k in ("sharp", "less_sharp", "flat", "surf") if not fc._same(out[k], default_out[k])]
    print(name, "changes", changed, {k: (len(default_out[k]), len(out[k])) for k in changed})
    assert changed
    if name.startswith("ds_rate"):
        rate = fc.SELECT_OPTIONS[name]["ds_rate"]
        rings = np.unique(np.rint(out["surf"][:, 3].astype(np.float64)).astype(int))
        assert len(rings) > 1 and (rings % rate == 0).all() and len(np.unique(np.rint(default_out["surf"][:, 3]))) > len(rings)


def test_projection_options_change_the_output(default_out):
    cases = fc.project_options()
    raw, kw, q = cases["min_range_10"]
    out = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw)
    assert 0 < out["kept"] < default_out["kept"]
    raw, kw, q = cases["q_lb_yaw"]
    out, plain = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw), pr.extract(raw, fc.N_SCANS, q_imu=q)
    d = np.linalg.norm(out["cut"][:, :3].astype(np.float64) - plain["cut"][:, :3], axis=1)
    print(f"q_lb under a yaw of {fc.YAW}: moves the cut cloud by up to {d.max():.3f} m")
    assert out["cut"].shape == plain["cut"].shape and d.max() > 0.01
    assert abs(np.linalg.norm(fc.q_lb_tilted()) - 1) < 1e-15 and np.abs(fc.q_lb_tilted()[1:]).min() > 0.004
    # with q_imu = identity the sandwich q_lb * 1 * q_lb^-1 is the identity up to rounding: the case then checks that rounding, bit for bit
    raw, kw, q = cases["q_lb_identity_imu"]
    out = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw)
    n = int((fc._bits(out["cut"][:, :3]) != fc._bits(default_out["cut"][:, :3])).any(1).sum())
    print(f"q_lb with q_imu = identity: {n} of {len(out['cut'])} points differ in a bit from the identity sandwich")


def test_near_origin_row_reaches_ft_near():
    raw, kw, q = fc.project_options()["min_range_0.2_near"]
    sid, _ = pr.scan_ids(raw[:, :3], fc.N_SCANS)
    assert (sid == 8).all()
    near = (raw[:, 0].astype(np.float64) ** 2 + raw[:, 1].astype(np.float64) ** 2) < 0.25
    assert near.sum() == 13
    rep = pr.orientation_report(raw, fc.N_SCANS, min_range=kw["min_range"])
    print(_line("near-origin row", rep))
    assert rep["margin"] >= fc.MARGIN
    out = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw)
    assert out["kept"] == len(raw) == len(out["cut"]) and _differs(out, pr.extract(raw, fc.N_SCANS))
    key = lambda a: {p[:3].tobytes() for p in a}
    near_pts = key(raw[near])
    assert near_pts <= key(out["cut"]) and not (near_pts & key(out["flat"])) and not (near_pts & key(out["surf"]))
    assert len(out["flat"]) > 0 and len(out["surf"]) > 0
    # without the skip a near point WOULD be picked: all curvatures of the row's interior are 0, below the threshold
    assert (out["curv"][near][:] < 0.1).all()


# ------------------------------------------------------------------------------------------------ hand-made rings
def test_hand_rows_stay_in_their_rings_and_give_the_paper_picks():
    raw = fc.hand_rings()
    sid, _ = pr.scan_ids(raw[:, :3], fc.N_SCANS)
    for n, x0, z, ring in fc.HAND_ROWS:
        mine = raw[:, 2] == np.float32(z)
        assert mine.sum() == n and (sid[mine] == ring).all(), (z, ring)
    assert (np.diff(sid[:10]) != 0).any(), "interleaved: the bucketing has to reorder"
    rep = pr.orientation_report(raw, fc.N_SCANS)
    print(_line("hand rings", rep))
    assert rep["margin"] > 1.5 and rep["rel_min"] == rep["rel_max"] == 0.0
    out = pr.extract(raw, fc.N_SCANS, ds_leaf=fc.HAND_LEAF)
    assert list(out["ring_size"]) == [0, 0, 0, 0, 0, 11, 17, 0, 125, 113, 16, 0, 0, 0, 0, 0]
    assert fc._same(out["cut"][:, :3], np.vstack([fc._row(n, x0, z) for n, x0, z, _ in sorted(fc.HAND_ROWS, key=lambda r: r[3])])[:, :3])
    fc.check_hand_picks(out)


def test_small_rings_alone():
    out = pr.extract(fc.small_rings(), fc.N_SCANS, ds_leaf=fc.HAND_LEAF)
    assert list(out["ring_size"][[5, 6, 10]]) == [11, 17, 16] and len(out["flat"]) == 1 and len(out["surf"]) == 6


def test_zigzag_is_one_ring_of_tied_curvatures():
    raw = fc.zigzag()
    sid, _ = pr.scan_ids(raw[:, :3], fc.N_SCANS)
    assert (sid == 8).all()
    rep = pr.orientation_report(raw, fc.N_SCANS)
    print(_line("zigzag", rep))
    assert rep["margin"] > 1.0 and not rep["half_passed"]
    out = pr.extract(raw, fc.N_SCANS)
    assert fc._same(out["cut"][:, :3], raw[:, :3])
    S, E = 5, len(raw) - 6
    c = out["curv"][S:E]
    tied = int(sum((c == v).sum() for v in np.unique(c) if (c == v).sum() > 1))
    print(f"zigzag: {tied} of {len(c)} sector points share their curvature with another ({np.unique(c)})")
    assert tied == len(c) == 180 and np.unique(c).tolist() == [576.0]
    assert len(out["sharp"]) == 12 and len(out["less_sharp"]) == 60
    fc.check_zigzag_order(out)


# ------------------------------------------------------------------------------------------------ q_imu
def test_axis_rows_have_exact_orientations():
    raw = fc.axis_rows()
    sid, _ = pr.scan_ids(raw[:, :3], fc.N_SCANS)
    assert (sid == 8).all()
    rep = pr.orientation_report(raw, fc.N_SCANS)
    print(_line("axis rows", rep))
    assert rep["margin"] > 1.5 and rep["start"] == 0.0 and rep["end"] == float(np.float32(float(np.float32(math.pi / 2)) + 2 * math.pi))
    assert (rep["rel"][:fc.AXIS_ROW] == 0).all() and np.abs(rep["rel"][fc.AXIS_ROW:] - 0.2).max() < 1e-6


def test_q_imu_forms_take_their_slerp_arms():
    forms = fc.q_imu_forms()
    for name, (q, branch, unit) in forms.items():
        norm = float(np.linalg.norm(q))
        print(f"{name}: q = {q}, |q| - 1 = {norm - 1:.3e}, {fc.slerp_branch(q)}")
        assert fc.slerp_branch(q) == branch, name
        assert (abs(norm - 1) < 1e-15) == unit or (unit and abs(norm - 1) < 1e-15), name
        if not unit:
            assert abs(norm - 1) > 1e-7, name
    assert forms["negated_yaw"][0][0] < 0
    q = forms["scan_rotation"][0]
    assert 0.03 < 2 * np.linalg.norm(q[1:]) < 0.07, "about 0.5 rad/s over 0.1 s"
    raw = fc.orientation_scan("baseline")
    plain = pr.extract(raw, fc.N_SCANS)
    for name, (q, _, _) in forms.items():
        assert _differs(pr.extract(raw, fc.N_SCANS, q_imu=q), plain), name
    # -q is the same rotation: the restatement gives the same cloud within rounding
    a, b = pr.extract(raw, fc.N_SCANS, q_imu=forms["negated_yaw"][0]), pr.extract(raw, fc.N_SCANS, q_imu=-forms["negated_yaw"][0])
    assert a["cut"].shape == b["cut"].shape and fc.position_gate(a["cut"], b["cut"]) <= 0

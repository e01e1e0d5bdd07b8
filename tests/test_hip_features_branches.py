"""glio_features_* on the inputs of tests/features_cases.py: every adjustment of the orientation state machine (reference Preprocessing.cpp:406,
:409, :491, :493, :501, :503), a scan that never sets halfPassed, relTime outside [0, 1] (a negative de-skew ratio on ring 0, int(intensity) the
ring below on the others), every option away from its default, tied curvatures, rings of 11 / 16 / 17 points, marks that cross sectors, the
q_imu forms production hands over, and a context that is reused or reconfigured -- against the restatement tests/preproc_restated.py, whose
orientation half tests/test_preproc_restated.py pins on paper.  tests/test_features_cases_cpu.py shows that the cases reach those branches
with a margin no atan2f can cross.

Gates are those of tests/test_hip_features.py: bit-identical xyz wherever only IEEE + - * / sqrt and comparisons are involved, intensities
within 2 float ulps of the ring's value (atan2f), positions within 2e-6 * range + 1e-6 m where the slerp goes through acos / sin."""
import functools

import numpy as np
import pytest

import features_cases as fc
import preproc_restated as pr
from features_cases import IDENTITY, OUTPUTS, _intensity_close, _same, _yaw_q
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu

ALL = OUTPUTS + [("cut", T.FEAT_CUT_CLOUD)]
KW = ("ds_rate", "edge_threshold", "surf_threshold", "ds_leaf")


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


def _context(hip, n_scans, n_points, **kw):
    from glio_amd import synth
    ctx = hip.Context(synth.default_opts(1, pts=1 << 16, map_pts=1 << 16))
    ctx.features_config(fc.device_opts(n_scans, max(n_points, 1), **kw))
    return ctx


def _run(hip, raw, q_imu=IDENTITY, n_scans=fc.N_SCANS, **kw):
    """one extraction on a fresh context sized to the scan: (counts, {output: array})"""
    ctx = _context(hip, n_scans, len(raw), **kw)
    cnt = ctx.features_extract(raw, q_imu)
    out = {name: ctx.features_read(which) for name, which in ALL}
    ctx.close()
    return cnt, out


@functools.lru_cache(maxsize=None)
def _want_orientation(name, yaw):
    """the restatement on an orientation case: computed once, shared, never modified"""
    out = pr.extract(fc.orientation_scan(name), fc.N_SCANS, q_imu=tuple(_yaw_q(yaw)))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _select_kw(kw):
    return {k: v for k, v in kw.items() if k in KW}


def _assert_selection_of_own_cut(cnt, got, n_scans=fc.N_SCANS, **kw):
    """steps 4-6 restated on the device's own cut cloud: every output bit for bit, the counts equal"""
    rs, size = pr.rings_of_cut(got["cut"], n_scans)
    want = pr.select(got["cut"], rs, size, **_select_kw(kw))
    for name, _ in OUTPUTS:
        assert _same(got[name], want[name]), (name, got[name].shape, want[name].shape)
    assert (cnt.sharp, cnt.less_sharp, cnt.flat, cnt.surf) == tuple(len(want[k]) for k in ("sharp", "less_sharp", "flat", "surf"))
    return want


def _assert_bit_identical_xyz(cnt, got, want, n_scans=fc.N_SCANS):
    """the assertions of test_end_to_end_from_the_raw_scan_identity_rotation"""
    assert cnt.kept == want["kept"] and cnt.cut == len(want["cut"]) == len(got["cut"])
    assert np.array_equal(pr.rings_of_cut(got["cut"], n_scans)[1], want["ring_size"])
    assert _same(got["cut"][:, :3], want["cut"][:, :3])
    assert _intensity_close(got["cut"][:, 3], want["cut"][:, 3])
    for name, _ in OUTPUTS:
        assert got[name].shape == want[name].shape and _same(got[name][:, :3], want[name][:, :3]), name
        assert len(want[name]) == 0 or _intensity_close(got[name][:, 3], want[name][:, 3]), name
    assert (cnt.sharp, cnt.less_sharp, cnt.flat, cnt.surf) == tuple(len(want[k]) for k in ("sharp", "less_sharp", "flat", "surf"))


def _assert_within_the_gate(cnt, got, want, n_scans=fc.N_SCANS):
    """the assertions of test_end_to_end_with_a_sweep_rotation: the same counts and order, positions within 2e-6 * range + 1e-6 m"""
    assert cnt.kept == want["kept"] and cnt.cut == len(want["cut"])
    assert np.array_equal(pr.rings_of_cut(got["cut"], n_scans)[1], want["ring_size"])
    for name, _ in ALL:
        assert got[name].shape == want[name].shape, name
        excess = fc.position_gate(got[name], want[name])
        print(f"{name}: {len(want[name])} points, worst error - gate {excess:.2e} m")
        assert excess <= 0, (name, excess)
    assert _intensity_close(got["cut"][:, 3], want["cut"][:, 3])


# ------------------------------------------------------------------------------------------------ orientation
@pytest.mark.parametrize("name", fc.ORIENTATION_NAMES)
def test_orientation_case_identity_rotation(hip, name):
    """q_imu = identity: kept, cut and the ring sizes equal, the cut cloud's xyz bit-identical, every intensity within 2 ulps of its ring's value (a
    branch taken the other way moves relTime by 2 pi / (endOri - startOri): five orders above the gate), all four outputs bit-identical in xyz"""
    raw = fc.orientation_scan(name)
    cnt, got = _run(hip, raw)
    assert cnt.in_ == len(raw)
    _assert_bit_identical_xyz(cnt, got, _want_orientation(name, 0.0))


@pytest.mark.parametrize("name", fc.ROTATED_NAMES)
def test_orientation_case_with_a_sweep_rotation(hip, name):
    """a yaw of 0.1 rad: where relTime leaves [0, 1] the negative ratio on ring 0 and the ratio 1 behind int(intensity) = ring - 1 meet a real rotation.
    Counts and order equal, positions within the gate; and the selection restated on the device's own cut cloud bit for bit"""
    cnt, got = _run(hip, fc.orientation_scan(name), _yaw_q(fc.YAW))
    _assert_within_the_gate(cnt, got, _want_orientation(name, fc.YAW))
    _assert_selection_of_own_cut(cnt, got)


# ------------------------------------------------------------------------------------------------ options
@pytest.mark.parametrize("name", list(fc.SELECT_OPTIONS))
def test_selection_option(hip, name):
    """ds_rate, the thresholds and the leaf away from their defaults: pr.select with the same options on the device's cut cloud, bit for bit"""
    kw = fc.SELECT_OPTIONS[name]
    cnt, got = _run(hip, fc.orientation_scan("baseline"), **kw)
    want = _assert_selection_of_own_cut(cnt, got, **kw)
    default = pr.select(got["cut"], *pr.rings_of_cut(got["cut"], fc.N_SCANS))
    assert any(not _same(want[k], default[k]) for k, _ in OUTPUTS), "the option matters on this cloud"


def test_min_range_10(hip):
    raw, kw, q = fc.project_options()["min_range_10"]
    cnt, got = _run(hip, raw, q, **kw)
    want = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw)
    assert cnt.kept < _want_orientation("baseline", 0.0)["kept"]
    _assert_bit_identical_xyz(cnt, got, want)


def test_min_range_below_half_a_metre_reaches_the_near_point_skip(hip):
    """min_range 0.2 on a row passing 0.25 m from the origin: the 13 points with a squared norm below 0.25 stay in the cut cloud and are skipped by
    the flat picks and the less-flat cloud (:603, :641)"""
    raw, kw, q = fc.project_options()["min_range_0.2_near"]
    cnt, got = _run(hip, raw, q, **kw)
    want = pr.extract(raw, fc.N_SCANS, q_imu=q, **kw)
    _assert_bit_identical_xyz(cnt, got, want)
    key = lambda a: {p[:3].tobytes() for p in a}
    near = raw[(raw[:, 0].astype(np.float64) ** 2 + raw[:, 1].astype(np.float64) ** 2) < 0.25]
    assert len(near) == 13 and key(near) <= key(got["cut"])
    assert not (key(near) & key(got["flat"])) and not (key(near) & key(got["surf"])) and len(got["flat"]) > 0 and len(got["surf"]) > 0


def test_q_lb_with_identity_q_imu_is_bit_identical(hip):
    """q_lb * q_si * q_lb^-1 with q_si = (1 - t) + t: IEEE + - * / in double only, contraction off"""
    raw, kw, q = fc.project_options()["q_lb_identity_imu"]
    cnt, got = _run(hip, raw, q, **kw)
    _assert_bit_identical_xyz(cnt, got, pr.extract(raw, fc.N_SCANS, q_imu=q, **kw))


def test_q_lb_with_a_sweep_rotation(hip):
    raw, kw, q = fc.project_options()["q_lb_yaw"]
    cnt, got = _run(hip, raw, q, **kw)
    _assert_within_the_gate(cnt, got, pr.extract(raw, fc.N_SCANS, q_imu=q, **kw))
    _assert_selection_of_own_cut(cnt, got)


# ------------------------------------------------------------------------------------------------ hand-made rings
def _assert_all_bits(cnt, got, want):
    for name, _ in ALL:
        assert _same(got[name], want[name]), (name, got[name].shape, want[name].shape)
    assert (cnt.kept, cnt.cut, cnt.sharp, cnt.less_sharp, cnt.flat, cnt.surf) == (want["kept"],) + tuple(len(want[k]) for k in ("cut", "sharp", "less_sharp", "flat", "surf"))


def test_hand_made_rings_bit_for_bit(hip):
    """five exact rows interleaved in the raw order (rings 8, 9, 6, 10, 5 of 125, 113, 17, 16 and 11 points; empty rings between): every curvature 0,
    so every pick is a tie decided by index.  Every output, intensities included (y = 0: relTime is exactly 0), bit for bit, and the indices derived
    on paper: the 4th flat marks nothing (5, 11, 17, 23, 24), marks cross into the next sector (.., 17, 23, 29, ..), 17 points give one flat and six
    surf points, 16 and 11 give nothing"""
    raw = fc.hand_rings()
    cnt, got = _run(hip, raw, ds_leaf=fc.HAND_LEAF)
    want = pr.extract(raw, fc.N_SCANS, ds_leaf=fc.HAND_LEAF)
    _assert_all_bits(cnt, got, want)
    fc.check_hand_picks(got)


def test_zigzag_ties_are_ranked_by_index(hip):
    """191 corners of one curvature (576) in ring 8: 12 sharp and 60 less-sharp points whose ORDER is the assertion (the highest index first)"""
    raw = fc.zigzag()
    cnt, got = _run(hip, raw)
    want = pr.extract(raw, fc.N_SCANS)
    _assert_bit_identical_xyz(cnt, got, want)
    assert cnt.sharp == 12 and cnt.less_sharp == 60
    fc.check_zigzag_order(got)


# ------------------------------------------------------------------------------------------------ q_imu forms
@pytest.mark.parametrize("name", ["negated_yaw", "non_unit_acos", "scan_rotation"])
def test_q_imu_form_on_the_acos_arm(hip, name):
    """d < 0 (the sign flip), a non-unit q below 1 - epsilon, ScanRotation's product: the position gate; -q also gives the cloud of +q"""
    q, branch, _ = fc.q_imu_forms()[name]
    assert branch == "acos"
    raw = fc.orientation_scan("baseline")
    cnt, got = _run(hip, raw, q)
    _assert_within_the_gate(cnt, got, pr.extract(raw, fc.N_SCANS, q_imu=tuple(q)))
    _assert_selection_of_own_cut(cnt, got)
    if name == "negated_yaw":
        _assert_within_the_gate(cnt, got, _want_orientation("baseline", fc.YAW))


def test_q_imu_non_unit_on_the_linear_arm_is_bit_identical(hip):
    """w = 1 with a non-zero vector part: slerp is (1 - t) + t q, then products and sums in double -- bit-identical GIVEN the ratio t, which comes from
    the intensity, which comes from atan2f.  On the two axis rows atan2f is exact on both sides (0 and -pi/2), t is 0 and about 0.2, and every bit of
    every output must agree.  On the noisy baseline the device's atan2f and glibc's differ by an ulp on some points (measured on the MI355X: the
    intensity differs in its last bit on 44 of 4673 points, the position on 18 of those and on no other): every point whose intensity has the same bits
    must have the same xyz bits, and all of them lie within the position gate"""
    q, branch, _ = fc.q_imu_forms()["non_unit_linear"]
    assert branch == "linear"
    raw = fc.axis_rows()
    cnt, got = _run(hip, raw, q)
    want = pr.extract(raw, fc.N_SCANS, q_imu=tuple(q))
    _assert_all_bits(cnt, got, want)
    moved = np.linalg.norm(got["cut"][:, :3].astype(np.float64) - pr.extract(raw, fc.N_SCANS)["cut"][:, :3], axis=1)
    assert (moved > 1e-3).sum() == fc.AXIS_ROW, "the second row is rotated"
    raw = fc.orientation_scan("baseline")
    cnt, got = _run(hip, raw, q)
    want = pr.extract(raw, fc.N_SCANS, q_imu=tuple(q))
    _assert_within_the_gate(cnt, got, want)
    same_t = (fc._bits(got["cut"][:, 3]) == fc._bits(want["cut"][:, 3]))
    same_xyz = (fc._bits(got["cut"][:, :3]) == fc._bits(want["cut"][:, :3])).all(1)
    print(f"linear arm on the baseline: {int((~same_t).sum())} of {len(same_t)} intensities differ in a bit, {int((~same_xyz).sum())} positions do, "
          f"{int((~same_xyz & same_t).sum())} of them at an equal intensity")
    assert same_t.sum() > 0.9 * len(same_t) and same_xyz[same_t].all()
    _assert_selection_of_own_cut(cnt, got)


# ------------------------------------------------------------------------------------------------ no stale state
def test_a_small_scan_after_a_large_one_equals_a_fresh_context(hip):
    """60 000 points in one ring leave every buffer, the global sort keys and the per-ring counts full; the rings of 11, 16 and 17 points after it
    must come out as from a fresh context, counts included"""
    big, small = fc.one_ring_60000(), fc.small_rings()
    ctx = _context(hip, fc.N_SCANS, len(big), ds_leaf=fc.HAND_LEAF)
    c0 = ctx.features_extract(big, IDENTITY)
    assert c0.cut == len(big) and c0.surf > 10000
    cnt = ctx.features_extract(small, IDENTITY)
    got = {name: ctx.features_read(which) for name, which in ALL}
    ctx.close()
    fresh_cnt, fresh = _run(hip, small, ds_leaf=fc.HAND_LEAF)
    assert cnt.as_dict() == fresh_cnt.as_dict()
    for name, _ in ALL:
        assert _same(got[name], fresh[name]), name
    _assert_all_bits(cnt, got, pr.extract(small, fc.N_SCANS, ds_leaf=fc.HAND_LEAF))
    assert (cnt.cut, cnt.flat, cnt.surf) == (44, 1, 6)


def test_a_reconfigured_context_equals_a_fresh_one(hip):
    """glio_features_config again on the same context, 64 lines -> 16 and ds_rate 1 -> 2: nothing of the first configuration survives"""
    from glio_amd import synth_lidar as sl
    raw64 = sl.make_scan(64, fc.N_AZ, seed=fc.SEED)
    raw = fc.orientation_scan("baseline")
    ctx = _context(hip, 64, len(raw64))
    c0 = ctx.features_extract(raw64, IDENTITY)
    assert c0.cut > 3 * len(raw) // 2 and len(np.unique(np.rint(ctx.features_read(T.FEAT_SURF)[:, 3]))) > 16
    ctx.features_config(fc.device_opts(fc.N_SCANS, len(raw), ds_rate=2))
    cnt = ctx.features_extract(raw, IDENTITY)
    got = {name: ctx.features_read(which) for name, which in ALL}
    ctx.close()
    fresh_cnt, fresh = _run(hip, raw, ds_rate=2)
    assert cnt.as_dict() == fresh_cnt.as_dict()
    for name, _ in ALL:
        assert _same(got[name], fresh[name]), name
    _assert_selection_of_own_cut(cnt, got, ds_rate=2)
    _assert_bit_identical_xyz(cnt, got, pr.extract(raw, fc.N_SCANS, ds_rate=2))

"""GPU: the GNSS frame estimate (glio_align_*, csrc/align_kernels.hip) against its numpy restatement (tests/gnss_align_restated.py) on the cases of
tests/test_gnss_align_restated.py, against the existing single-factor evaluator and the batch stage (one definition of the DD row), on ragged factor sets,
on unobservable inputs, and its bits and refusals.

THE GATE is the project's: max(1e-9, 100 x the case's floor) relative to max(1, |value|); the floor is the restatement against itself with every input one
ulp up (2e-10 .. 3.3e-9 on these cases); the integer outputs are exact."""
import ctypes as C
import math

import numpy as np
import pytest

import gnss_align_restated as R

pytestmark = pytest.mark.gpu
CASE_IDS = [f"{s}-{o}" for s, o in R.CASES]


def _frame(psi, anc):
    from glio_amd import align
    return align.frame_of(psi, anc)


def device_result(al, res, start_anc, coarse=True):
    """an AlignResult in the restatement's form"""
    i = res.info
    return dict(status=i["status"], winner=i["winner"], n_rows=i["n_rows"], rounds=i["rounds"], coarse=al.read_coarse() if coarse and al.n_hypotheses > 0 else np.zeros(0),
                coarse_cost=i["coarse_cost"], runner_up_cost=i["runner_up_cost"], psi=res.yaw, anc=res.anchor, yaw_sigma=i["yaw_sigma"], covariance=i["covariance"],
                start_anc=np.asarray(start_anc, float))


class Device:
    """one glio_align per case, its factors and positions uploaded once"""

    def __init__(self, case):
        from glio_amd import align
        self.case = case
        self.al = align.GnssAlignment(len(case["dd"]), len(case["P"]))
        self.al.set_factors(case["dd"])
        self.al.set_positions(case["P"])

    def solve(self, H=R.H_DEFAULT, start_psi=None, **kw):
        c = self.case
        self.al.set_opts(n_hypotheses=H, **kw)
        psi0 = (c["true_psi"] + 0.05 if H == 0 else c["start_psi"]) if start_psi is None else start_psi
        return device_result(self.al, self.al.solve(_frame(psi0, c["start_anc"])), c["start_anc"])


_devices = {}


def device_of(case):
    if case["name"] not in _devices:
        _devices[case["name"]] = Device(case)
    return _devices[case["name"]]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for d in _devices.values():
        d.al.close()
    _devices.clear()


@pytest.fixture(scope="module", params=R.CASES, ids=CASE_IDS)
def case(request):
    return R.make_case(*request.param)


# ------------------------------------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("H", [72, 0, 1, 7, 360])
def test_parity_with_the_restatement(case, H):
    """all H coarse costs, the winner, every round's iterations / cost / down-weighted count, the yaw, the anchor (ENU, metres), sigma_psi, the covariance"""
    want = R.restate(case, H)
    floor = R.floor_of(case, H)
    assert floor <= 1e-7
    got = device_of(case).solve(H)
    dev = R.deviation(got, want)
    print(f"{case['name']} H = {H}: floor {floor:.2e}, gate {R.gate_of(floor):.2e}, deviation {dev:.2e}, rounds {got['rounds']}")
    R.compare(got, want, R.gate_of(floor), case["name"])
    assert (got["status"], got["winner"], got["n_rows"]) == (want["status"], want["winner"], want["n_rows"])
    assert [(r[0], r[2]) for r in got["rounds"]] == [(r[0], r[2]) for r in want["rounds"]]
    assert -math.pi < got["psi"] <= math.pi


# ------------------------------------------------------------------------------------------------ one definition
@pytest.fixture(scope="module")
def eval_ctx():
    from glio_amd import capi, synth
    ctx = capi.Context(synth.default_opts(W=2, pts=1024, map_pts=1 << 12))
    yield ctx
    ctx.close() if hasattr(ctx, "close") else None


def evaluator_cost(ctx, case, psi, anc, threshold):
    """the sum over the factors of glio_eval_dd_psr's residuals (capi.hip's host rotation, k_eval_dd)"""
    total, P = 0.0, case["P"]
    for f in case["dd"]:
        f.threshold = threshold
        r, _ = ctx.eval_dd_psr(f, P[f.slot_i], P[f.slot_j], psi, anc)
        total += 0.5 * float(r @ r)
    return total


@pytest.mark.parametrize("scene_offset", [R.CASES[0], R.CASES[1]], ids=CASE_IDS[:2])
def test_cost_is_the_existing_evaluators(eval_ctx, scene_offset):
    """glio_align_cost at the start frame and at the estimate, thresholds 1e9 and 6: the new kernels and the device ecef2rotation tied to glio_eval_dd_psr
    and the host rotation"""
    c = R.make_case(*scene_offset)
    d = device_of(c)
    est = d.solve()
    gate = R.gate_of(R.floor_of(c))
    for psi, anc in ((c["start_psi"], c["start_anc"]), (est["psi"], est["anc"])):
        for thr in (1e9, 6.0):
            got, nd = d.al.cost(_frame(psi, anc), thr)
            want = evaluator_cost(eval_ctx, c, psi, anc, thr)
            rc, rn = R.cost(c["fs"], c["P"], psi, anc, thr)
            print(f"{c['name']} threshold {thr:g}: cost {got!r}, evaluator {want!r}, restated {rc!r}, down-weighted {nd}")
            assert abs(got - want) <= gate * max(1.0, abs(want))
            assert abs(got - rc) <= gate * max(1.0, abs(rc)) and nd == rn


def test_the_frame_goes_into_the_batch_stage_unchanged():
    """BatchStage.set_small_factors takes the frame, and its DD cost at these positions is glio_align_cost's"""
    from glio_amd import batch
    c = R.make_case("K24", "near")
    d = device_of(c)
    d.al.set_opts(n_hypotheses=R.H_DEFAULT)
    res = d.al.solve(_frame(c["start_psi"], c["start_anc"]))
    K, band = c["K"], 6
    gt = batch.make_poses(K)[0]
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 20, band)
    st = batch.BatchStage(K, band, len(ci))
    st.set_constraints(ci, cj, cp.numpy(), nc.numpy(), score.numpy())
    st.set_small_factors(dd=c["dd"], frame=res.frame, threshold=6.0)
    poses = np.zeros((K, 7)); poses[:, :3] = c["P"]; poses[:, 3] = 1.0
    Hg = st.new_hg()
    st.add_small(poses, Hg)
    stage_cost = float(Hg[-1].item())
    st.close()
    got, _ = d.al.cost(res.frame, 6.0)
    print(f"batch stage DD cost {stage_cost!r}, glio_align_cost {got!r}")
    assert abs(got - stage_cost) <= R.gate_of(R.floor_of(c)) * max(1.0, abs(stage_cost))


# ------------------------------------------------------------------------------------------------ ragged shapes
def ragged_case(total_rows):
    """factors of 1 .. 19 rows (n_sat 2 .. 20) cut from 20-satellite factors: master first and last, a non-identity lower-triangular W, `total_rows` rows"""
    from glio_amd import batch, synth
    from glio_amd import ctypes_types as T
    K = 24
    gt = batch.make_poses(K)[0]
    full, _ = batch.make_batch_gnss(gt, sats_per_sys=20)
    sizes, dd, rows, k = [2, 20, 7, 11, 3, 20, 5], [], 0, 0
    while rows < total_rows:
        ns = min(sizes[k % len(sizes)], total_rows - rows + 1)
        src = full[k % len(full)]
        f = T.GlioDdPsr()
        f.slot_i, f.slot_j, f.n_sat, f.ratio, f.threshold = src.slot_i, src.slot_j, ns, src.ratio, 1e9
        f.master = 0 if k % 2 == 0 else ns - 1
        f.station[:] = src.station[:]
        for i in range(ns):
            f.user_sat_pos[i][:] = src.user_sat_pos[i][:]; f.ref_sat_pos[i][:] = src.ref_sat_pos[i][:]
            f.user_psr[i], f.ref_psr[i] = src.user_psr[i], src.ref_psr[i]
        W = np.tril(0.15 * np.cos(1.0 + np.arange((ns - 1) ** 2).reshape(ns - 1, ns - 1) + k)) + np.eye(ns - 1)
        f.weight[:W.size] = list(W.ravel())
        dd.append(f); rows += ns - 1; k += 1
    shift, psi = np.array([35.0, -20.0, 4.0]), 2.1
    A = np.array(synth.ANCHOR_ECEF, float)
    fac = [R.factor_dict(f) for f in dd]
    c = dict(name=f"ragged-{total_rows}", dd=dd, factors=fac, fs=R.Factors(fac), P=np.ascontiguousarray((gt[:, :3] - shift) @ R.rz(psi)), true_psi=psi,
             true_anc=A + R.ecef2rotation(A) @ shift, start_psi=0.0, start_anc=A.copy(), K=K)
    assert c["fs"].n_rows == total_rows
    return c


@pytest.mark.parametrize("total_rows", [255, 256, 257, 601])
def test_ragged_factor_sets(total_rows):
    """one workgroup's share of rows (256) and one less and one more, a count that is no multiple of 64, one-row and 19-row factors side by side"""
    c = ragged_case(total_rows)
    assert {f.n_sat for f in c["dd"]} >= {2, 20} and {f.master for f in c["dd"]} >= {0, 19}
    d = Device(c)
    try:
        for thr in (1e9, 6.0):
            got, nd = d.al.cost(_frame(c["true_psi"], c["true_anc"]), thr)
            want, wn = R.cost(c["fs"], c["P"], c["true_psi"], c["true_anc"], thr)
            assert abs(got - want) <= 1e-9 * max(1.0, want) and nd == wn, (thr, got, want, nd, wn)
        want = R.restate(c, 36)
        floor = R.floor_of(c, 36)
        assert floor <= 1e-7 and want["min_margin"] >= 1e-6
        got = d.solve(36)
        print(f"{c['name']}: floor {floor:.2e}, deviation {R.deviation(got, want):.2e}, rounds {got['rounds']}")
        R.compare(got, want, R.gate_of(floor), c["name"])
    finally:
        d.al.close()


# ------------------------------------------------------------------------------------------------ observability
def _bits(frame):
    return bytes(frame)


def test_standing_still_is_unobservable():
    from glio_amd import align
    c = R.make_case("K24", "near")
    al = align.GnssAlignment(len(c["dd"]), len(c["P"]))
    al.set_factors(c["dd"])
    al.set_positions(np.tile(c["P"][:1], (len(c["P"]), 1)))
    start = _frame(0.3, c["start_anc"])
    res = al.solve(start)
    assert res.status == align.UNOBSERVABLE and not res.delivered and _bits(res.frame) == _bits(start)
    assert res.info["yaw_sigma"] == 0.0 and not res.info["yaw_schur"] > 1e-9 * res.info["h_yaw_yaw"] and not res.info["covariance"].any()
    al.set_factors(c["dd"][:1])                           # one factor only: every row shares one position
    al.set_positions(c["P"])
    res = al.solve(start)
    assert res.status == align.UNOBSERVABLE and _bits(res.frame) == _bits(start)
    al.close()


@pytest.mark.parametrize("offset", list(R.OFFSETS))
def test_max_yaw_sigma_turns_a_result_weak(offset):
    """K = 24: sigma_psi is 0.016"""
    from glio_amd import align
    d = device_of(R.make_case("K24", offset))
    fine, weak = d.solve(max_yaw_sigma=0.05), d.solve(max_yaw_sigma=0.01)
    assert fine["status"] == align.OK and weak["status"] == align.WEAK and 0.01 < fine["yaw_sigma"] < 0.05
    assert weak["psi"] == fine["psi"] and np.array_equal(weak["anc"], fine["anc"])          # delivered, the same bits
    d.al.set_opts()


# ------------------------------------------------------------------------------------------------ bits and refusals
def test_two_solves_and_a_solve_after_a_refusal_give_equal_bytes():
    from glio_amd import capi
    from glio_amd import ctypes_types as T
    c = R.make_case("K120", "wrap_1km")
    d = device_of(c)
    d.al.set_opts()
    start = _frame(c["start_psi"], c["start_anc"])

    def run():
        out, info = T.GlioGnssFrame(), T.GlioAlignInfo()
        capi._check(capi.load().glio_align_solve(d.al._h, C.byref(start), C.byref(out), C.byref(info)))
        return bytes(out) + bytes(info) + d.al.read_coarse().tobytes()

    a, b = run(), run()
    assert a == b
    bad = _frame(math.nan, c["start_anc"])
    out = _frame(7.0, [1.0, 2.0, 3.0])
    before = bytes(out)
    assert capi.load().glio_align_solve(d.al._h, C.byref(bad), C.byref(out), None) == capi.E_ARG and bytes(out) == before
    with pytest.raises(capi.GlioError):
        d.al.set_opts(thresholds=[1.0] * 9)
    d.al.cost(start, 6.0)                                  # a cost query between solves changes nothing either
    assert run() == a


def test_refusals():
    from glio_amd import align, capi
    from glio_amd import ctypes_types as T
    lib = capi.load()
    c = R.make_case("K24", "near")
    h = C.c_void_p()
    for args in ((0, 0, 10), (0, 10, 0), (0, -1, 10), (99, 10, 10)):
        assert lib.glio_align_create(*args, C.byref(h)) == capi.E_ARG, args
    assert lib.glio_align_create(0, 10, 10, None) == capi.E_ARG
    al = align.GnssAlignment(4, 5)
    start, out = _frame(0.0, c["start_anc"]), _frame(7.0, [1.0, 2.0, 3.0])
    before = bytes(out)
    refused = lambda rc: rc == capi.E_ARG and bytes(out) == before
    arr = lambda fs: (T.GlioDdPsr * len(fs))(*fs)

    def variant(**kw):
        f = T.GlioDdPsr.from_buffer_copy(bytes(c["dd"][0]))
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    assert refused(lib.glio_align_solve(al._h, C.byref(start), C.byref(out), None))                        # no factors
    assert lib.glio_align_set_factors(al._h, 0, arr([variant()])) == capi.E_ARG                            # no factors
    assert lib.glio_align_set_factors(al._h, 5, arr([variant()] * 5)) == capi.E_ARG                        # capacity
    assert lib.glio_align_set_factors(al._h, 1, None) == capi.E_ARG
    for kw in (dict(slot_i=5), dict(slot_j=-1), dict(n_sat=1), dict(n_sat=21), dict(master=-1), dict(master=6)):
        assert lib.glio_align_set_factors(al._h, 1, arr([variant(**kw)])) == capi.E_ARG, kw
    assert refused(lib.glio_align_solve(al._h, C.byref(start), C.byref(out), None))                        # still none
    al.set_factors([variant(slot_i=3, slot_j=4)])
    assert refused(lib.glio_align_solve(al._h, C.byref(start), C.byref(out), None))                        # no positions
    P = np.ascontiguousarray(c["P"][:5])
    assert lib.glio_align_set_positions(al._h, 6, T.dptr(P), 3) == capi.E_ARG                              # capacity
    assert lib.glio_align_set_positions(al._h, 0, T.dptr(P), 3) == capi.E_ARG
    assert lib.glio_align_set_positions(al._h, 5, T.dptr(P), 2) == capi.E_ARG
    assert lib.glio_align_set_positions(al._h, 5, None, 3) == capi.E_ARG
    al.set_positions(P[:4])
    assert refused(lib.glio_align_solve(al._h, C.byref(start), C.byref(out), None))                        # slot 4 of a table of 4
    cost = C.c_double(-1.0)
    assert lib.glio_align_cost(al._h, C.byref(start), C.c_double(6.0), C.byref(cost), None) == capi.E_ARG and cost.value == -1.0
    al.set_positions(P)
    assert refused(lib.glio_align_solve(al._h, None, C.byref(out), None))
    assert lib.glio_align_solve(al._h, C.byref(start), None, None) == capi.E_ARG
    assert lib.glio_align_cost(al._h, C.byref(start), C.c_double(0.0), C.byref(cost), None) == capi.E_ARG
    assert lib.glio_align_cost(al._h, C.byref(start), C.c_double(6.0), None, None) == capi.E_ARG
    for kw in (dict(thresholds=[1.0] * 9), dict(n_rounds=0), dict(n_hypotheses=-1), dict(n_hypotheses=4097), dict(max_iterations_per_round=0),
               dict(max_iterations_per_round=65), dict(thresholds=[1e9, 0.0]), dict(thresholds=[math.nan]), dict(yaw_tolerance=-1.0), dict(pos_tolerance=math.inf),
               dict(max_yaw_sigma=math.nan)):
        o = capi.align_opts(**kw)
        assert lib.glio_align_set_opts(al._h, C.byref(o)) == capi.E_ARG, kw
    assert lib.glio_align_set_opts(al._h, None) == capi.E_ARG
    assert lib.glio_align_read_coarse(al._h, T.dptr(np.zeros(72)), 72, None) == capi.E_STATE               # no solve yet
    ms = C.c_float()
    assert lib.glio_align_last_device_ms(al._h, C.byref(ms)) == capi.E_STATE
    res = al.solve(start)                                  # and after all of it the object works: one factor is unobservable
    assert res.status == align.UNOBSERVABLE and bytes(res.frame) == bytes(start)
    few = np.full(72, -1.0)
    assert lib.glio_align_read_coarse(al._h, T.dptr(few), 71, None) == capi.E_ARG and (few == -1.0).all()   # room for fewer than the search had
    assert lib.glio_align_read_coarse(al._h, None, 0, None) == capi.E_ARG and len(al.read_coarse()) == 72
    assert al.last_device_ms() > 0
    al.close()


def test_a_pose_table_is_passed_as_it_lies():
    c = R.make_case("K24", "near")
    d = device_of(c)
    want = d.al.cost(_frame(c["true_psi"], c["true_anc"]), 6.0)
    poses = np.zeros((len(c["P"]), 7)); poses[:, :3] = c["P"]; poses[:, 3:] = 9.0
    d.al.set_positions(poses)
    assert d.al._pos.strides[0] == 56 and d.al.cost(_frame(c["true_psi"], c["true_anc"]), 6.0) == want
    d.al.set_positions(c["P"])

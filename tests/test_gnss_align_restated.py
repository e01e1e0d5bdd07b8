"""CPU: the numpy restatement of the GNSS frame estimate (tests/gnss_align_restated.py) held to what makes it a reference for the kernels -- its Jacobian
against finite differences, the truth of the scenes, the cases' distance from every knife edge, and the deliberately wrong variants refused by the same
comparison the device goes through.

Figures of the restatement on these cases (H = 72, start: yaw 0 at the scene's anchor), re-derived here:
    case            winner        yaw error (in sigma_psi)   mapped error   C(estimate; 6)   C(truth; 6)    lead         least |raw| - threshold
    K24-near        24 (120 deg)  0.01238 rad (0.78)         0.411 m        252.158          255.586        6.0e-5       0.890 m
    K24-wrap_1km    37 (185 deg)  0.01242 rad (0.78)         0.420 m        252.163          255.535        2.6e-3       0.890 m
    K120-near       24 (120 deg)  0.00191 rad (1.63)         0.227 m        2281.267         2286.994       4.7e-2       0.353 m
    K120-wrap_1km   38 (190 deg)  0.00188 rad (1.60)         0.156 m        2281.329         2283.507       4.9e-2       0.307 m
s / H_psipsi is 5.7e-2 / 7.9e-5 (K24) and 0.56 / 1.3e-3 (K120): with the local origin 1 km from the drive the anchor moves by sigma_psi x 1 km, so the
anchor alone is never compared."""
import math

import numpy as np
import pytest

import gnss_align_restated as R

CASE_IDS = [f"{s}-{o}" for s, o in R.CASES]


@pytest.fixture(scope="module", params=R.CASES, ids=CASE_IDS)
def case(request):
    return R.make_case(*request.param)


def lower_w_case():
    """K24-near with a non-identity lower-triangular W on every factor: the whitening couples a factor's rows"""
    base = R.make_case("K24", "near")
    fac = []
    for k, f in enumerate(base["factors"]):
        n = f["n_sat"] - 1
        W = np.tril(0.15 * np.cos(1.0 + np.arange(n * n).reshape(n, n) + k)) + np.eye(n)
        fac.append(dict(f, weight=W))
    return dict(base, name="K24-near-lowerW", factors=fac, fs=R.Factors(fac))


# ------------------------------------------------------------------------------------------------ (1) the Jacobian
def jacobian_check(c, psi, anc, threshold):
    """Central differences in (d_e, d_n, d_u, d_psi) with the rotation frozen at the anchor.  The rows are differences of ranges of 2.6e7 m, so a residual
    carries ~4e-9 m of rounding: the quotient is off by up to 2e-8 / h, the yaw's also by the truncation |lp| h^2.  Steps of 1e-2 m and 3e-4 rad, cut down
    where a quarter of the distance of the nearest raw row from the threshold is less (no weight may flip inside the difference); x 3 for a W that sums
    rows.  The bound comes to 1e-6 .. 1e-4 of a column's scale."""
    fs, P = c["fs"], c["P"]
    Ree = R.ecef2rotation(anc)
    _, J, _, margin = R.rows(fs, P, psi, anc, Ree, threshold)
    extent = float(np.sqrt((P ** 2).sum(1)).max())
    for k in range(4):
        lever = extent if k == 3 else 1.0
        h = min(3e-4 if k == 3 else 1e-2, 0.25 * margin / lever)
        d = np.zeros(4); d[k] = h
        rp = R.rows(fs, P, psi + d[3], anc + Ree @ d[:3], Ree, threshold)[0]
        rm = R.rows(fs, P, psi - d[3], anc - Ree @ d[:3], Ree, threshold)[0]
        err = np.abs((rp - rm) / (2 * h) - J[:, k]).max()
        tol = 3.0 * (2e-8 / h + (extent * h * h if k == 3 else 1e-9))
        assert tol <= 1e-4 * max(1.0, np.abs(J[:, k]).max()), (k, h, tol)           # far below a wrong sign or a missing rotation (order 1)
        assert err <= tol, (k, h, err, tol, np.abs(J[:, k]).max())


@pytest.mark.parametrize("threshold", [1e9, 6.0])
def test_jacobian_against_central_differences(case, threshold):
    r = R.restate(case)                                    # at the estimate: the nearest raw row is 0.3 m from the threshold there
    jacobian_check(case, r["psi"], r["anc"], threshold)


def test_jacobian_through_a_coupling_whitening():
    c = lower_w_case()
    jacobian_check(c, c["true_psi"], c["true_anc"], 6.0)


# ------------------------------------------------------------------------------------------------ (2) the truth of the scene
def test_the_estimate_against_the_truth(case):
    r = R.restate(case)
    assert r["status"] == R.OK and r["n_rows"] == case["fs"].n_rows
    won = (2.0 * math.pi * r["winner"]) / R.H_DEFAULT
    assert abs(R.wrap(won - case["true_psi"])) <= math.radians(5.0)
    yaw_err = abs(R.wrap(r["psi"] - case["true_psi"]))
    sig = np.sqrt(np.diag(r["covariance"]))
    assert sig[3] == pytest.approx(r["yaw_sigma"], rel=1e-9)
    assert yaw_err <= 4.0 * r["yaw_sigma"], (yaw_err, r["yaw_sigma"])
    extent = float(np.sqrt((case["P"][:, :2] ** 2).sum(1)).max())
    bound = 4.0 * math.sqrt(sig[0] ** 2 + sig[1] ** 2 + sig[2] ** 2 + (r["yaw_sigma"] * extent) ** 2)
    mapped = R.mapped_error(case, r["psi"], r["anc"])
    assert mapped <= bound, (mapped, bound)
    c_est, c_true = R.cost(case["fs"], case["P"], r["psi"], r["anc"], 6.0)[0], R.cost(case["fs"], case["P"], case["true_psi"], case["true_anc"], 6.0)[0]
    print(f"{case['name']}: winner {r['winner']}, yaw error {yaw_err:.5f} rad = {yaw_err / r['yaw_sigma']:.2f} sigma, mapped {mapped:.3f} m (bound {bound:.2f}), "
          f"C(estimate) {c_est:.3f}, C(truth) {c_true:.3f}, rounds {r['rounds']}")
    assert c_est <= c_true
    assert -math.pi < r["psi"] <= math.pi


def test_the_figures_of_the_docstring():
    want = {"K24-near": (24, 252.158, 255.586), "K24-wrap_1km": (37, 252.163, 255.535), "K120-near": (24, 2281.267, 2286.994), "K120-wrap_1km": (38, 2281.329, 2283.507)}
    for s, o in R.CASES:
        c = R.make_case(s, o)
        r = R.restate(c)
        w, ce, ct = want[c["name"]]
        assert r["winner"] == w
        assert R.cost(c["fs"], c["P"], r["psi"], r["anc"], 6.0)[0] == pytest.approx(ce, abs=2e-3)
        assert R.cost(c["fs"], c["P"], c["true_psi"], c["true_anc"], 6.0)[0] == pytest.approx(ct, abs=2e-3)


# ------------------------------------------------------------------------------------------------ (3) knife edges
@pytest.mark.parametrize("H", [72, 0, 1, 7, 360])
def test_no_case_stands_on_a_knife_edge(case, H):
    """the winner leads by >= 1e-6 relative, no raw row within 1e-6 m of a threshold at any linearisation, and one ulp on every input changes no decision
    and moves no output by more than 1e-7"""
    r = R.restate(case, H)
    if H > 1:
        srt = np.sort(r["coarse"])
        assert (srt[1] - srt[0]) >= 1e-6 * srt[0], (srt[0], srt[1])
        assert r["runner_up_cost"] == srt[1] and r["coarse_cost"] == srt[0]
    assert r["min_margin"] >= 1e-6, r["min_margin"]
    floor = R.floor_of(case, H)
    print(f"{case['name']} H = {H}: floor {floor:.2e}, iterations {[x[0] for x in r['rounds']]}")
    assert floor <= 1e-7


# ------------------------------------------------------------------------------------------------ (4) wrong restatements
@pytest.mark.parametrize("wrong", ["yaw_sign", "enu_unrotated"])
def test_a_wrong_derivative_is_refused(case, wrong):
    right = R.restate(case)
    bad = R.solve(case["fs"], case["P"], case["start_psi"], case["start_anc"], H=R.H_DEFAULT, wrong=wrong)
    with pytest.raises(AssertionError):
        R.compare(bad, right, R.gate_of(R.floor_of(case)), wrong)


def test_the_threshold_after_the_whitening_is_refused():
    """needs a W that couples rows: with W = I the two orders are the same arithmetic"""
    c = lower_w_case()
    right = R.restate(c)
    assert right["status"] == R.OK and right["min_margin"] >= 1e-6 and sum(x[2] for x in right["rounds"]) > 0
    gate = R.gate_of(R.floor_of(c))
    assert gate <= 1e-5
    bad = R.solve(c["fs"], c["P"], c["start_psi"], c["start_anc"], H=R.H_DEFAULT, wrong="threshold_after_whitening")
    with pytest.raises(AssertionError):
        R.compare(bad, right, gate)
    same = R.solve(c["fs"], c["P"], c["start_psi"], c["start_anc"], H=R.H_DEFAULT)
    assert R.compare(same, right, gate) == 0.0


def test_the_tie_taking_the_highest_hypothesis_is_refused():
    """No case of the list ties (test_no_case_stands_on_a_knife_edge), and costs of a real scene tie only up to rounding, so the rule is held where a tie is
    exact: a cost list with two equal minima.  The comparison refuses the other winner."""
    costs = np.array([5.0, 3.0, 4.0, 3.0, 9.0])
    assert R.pick(costs) == (1, 3.0, 3.0) and R.pick(costs, tie_highest=True)[0] == 3
    assert R.pick([math.inf, math.inf])[0] == -1 and R.pick([2.0]) == (0, 2.0, math.inf)
    c = R.make_case("K24", "near")
    right = R.restate(c, 2)                                # H = 2: the costs of 0 and pi
    tied = dict(right, coarse=np.array([right["coarse"].min()] * 2))
    lo, hi = R.pick(tied["coarse"])[0], R.pick(tied["coarse"], tie_highest=True)[0]
    assert (lo, hi) == (0, 1)
    with pytest.raises(AssertionError):
        R.compare(dict(right, winner=hi if right["winner"] == lo else lo), right, 1e-9)


def test_a_rotation_that_is_not_recomputed_is_refused_on_the_1km_case():
    for scene in R.SCENES:
        c = R.make_case(scene, "wrap_1km")
        right = R.restate(c)
        bad = R.solve(c["fs"], c["P"], c["start_psi"], c["start_anc"], H=R.H_DEFAULT, wrong="rotation_not_recomputed")
        with pytest.raises(AssertionError):
            R.compare(bad, right, R.gate_of(R.floor_of(c)))


# ------------------------------------------------------------------------------------------------ observability
def test_standing_still_and_one_factor_are_unobservable():
    c = R.make_case("K24", "near")
    still = R.solve(c["fs"], np.tile(c["P"][:1], (len(c["P"]), 1)), 0.3, c["start_anc"], H=8)
    assert still["status"] == R.UNOBSERVABLE and still["psi"] == 0.3 and np.array_equal(still["anc"], c["start_anc"])
    assert 0 <= still["yaw_schur"] <= 1e-9 * still["h_yaw_yaw"] or not still["yaw_schur"] > 0
    one = R.solve(R.Factors(c["factors"][:1]), c["P"], 0.3, c["start_anc"], H=8)
    assert one["status"] == R.UNOBSERVABLE and one["psi"] == 0.3
    weak = R.restate(c, max_yaw_sigma=0.01)
    fine = R.restate(c, max_yaw_sigma=0.05)
    assert weak["status"] == R.WEAK and fine["status"] == R.OK and weak["psi"] == fine["psi"] and 0.01 < fine["yaw_sigma"] < 0.05

"""CPU: the numpy restatement of the every-frame trajectory (tests/trajectory_restated.py) held to the reference's own functor, to central differences and
to known answers, and the shared case builder's margins; the branch cases (what they reach, their margins and one-ulp condition) and the proof that the
comparison the GPU tests use refuses deliberately wrong solvers on them."""
import numpy as np
import pytest

import np_ceres
import trajectory_restated as tr
from glio_amd import trajectory
from oracle import pyref


def _pose(rng, scale=1.0):
    q = rng.normal(size=4)
    return np.concatenate([scale * rng.normal(size=3), q / np.linalg.norm(q) * (1.0 + 0.05 * rng.normal())])          # not exactly unit: the Jets see |q|


@pytest.mark.skipif(not pyref.available(), reason="the reference's factor layer is not on this machine")
def test_factor_against_the_reference_functor():
    """LidarPoseFactorBatchRelativeAutoDiff rows / 10 resp. / 20 and * 0.2 are LidarPoseFactorAutoDiff's (same functor, other weights): 1e-12 relative"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        pa, pb, mq = _pose(rng), _pose(rng), _pose(rng)
        m = np.concatenate([mq[3:7], rng.normal(size=3)])
        r_ref, J_ref = pyref.eval_relative_pose(m[0:4], m[4:7], pa[0:3], pa[3:7], pb[0:3], pb[3:7])
        w = np.array([10.0, 10.0, 10.0, 20.0, 20.0, 20.0])
        r, Jp1, Jq1, Jp2, Jq2 = tr.factor_global(m, pa, pb)
        for got, ref in ((r, r_ref), (Jp1, J_ref[0]), (Jq1, J_ref[1]), (Jp2, J_ref[2]), (Jq2, J_ref[3])):
            want = (ref.T / w * 0.2).T
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_analytic_jacobians_against_central_differences():
    rng = np.random.default_rng(4)
    for _ in range(5):
        pa, pb, mq = _pose(rng), _pose(rng), _pose(rng)
        m = np.concatenate([mq[3:7], rng.normal(size=3)])
        r, Ja, Jb = tr.factor_local(m, pa, pb)
        h = 1e-6
        for which, J in ((0, Ja), (1, Jb)):
            for c in range(6):
                d = np.zeros(6); d[c] = h
                def moved(s):
                    x = [pa.copy(), pb.copy()]
                    x[which] = np.concatenate([x[which][0:3] + s * d[0:3], tr.quat_plus(x[which][3:7], s * d[3:6])])
                    return tr.factor_residual(m, x[0], x[1])
                num = (moved(1.0) - moved(-1.0)) / (2 * h)
                assert np.abs(num - J[:, c]).max() < 1e-7 * max(1.0, np.abs(J).max())


def _consistent_chain(rng, N):
    """anchors and poses that satisfy every factor exactly as the reference wires them: between factor i -> i + 1 takes measurement i"""
    left = _pose(rng); left[3:7] /= np.linalg.norm(left[3:7])
    meas = []
    for i in range(N + 1):
        q = rng.normal(size=4); q[0] += 4.0
        meas.append(np.concatenate([q / np.linalg.norm(q), 0.3 * rng.normal(size=3)]))
    meas = np.array(meas)
    x = tr.resolve_init(meas, left, N)
    right = tr.compose(x[-1], meas[N])
    return meas, left, right, x


def test_a_consistent_chain_ends_at_once():
    rng = np.random.default_rng(5)
    meas, left, right, x = _consistent_chain(rng, 4)
    sol, summ, _ = tr.local_graph(meas, left, right, x)
    assert summ["termination"] == np_ceres.GRADIENT_TOL and summ["iterations"] == 0 and np.array_equal(sol, x)


def test_no_frame_changes_nothing_and_one_frame_has_no_between_factor():
    rng = np.random.default_rng(6)
    meas, left, right, x = _consistent_chain(rng, 1)
    sol, summ, _ = tr.local_graph(meas, left, right, np.zeros((0, 7)))
    assert summ["termination"] == tr.NOT_SOLVED and summ["iterations"] == 0 and sol.shape == (0, 7)
    assert tr.factor_list(1) == [(-1, 0, 0), (0, -1, 1)]
    assert tr.factor_list(3) == [(-1, 0, 0), (0, 1, 0), (1, 2, 1), (2, -1, 3)]          # measurement 0 twice, measurement 2 never (:3490-3491)


def test_right_anchor_translation_is_shared_by_weighted_least_squares():
    """All measurements the identity with dp = 0, every pose on the left anchor: the translation rows are R_k^T (x_{k+1} - x_k), whose norm no rotation
    changes, so the rotations stay put (their rows are zero) and the N + 1 equally weighted links minimise sum |x_{k+1} - x_k|^2 with x_{-1} = left,
    x_N = left + d: the misclosure spreads evenly, pose k (0-based) moves by (k + 1) / (N + 1) d.
    The bound: the problem is linear, so the first Gauss-Newton step would be exact but for Ceres' damping mu = 1e-8 on the (Jacobi-scaled) diagonal, and the
    loop then ends on the function tolerance.  (H + mu diag H) instead of H shortens the step by at most mu * max(diag) / lambda_min = mu * 2 / (2 - 2 cos(pi /
    (N + 1))) of its length (H is the -1, 2, -1 chain matrix), and no step is longer than |d|."""
    N = 4
    ident = np.array([1.0, 0, 0, 0])
    left = np.concatenate([[1.0, -2.0, 0.5], ident])
    step = np.zeros(3)
    meas = np.array([np.concatenate([ident, step])] * (N + 1))
    x = np.array([np.concatenate([left[0:3] + (k + 1) * step, ident]) for k in range(N)])
    d = np.array([0.3, -0.2, 0.1])
    right = np.concatenate([left[0:3] + (N + 1) * step + d, ident])
    sol, summ, _ = tr.local_graph(meas, left, right, x)
    bound = 1e-8 * 2.0 / (2.0 - 2.0 * np.cos(np.pi / (N + 1))) * np.abs(d).max()
    for k in range(N):
        assert np.abs(sol[k, 0:3] - (x[k, 0:3] + (k + 1) / (N + 1) * d)).max() < bound
        assert np.abs(sol[k, 3:7] - ident).max() < bound


def test_direct_reading_and_sample_rows_agree():
    """the reference's loop read straight off the IMU buffer == trajectory.frame_samples + the recurrence over its rows, bit for bit"""
    rng = np.random.default_rng(7)
    stamps = 100.0 + np.cumsum(rng.uniform(0.004, 0.006, 120))
    acc = np.array([0.0, 0.0, 9.8]) + rng.normal(0, 4.0, (120, 3))
    gyr = rng.normal(0, 0.3, (120, 3))
    fs = [stamps[3] + 0.001, stamps[20] + 0.002, stamps[41], stamps[41] + 0.0005, stamps[70] + 0.003]          # one on a sample, one segment with no whole sample
    P, V, R, g = rng.normal(size=3), rng.normal(size=3), tr.q2R_np(tr.rot_q([0.2, 0.1, 1.0], 0.7)), [0, 0, 9.805]
    rows, br, segs = tr.fill_in_direct(stamps, acc, gyr, fs, 3, P, V, R, g)
    offs, smp, _ = trajectory.frame_samples(stamps, acc, gyr, fs, 3)
    assert np.array_equal(np.concatenate(segs), smp) and list(offs) == list(np.cumsum([0] + [len(s) for s in segs]))
    rows2, br2 = tr.dead_reckon(offs, smp, P, V, R, g)
    assert np.array_equal(rows, rows2) and br == br2


def test_quaternion_from_matrix_branches():
    for axis, angle, want in (((0, 0, 1), 0.1, 0), ((1, 0, 0), 3.1, 1), ((0, 1, 0), 3.1, 2), ((0, 0, 1), 3.1, 3)):
        q, br = tr.quat_from_matrix(tr.q2R(tr.rot_q(axis, angle)))
        assert br == want
        ref = tr.rot_q(axis, angle)
        assert min(np.abs(q - ref).max(), np.abs(q + ref).max()) < 1e-12


def test_case_builder_margins_and_expected_ends():
    got = {name: res[3] for name, _, res in tr.cases()}
    s = got["nominal_3"]
    assert (s["termination"], s["iterations"], s["successful_steps"]) == (np_ceres.FUNCTION_TOL, 3, 2)
    s = got["far_anchor_3"]
    assert s["termination"] == np_ceres.NO_CONVERGENCE and s["iterations"] == 15 and s["successful_steps"] < 15
    assert bin(s["accepted_mask"]).count("1") == s["successful_steps"]


# ------------------------------------------------------------------ the branch cases: what they reach, their conditions, and that the comparison bites
def _census(summaries):
    dogleg, rules, ends = set(), set(), set()
    for s in summaries:
        dogleg |= {b for b, _ in s["census"]}
        rules |= {r for _, r in s["census"]}
        ends.add(s["termination"])
    return dict(dogleg=dogleg, rules=rules, ends=ends)


def test_branch_cases_reach_every_branch_with_margins():
    """Building the list asserts, per case, assert_margins and the one-ulp condition (the same decisions with every input one ulp up, a noise floor of at
    most 1e-7).  Here: the union of the census is the required set -- so a changed seed cannot lose a branch silently -- and the cases the list has to hold."""
    cases = tr.branch_cases()
    by_name = {b["name"]: b for b in cases}
    assert len(by_name) == len(cases)
    summ = {b["name"]: b["restated"][3] for b in cases}
    assert _census(summ.values()) == tr.REQUIRED_CENSUS
    for b in cases:
        assert b["floor"] <= 1e-7 and b["gate"] == max(1e-9, 100.0 * b["floor"])
        assert all(r["c"] > 0.0 for r in summ[b["name"]]["dogleg"] if r["branch"] == "interp"), b["name"]
    # (a) a nominal gap on both sides of every pass boundary
    for N in (9, 10, 18, 19, 27, 28):
        assert by_name[f"nominal_{N}"]["gap"]["n_frames"] == N and summ[f"nominal_{N}"]["termination"] == np_ceres.FUNCTION_TOL
    # (b) cauchy and interp in every pass-count class; (c) every radius rule on a gap of more than one pass
    reached, rules = set(), set()
    for b in cases:
        N = b["gap"]["n_frames"]
        for branch, rule in summ[b["name"]]["census"]:
            reached.add((branch, tr.pass_class(N)))
            if N > 9:
                rules.add(rule)
    assert {(br, k) for br in ("cauchy", "interp") for k in range(4)} <= reached, reached
    assert rules == set(tr.RADIUS_RULES), rules
    # (d) PARAMETER_TOLERANCE at 3 frames and over more than one pass, at iteration 1 and at iteration 2 (assert_margins took an IndexError on this end)
    pt = {(b["gap"]["n_frames"], s["iterations"]) for b in cases for s in [summ[b["name"]]] if s["termination"] == np_ceres.PARAMETER_TOL}
    assert {n for n, _ in pt} >= {3} and any(n > 9 for n, _ in pt) and {i for _, i in pt} == {1, 2}, pt
    for b in cases:
        s = summ[b["name"]]
        if s["termination"] == np_ceres.PARAMETER_TOL:          # the estimate is the last accepted iterate, never the candidate that ended the solve
            assert s["successful_steps"] == s["iterations"] - 1 and np.abs(b["restated"][2][:, 0:3]).min() > 9e4
    # (e) FAILURE at entry; GRADIENT_TOLERANCE before the first iteration
    s = summ["failure_at_entry_3"]
    assert (s["termination"], s["iterations"], s["successful_steps"], s["accepted_mask"]) == (np_ceres.FAILURE, 0, 0, 0)
    assert np.array_equal(by_name["failure_at_entry_3"]["restated"][2], by_name["failure_at_entry_3"]["restated"][0][:3])
    assert (summ["gradient_tol_1"]["termination"], summ["gradient_tol_1"]["iterations"]) == (np_ceres.GRADIENT_TOL, 0)


def test_iteration_limit_cases():
    got = {b["name"]: b for b in tr.limit_cases()}
    b = got["nominal_10_limit_0"]
    s = b["restated"][3]
    assert (s["termination"], s["iterations"], s["accepted_mask"]) == (np_ceres.NO_CONVERGENCE, 0, 0) and s["final_cost"] == s["initial_cost"]
    assert np.array_equal(b["restated"][2], b["restated"][0][:10])
    for name, first in (("cauchy_1_limit_1", "cauchy"), ("nominal_9_limit_1", "gn")):
        s = got[name]["restated"][3]
        assert (s["termination"], s["iterations"], s["accepted_mask"]) == (np_ceres.NO_CONVERGENCE, 1, 1) and s["census"][0][0] == first
    s = got["interp_18_far_limit_32"]["restated"][3]
    assert (s["termination"], s["iterations"]) == (np_ceres.NO_CONVERGENCE, 32) and s["accepted_mask"] >> 31 == 1 and 0 < s["successful_steps"] < 32
    assert bin(s["accepted_mask"]).count("1") == s["successful_steps"] and {"gn", "interp"} <= {br for br, _ in s["census"]}


def test_resolve_cases():
    gaps, kf = tr.resolve_cases()
    assert {g["spec"]["n_frames"] for g in gaps} == {0, 1, 9, 10, 18, 19, 27, 28, 32} and len(kf) == len(gaps) + 1
    c = _census(g["summary"] for g in gaps)
    assert c["dogleg"] == set(tr.DOGLEG_BRANCHES) and c["rules"] == set(tr.RADIUS_RULES), c
    assert {np_ceres.GRADIENT_TOL, np_ceres.FUNCTION_TOL, np_ceres.NO_CONVERGENCE, tr.NOT_SOLVED} <= c["ends"]
    for kind in ("consistent", "disturbed", "closure"):
        classes = {tr.pass_class(g["spec"]["n_frames"]) for g in gaps if g["spec"]["kind"] == kind and g["spec"]["n_frames"]}
        assert 0 in classes and len(classes) >= 3, (kind, classes)          # one pass, and at least two of the multi-pass classes
    multi = {br for g in gaps if g["spec"]["n_frames"] > 9 for br, _ in g["summary"]["census"]}
    assert multi == set(tr.DOGLEG_BRANCHES), multi
    for k, g in enumerate(gaps):
        N = g["spec"]["n_frames"]
        assert np.array_equal(g["left"], kf[k]) and np.array_equal(g["right"], kf[k + 1])
        if g["spec"]["kind"] == "consistent" and N:
            assert (g["summary"]["termination"], g["summary"]["iterations"]) == (np_ceres.GRADIENT_TOL, 0)
            assert np.array_equal(g["poses"], tr.resolve_init(g["meas"], kf[k], N))


class _SwappedBeta(tr.CensusDogleg):
    def _traditional_step(self):
        step = super()._traditional_step()
        if self.log[-1]["branch"] != "interp":
            return step
        g, gn, r, a = self.grad, self.gn, self.radius, self.alpha
        b_dot_a = -a * (g @ gn)
        a2 = a * a * (g @ g)
        bma2 = gn @ gn - 2 * b_dot_a + a2
        c = b_dot_a - a2
        d = np.sqrt(c * c + bma2 * (r * r - a2))
        beta = (d - c) / bma2 if c > 0 else (r * r - a2) / (d + c)
        s = (-a * (1 - beta)) * g + beta * gn
        self.step_norm = np.linalg.norm(s)
        return s


class _MisSignedBeta(tr.CensusDogleg):
    """the root of the other sign: beta = (-d - c) / |b - a|^2"""
    def _traditional_step(self):
        step = super()._traditional_step()
        if self.log[-1]["branch"] != "interp":
            return step
        g, gn, r, a = self.grad, self.gn, self.radius, self.alpha
        b_dot_a = -a * (g @ gn)
        a2 = a * a * (g @ g)
        bma2 = gn @ gn - 2 * b_dot_a + a2
        c = b_dot_a - a2
        d = np.sqrt(c * c + bma2 * (r * r - a2))
        beta = (-d - c) / bma2
        s = (-a * (1 - beta)) * g + beta * gn
        self.step_norm = np.linalg.norm(s)
        return s


class _RadiusFromRadius(tr.CensusDogleg):
    def accepted(self, q):
        self.step_norm = self.radius          # radius = max(radius, 3 radius) where the code has 3 step_norm
        super().accepted(q)


class _CauchyTimesAlpha(tr.CensusDogleg):
    def _traditional_step(self):
        step = super()._traditional_step()
        if self.log[-1]["branch"] != "cauchy":
            return step
        self.step_norm = self.radius * self.alpha
        return -(self.radius * self.alpha / np.linalg.norm(self.grad)) * self.grad


def _boundary_cost(sign):
    class Graph(tr.LocalGraph):
        """factor k0 + 9, which evaluate() meets as the last of one pass and the first of the next, counted twice (sign 1) or not at all (-1)"""
        def evaluate(self, x):
            ev = super().evaluate(x)
            if ev is None:
                return None
            cost, H, g = ev
            N = len(x)
            for a, b, mi in tr.factor_list(N):
                f = a + 1
                if 0 < f < N and f % 9 == 0:
                    r = tr.factor_residual(self.meas[mi], x[a], x[b])
                    cost = cost + sign * 0.5 * (r @ r)
            return cost, H, g
    return Graph


PUSH_VARIANTS = {
    "the cost of factor k0 + 9 counted twice": dict(graph=_boundary_cost(1.0)),
    "the cost of factor k0 + 9 not counted": dict(graph=_boundary_cost(-1.0)),
    "beta of the other root": dict(dogleg=_MisSignedBeta),
    "radius = max(radius, 3 radius)": dict(dogleg=_RadiusFromRadius),
    "the candidate taken at a tolerance end": dict(take_candidate=True),
    "a Cauchy step of length radius alpha": dict(dogleg=_CauchyTimesAlpha),
}


def _rejecting_cases(variant, stop_at_first=True):
    out = []
    for b in tr.branch_cases() + tr.limit_cases():
        rows, meas, sol, summ, _ = b["restated"]
        c, N = b["gap"], b["gap"]["n_frames"]
        if summ["termination"] == np_ceres.FAILURE:
            continue
        got, gs, _ = tr.local_graph(meas, c["anchor_left"], c["anchor_right"], rows[:N], b["max_iterations"], **variant)
        try:
            tr.assert_same_solve(b["name"], got, gs, sol, summ, b["gate"])
        except AssertionError:
            out.append(b["name"])
            if stop_at_first:
                break
    return out


@pytest.mark.parametrize("what", sorted(PUSH_VARIANTS))
def test_the_comparison_rejects_a_wrong_solver(what):
    """assert_same_solve, the function the GPU tests hold the device to, fed a deliberately wrong restatement on the cases of the list with each case's own
    gate: at least one case refuses it.  The right restatement passes (the first assertion)."""
    b = tr.branch_cases()[0]
    tr.assert_same_solve(b["name"], b["restated"][2], b["restated"][3], b["restated"][2], b["restated"][3], b["gate"])
    assert _rejecting_cases(PUSH_VARIANTS[what]), what


def test_a_candidate_taken_at_either_tolerance_end_is_rejected():
    names = _rejecting_cases(dict(take_candidate=True), stop_at_first=False)
    assert any(n.startswith("parameter_tol") for n in names) and any(n.startswith("nominal") or n.startswith("function_tol") for n in names), names


def test_the_two_beta_formulas_are_one_root():
    """Swapping the two formulas of beta is NOT a wrong solver and no case can refuse it: with d^2 = c^2 + |b - a|^2 (r^2 - |a|^2),
    (d - c) / |b - a|^2 = (r^2 - |a|^2) / (d + c) identically -- the same root of the quadratic, each form free of cancellation on its side of c = 0.  The
    swapped forms agree with the code's to the cases' gates on every case (held here, so that nobody adds the swap to PUSH_VARIANTS and hunts for a seed);
    the beta that IS wrong, the other root (-d - c) / |b - a|^2, is in PUSH_VARIANTS and is refused."""
    assert _rejecting_cases(dict(dogleg=_SwappedBeta), stop_at_first=False) == []
    rng = np.random.default_rng(8)
    for _ in range(100):
        c, bma2, r2_a2 = rng.normal(), rng.uniform(0.1, 10.0), rng.uniform(0.1, 10.0)
        d = np.sqrt(c * c + bma2 * r2_a2)
        assert abs((d - c) / bma2 - r2_a2 / (d + c)) <= 1e-9 * abs(r2_a2 / (d + c))


def test_the_comparison_rejects_a_wrong_resolve_start():
    """the start chain of a resolve composed with measurement i where the code takes max(i - 1, 0)"""
    gaps, kf = tr.resolve_cases()
    rejected = []
    for g in gaps:
        N = g["spec"]["n_frames"]
        cur, x0 = g["left"], []
        for i in range(N):
            cur = tr.compose(cur, g["meas"][i])
            x0.append(cur)
        got, gs, _ = tr.local_graph(g["meas"], g["left"], g["right"], np.array(x0).reshape(-1, 7))
        try:
            tr.assert_same_solve(g["name"], got, gs, g["poses"], g["summary"], g["gate"])
        except AssertionError:
            rejected.append(g["name"])
    assert rejected, "no gap of the resolve tells the two start chains apart"
    print(rejected)

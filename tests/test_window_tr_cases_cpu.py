"""The cases of tests/window_tr_cases.py do what the table claims (CPU only): the oracle and the numpy restatement of the Ceres loop agree on
every one, together they take every branch of the trust-region loop a solve can reach, no decision of the loop sits near its threshold,
and the spread between the two witnesses' iterates -- the yardstick tests/test_hip_window_tr_branches.py measures the device's prefixes
with -- is the one recorded in tests/golden/window_tr_spread.json."""
import numpy as np
import pytest

import window_tr_cases as wc

NAMES = list(wc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_witnesses_agree(name):
    """the tolerances of tests/test_oracle_tr_pins.py's _compare_window, plus the final radius (1e-9, as the per-iteration radius) and the gradient
    norm of the summary (1e-6, the device's gate)"""
    c = wc.classify(name)
    summ, info, hist, nh = c["summary"], c["np_summary"], c["hist"], c["np_hist"]
    assert (info["iterations"], info["termination"], info["successful_steps"]) == (summ.iterations, summ.termination, summ.successful_steps), (info, summ.as_dict())
    if summ.termination == wc.TERMINATIONS["FAILURE"]:           # the fifth invalid step ends the solve before either side writes its row
        assert len(nh) == len(hist) - 1 and not hist[-1].any()
        hist = hist[:-1]
    assert len(nh) == len(hist)
    assert np.allclose(nh[:, 0], hist[:, 0], rtol=1e-9), (nh[:, 0], hist[:, 0])
    assert np.allclose(nh[:, 1], hist[:, 1], rtol=1e-9), (nh[:, 1], hist[:, 1])
    assert np.allclose(nh[:, 2], hist[:, 2], rtol=1e-6, atol=1e-12)
    assert np.isclose(info["final_cost"], summ.final_cost, rtol=1e-10) and np.isclose(info["initial_cost"], summ.initial_cost, rtol=1e-10)
    assert np.isclose(info["final_radius"], summ.final_radius, rtol=1e-9), (info["final_radius"], summ.final_radius)
    assert np.isclose(info["gradient_max_norm"], summ.gradient_max_norm, rtol=1e-6), (info["gradient_max_norm"], summ.gradient_max_norm)
    assert np.abs(wc.flat_state(c["np_solution"]) - wc.flat_state(c["solution"])).max() < 1e-9
    if wc.exact_radius_prefix(name) >= summ.iterations:
        assert info["final_radius"] == summ.final_radius


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_branches(name):
    """if synth changes and a case drifts off its branch, this fails rather than the GPU test silently testing less"""
    want, got = wc.CASES[name]["expect"], wc.labels(name)
    print(name, got, "iterations", len(wc.classify(name)["iterations"]))
    assert want.get("kinds", set()) <= got["kinds"], (name, got)
    assert want.get("outcomes", set()) <= got["outcomes"], (name, got)
    if "termination" in want:
        assert got["termination"] == want["termination"], (name, got)
    its = wc.classify(name)["iterations"]
    if name in ("small_radius", "radius_20", "marg_prior"):      # boundary steps first, each tripling the radius, then Gauss-Newton steps
        nb = sum(r["kind"] == "cauchy" for r in its)
        assert nb == dict(small_radius=9, radius_20=2, marg_prior=6)[name]
        assert all(r["kind"] == "cauchy" and r["radius_after"] == 3.0 * r["radius_before"] for r in its[:nb]) and all(r["kind"] == "gn" for r in its[nb:])
    if name in ("far_w5", "far_w12_prior"):                      # a natural rejection followed by the re-entry with the stored vectors and the halved radius
        assert any(a["outcome"] == "rejected" and a["ratio"] < 0 and b["radius_before"] == 0.5 * a["radius_before"] and b.get("gn_norm") == a.get("gn_norm")
                   for a, b in zip(its, its[1:]))
        assert any(r["outcome"] == "accept_lo" and r["radius_after"] == 0.5 * r["radius_before"] for r in its)
    if name == "far_w5_prior":
        run = best = 0
        for r in its:
            run = run + 1 if r["outcome"] == "rejected" else 0
            best = max(best, run)
        assert best >= 20
    if name == "mid_ratios":
        assert all(r["radius_after"] == r["radius_before"] for r in its) and sum(r["outcome"] == "accept_mid" for r in its) >= 15
    if name == "forced_rejects":
        assert [k for k, _ in __import__("itertools").groupby(r["kind"] for r in its)] == ["gn", "interp", "cauchy"]
    if name == "lm_reject":                                      # the doubling decrease factor: radius / 2, / 4, / 8, ...
        assert [r["radius_before"] / r["radius_after"] for r in its[:-1]] == [2.0 ** (k + 1) for k in range(len(its) - 1)]
        assert wc.classify(name)["summary"].final_radius == 1e-2 / 2.0 ** 21
    if name == "failure":
        win, _, start, _ = wc.build(name)
        assert len(its) == 5 and all(r["outcome"] == "invalid" for r in its)
        assert np.array_equal(wc.flat_state(wc.classify(name)["solution"]), wc.flat_state(start))


def test_the_table_covers_every_branch():
    kinds, outcomes, terms, strategies = set(), set(), set(), set()
    for name in NAMES:
        l = wc.labels(name)
        kinds |= l["kinds"]; outcomes |= l["outcomes"]; terms.add(l["termination"]); strategies.add(l["strategy"])
    assert kinds == set(wc.KINDS), kinds
    assert outcomes == set(wc.OUTCOMES), outcomes
    assert terms == set(range(6)), terms
    assert strategies == {0, 1}
    # both strategies reject, and Levenberg-Marquardt ends on its own minimum radius
    assert "rejected" in wc.labels("lm_reject")["outcomes"] and wc.labels("lm_min_radius")["termination"] == wc.TERMINATIONS["MIN_RADIUS"]
    # the interpolation's other sign (c <= 0) is not reachable from a solve (module docstring): every interpolated step has c > 0
    cs = [r["interp_c"] for name in NAMES for r in wc.classify(name)["iterations"] if r["kind"] == "interp"]
    print(f"{len(cs)} interpolated steps, c / (|a| |b|) in [{min(cs):.3g}, {max(cs):.3g}]")
    assert len(cs) >= 20 and min(cs) > 0


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_sits_on_its_threshold(name):
    """A condition on the inputs: every comparison the loop decides on stays clear of its threshold by a relative 1e-4, six orders above the
    1e-10 to which device and oracle linearisations agree.
    far_w5 accepts a step with ratio 1.03e-3 against min_relative_decrease = 1e-3 at iteration 21: 3 % clear of the threshold, i.e. 3e-5 in
    the ratio.  The two witnesses' iterates differ by 1e-11 m there and their candidate costs by 5e-12 relative, which moves the ratio by
    ~1e-8: three orders inside the gap, so the case is kept whole."""
    worst = (np.inf, None)
    for k, what, v, t in wc.margins(name):
        rel = abs(v - t) / max(abs(v), abs(t), 1e-300)
        worst = min(worst, (rel, (k, what, v, t)), key=lambda w: w[0])
        assert rel > wc.MARGIN, (name, k, what, v, t)
    print(f"{name}: closest decision {worst[1]} at a relative {worst[0]:.3g}")
    assert len(wc.margins(name)) >= 2


def test_truncations_cut_at_most_a_quarter():
    """lm_accept is the one case cut short (window_tr_cases.py says why): 18 of the 24 iterations the uncapped solve takes"""
    from oracle import pyoracle as po
    win, corr, start, use = wc.build("lm_accept")
    _, full = po.Problem(wc.with_max_iterations(win, 60), corr, **use).solve(start)
    assert full.termination == wc.TERMINATIONS["FUNCTION_TOL"]
    assert 4 * win.opts.max_iterations >= 3 * full.iterations, (win.opts.max_iterations, full.iterations)


@pytest.mark.parametrize("name", NAMES)
def test_prefix_spread_is_the_recorded_one(name):
    """S_k = max |x_oracle,k - x_numpy,k| per part of the state after k iterations.  The golden file holds the values the GPU tolerances come
    from (PYTHONPATH=. python tests/window_tr_cases.py rewrites it); they are rounding noise and differ between machines, so what is asserted is that this
    machine's values stay inside the tolerance the GPU test derives from the recorded ones, and that the record is complete."""
    golden = wc.load_golden()
    rows = wc.spread(name)
    assert name in golden and all(len(golden[name][p]) == len(rows) for p in wc.STATE_GATES), name
    tol = wc.prefix_tolerances(name, golden)
    worst = 0.0
    for k, row in enumerate(rows):
        for p, v in row.items():
            worst = max(worst, v / tol[k][p])
            assert v <= tol[k][p], (name, k, p, v, tol[k][p])
    print(f"{name}: {len(rows)} prefixes, largest S_k / tolerance {worst:.2e}, largest S_k {max(max(r.values()) for r in rows):.2e}")
    # the oracle's capped runs are the prefixes of its own solve: same summary at k = n, iteration counts 0 .. n
    pre = wc.oracle_prefixes(name)
    assert [m.iterations for _, m in pre] == list(range(len(pre)))
    assert pre[-1][1].final_cost == wc.classify(name)["summary"].final_cost

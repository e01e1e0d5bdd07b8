"""CPU: the numpy restatement of the damped solve (tests/pose_graph_lm_restated.py) checked against itself -- the radius rule on hand-made gains, the short
form of the model decrease against the Jacobian, the damped against the undamped restatement where Gauss-Newton converges, and the drives whose drift makes
Gauss-Newton end ABOVE its start.  The spreads between the restatement's own three linear solvers on those drives are what the GPU tests
(test_hip_pose_graph_lm.py) scale their tolerances from; they are committed in tests/golden/pose_graph_lm_spread.json
(`python tests/test_pose_graph_lm_restated.py` writes the file again)."""
import json
import os

import numpy as np
import pytest

import pose_graph_lm_restated as LM
import pose_graph_restated as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pose_graph_lm_spread.json")
GN_GOLD = json.load(open(os.path.join(HERE, "golden", "pose_graph_spread.json")))
# What bounds the spreads.  Relative poses: the damped systems are better conditioned than the undamped ones of pose_graph_spread.json, but the drives are up to
# 200 nodes with poses disturbed by 0.1 rad per edge and ten to thirteen accepted steps feed on each other: 1e-10 m / 1e-11 rad leaves one digit above what was
# measured when the file was written (9.4e-12 m, 2.7e-13 rad).  The error per trial is a sum of ~1e3 squares of size ~1e4: 1e-11 relative.  The model decrease
# is a difference that shrinks to ~1e-6 of the error as the solve converges, and the radius carries the cube of a gain formed from it: 1e-6 relative.
BOUNDS = dict(S_rel_m=1e-10, S_rel_rad=1e-11, S_error_rel=1e-11, S_model_rel=1e-6, S_radius_rel=1e-6)
SOLVERS = ("lstsq", "cholesky", "sparse")
PAIRS = (("lstsq", "cholesky"), ("lstsq", "sparse"), ("cholesky", "sparse"))


# ------------------------------------------------------------------------------------------------------------------------------------ the radius rule
def test_radius_rule_on_hand_made_gains():
    assert LM.radius_accepted(1e4, 1.0) == 3e4                              # 1 - (2 - 1)^3 = 0: the floor 1/3
    assert LM.radius_accepted(1e4, 0.5) == 1e4                              # 1 - 0 = 1
    assert LM.radius_accepted(1e4, 1e-3) == pytest.approx(1e4 / (1.0 - (2e-3 - 1.0) ** 3), rel=1e-15) and LM.radius_accepted(1e4, 1e-3) < 1e4 / 1.99
    assert LM.radius_accepted(1e16, 1.0) == 1e16                            # max_radius
    r, f, seen = 8e3, 2.0, []
    for _ in range(3):
        r, f = LM.radius_rejected(r, f)
        seen.append(r)
    assert seen == [4e3, 1e3, 125.0] and f == 16.0                          # / 2, / 4, / 8
    # an acceptance resets the factor
    state = (8e3, 2.0)
    for accepted, gain, want in ((False, None, (4e3, 4.0)), (False, None, (1e3, 8.0)), (True, 0.5, (1e3, 2.0)), (False, None, (500.0, 4.0)), (True, 1.0, (1500.0, 2.0))):
        state = LM.radius_update(*state, accepted, gain)
        assert state == want
    # ... and in the loop itself, on a drive made to reject
    x0, _, g = LM.drift_scene(80, 0.1, 0.05, 1)
    _, info = LM.levenberg_marquardt(g, x0)
    h = info["history"]
    v = h[:, 3].astype(int).tolist()
    k = v.index(0)
    assert 0 < k < len(v) - 2 and v[k + 1] == 1, v
    assert h[k + 1, 1] == h[k, 1] / 2.0                                     # the rejection halves the radius
    assert h[k + 2, 1] == LM.radius_accepted(h[k + 1, 1], (h[k - 1, 0] - h[k + 1, 0]) / h[k + 1, 2])    # the trial after it starts from the error before it
    assert info["final_error"] < info["initial_error"] and info["accepted"] + info["rejected"] == info["trials"]


def test_every_trial_invalid_leaves_the_start():
    """a node at its prior: g = 0, delta = 0, m = 0 -- invalid every time; 1e4 / 2^(k (k + 1) / 2) <= 1e-32 first at k = 15"""
    x0 = W.circle_truth(3)[:1]
    g = W.Graph()
    g.add_prior(0, x0[0])
    x, info = LM.levenberg_marquardt(g, x0)
    assert info["termination"] == LM.MIN_RADIUS and info["trials"] == 15 and info["invalid"] == 15 and info["accepted"] == 0
    assert np.array_equal(x, x0)
    x, info = LM.levenberg_marquardt(g, x0, max_trials=4)
    assert info["termination"] == LM.ITERATION_LIMIT and info["trials"] == 4 and np.array_equal(x, x0)


# ------------------------------------------------------------------------------------------------------------------------------------ the model decrease
@pytest.mark.parametrize("radius", [1e-3, 1.0, 1e4, 1e12])
def test_short_form_of_the_model_decrease(radius):
    x0, _, g = LM.drift_scene(40, 5e-2, 3e-2, 3)
    g.add_gps(7, x0[7, :3] + [0.5, -0.2, 0.1], [1.0, 1.0, 4.0])
    g.add_between(30, 2, W.between(x0[31], x0[2]), np.full(6, 0.09))         # two loops share node 2
    r, J = g.linearize(x0)
    d = LM.damping(J)
    for solver in ("cholesky", "lstsq"):
        delta = LM.damped_step(J, r, d, radius, solver)
        short, full = LM.model_decrease(delta, J.T @ r, d, radius), LM.model_decrease_from_jacobian(J, r, delta)
        assert short > 0 and abs(short - full) <= 1e-9 * full, (solver, short, full)
    # the diagonal is the complete one: node 2 carries its two chain factors and both loops
    H = J.T @ J
    assert np.allclose(LM.normal_diagonal(J), np.diag(H), rtol=1e-14)
    _, Js = g.linearize(x0, sparse=True)
    assert np.allclose(LM.normal_diagonal(Js), np.diag(H), rtol=1e-14)


# ------------------------------------------------------------------------------------------------------------------------------------ where Gauss-Newton converges
def test_damped_and_undamped_end_at_the_same_poses_on_the_circle():
    """both run to rounding (no termination on the error): the relative poses agree within the committed spread between the undamped solvers itself
    (1.42e-14 m / 6.66e-16 rad against the committed 1.53e-14 m / 7.84e-16 rad when this was written).  (The absolute translation is a gauge that the
    damping releases only as the radius grows past 1e12: it is not compared.)"""
    x0, _, g = W.circle_scene()
    want, wi = W.gauss_newton(g, x0, solver="cholesky", max_iterations=10, fixed=True)
    x, info = LM.levenberg_marquardt(g, x0, solver="cholesky", max_trials=30, rel_tol=0.0, abs_tol=-1e300)
    dt, da = W.spread(x, want, True)
    print(dt, da, info["history"][:, 3].astype(int).tolist())
    assert info["trials"] == 30 and info["termination"] == LM.ITERATION_LIMIT
    assert dt <= GN_GOLD["S_rel_m"] and da <= GN_GOLD["S_rel_rad"], (dt, da)
    assert abs(info["final_error"] - wi["final_error"]) <= 1e-12 * wi["final_error"]
    # with the object's own termination the two stop at the same minimum, each by its own last decrease: micrometres
    xd, di = LM.levenberg_marquardt(g, x0)
    assert di["termination"] == LM.CONVERGED and di["rejected"] == 0
    dt, da = W.spread(xd, want, True)
    assert dt < 1e-5 and da < 1e-6 and abs(di["final_error"] - wi["final_error"]) < 1e-5


# ------------------------------------------------------------------------------------------------------------------------------------ the drives with drift
@pytest.fixture(scope="module")
def drift():
    out = {}
    for sc in LM.DRIFT_SCENES:
        x0, _, g = LM.drift_scene(*sc)
        out[sc] = (x0, g, W.gauss_newton(g, x0, solver="sparse"), LM.levenberg_marquardt(g, x0, solver="sparse"))
    return out


@pytest.mark.parametrize("sc", LM.DRIFT_SCENES)
def test_gauss_newton_ends_above_its_start_and_the_damped_solve_below(drift, sc):
    x0, g, (xg, gi), (xl, li) = drift[sc]
    print(sc, gi, {k: v for k, v in li.items() if k not in ("history", "steps")})
    assert gi["termination"] == W.CONVERGED and gi["iterations"] == 1 and gi["final_error"] > gi["initial_error"]
    assert li["termination"] == LM.CONVERGED and li["final_error"] < 0.6 * li["initial_error"] and 8 <= li["accepted"] <= 15
    assert li["initial_error"] == gi["initial_error"]
    e = np.r_[li["initial_error"], li["history"][li["history"][:, 3] == 1, 0]]
    assert (np.diff(e) < 0).all()                                           # monotonic: every accepted trial lowers the error
    assert abs(g.error(xl) - li["final_error"]) <= 1e-12 * li["final_error"] and abs(g.error(xg) - gi["final_error"]) <= 1e-12 * gi["final_error"]


def drift_spreads(scenes):
    s = dict.fromkeys(BOUNDS, 0.0)
    for sc in scenes:
        x0, _, g = LM.drift_scene(*sc)
        runs = {k: LM.levenberg_marquardt(g, x0, solver=k) for k in SOLVERS}
        for a, b in PAIRS:
            (xa, ia), (xb, ib) = runs[a], runs[b]
            ha, hb = ia["history"], ib["history"]
            assert np.array_equal(ha[:, 3], hb[:, 3]), (sc, a, b)           # the same accept / reject sequence
            dt, da = W.spread(xa, xb, True)
            rel = lambda c: float(np.max(np.abs(ha[:, c] - hb[:, c]) / np.abs(ha[:, c])))
            for key, v in (("S_rel_m", dt), ("S_rel_rad", da), ("S_error_rel", rel(0)), ("S_radius_rel", rel(1)), ("S_model_rel", rel(2))):
                s[key] = max(s[key], v)
    return s


def test_solvers_agree_on_a_drive_with_drift_and_the_spreads_are_the_committed_ones():
    """the three solvers on the cheapest of the drives (the file holds the largest over all four), and the committed figures inside their bounds"""
    s = drift_spreads([LM.DRIFT_SCENES[2]])
    print(s)
    gold = json.load(open(GOLDEN))
    assert [list(x) for x in LM.DRIFT_SCENES] == gold["scenes"]
    for key, bound in BOUNDS.items():
        assert 0 < gold[key] <= bound, key
        assert s[key] <= bound, (key, s[key])


if __name__ == "__main__":
    s = drift_spreads(LM.DRIFT_SCENES)
    s.update(scenes=[list(x) for x in LM.DRIFT_SCENES],
             what="largest difference between the lstsq, dense Cholesky and sparse LU runs of pose_graph_lm_restated.levenberg_marquardt on its DRIFT_SCENES: final "
                  "poses relative to node 0, and per trial the error tried, the model decrease and the radius (relative)")
    json.dump(s, open(GOLDEN, "w"), indent=1)
    print(open(GOLDEN).read())

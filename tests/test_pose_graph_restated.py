"""CPU: the numpy restatement of the pose graph (tests/pose_graph_restated.py) checked against itself -- analytic Jacobians against central differences, the
linear solvers against each other and against scipy.optimize.least_squares on the 60-node circle.  The two spreads between the solvers are what the GPU tests
(test_hip_pose_graph.py) scale their tolerances from; they are committed in tests/golden/pose_graph_spread.json (`python tests/test_pose_graph_restated.py`
writes the file again)."""
import json
import os

import numpy as np
import pytest

import pose_graph_restated as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_spread.json")
# The relative poses are determined to about cond * eps of their size: information 1e6 (rotation) / 1e4 (translation) per edge against a loop of 1 / 0.09 over
# 60 nodes, poses of 20 m -- 1e-12 m / 1e-13 rad leaves two digits above the 1.5e-14 m / 8e-16 rad measured when the file was written.  The absolute poses hang on
# the prior's 1e-8 translation information against 1e4: a gauge, loose to ~1e-4 m after 10 iterations.
S_REL_BOUND = (1e-12, 1e-13)
S_ABS_BOUND = (1e-2, 1e-7)


def rand_pose(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return np.r_[rng.normal(0, 3, 3), W.so3_exp(angle * ax)]


def numeric_jac(fun, xs, k, h=1e-6):
    cols = []
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        xp, xm = list(xs), list(xs)
        xp[k], xm[k] = W.retract(xs[k], d), W.retract(xs[k], -d)
        cols.append((fun(*xp) - fun(*xm)) / (2 * h))
    return np.array(cols).T


# residual angles: exactly 0, far below / just below / just above the series switches of Log (|v| = 1e-3 <-> theta = 2e-3) and of the inverse right Jacobian
# (theta = 1e-2), ordinary and large
ANGLES = [0.0, 1e-9, 1e-5, 1.9e-3, 2.1e-3, 0.99e-2, 1.01e-2, 0.3, 1.5, 3.0]


@pytest.mark.parametrize("angle", ANGLES)
def test_between_jacobians_against_central_differences(angle):
    rng = np.random.default_rng(3)
    xi, xj = rand_pose(rng, 0.7), rand_pose(rng, 2.0)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    m = W.between(xi, xj)
    m = np.r_[m[:3] + rng.normal(0, 0.1, 3), W.q_mul(m[3:], W.so3_exp(-angle * ax))]     # the residual rotation is Exp(angle ax)
    var = np.array([1e-2, 2e-2, 3e-2, 0.5, 1.0, 2.0])
    r, Ji, Jj = W.between_factor(xi, xj, m, var)
    assert abs(np.linalg.norm(r[:3] * np.sqrt(var[:3])) - angle) < 1e-12
    f = lambda a, b: W.between_factor(a, b, m, var)[0]
    for k, J in ((0, Ji), (1, Jj)):
        num = numeric_jac(f, [xi, xj], k)
        assert np.abs(num - J).max() < 2e-8 * max(1.0, np.abs(J).max()), (k, np.abs(num - J).max())


@pytest.mark.parametrize("angle", ANGLES)
def test_prior_and_gps_jacobians_against_central_differences(angle):
    rng = np.random.default_rng(4)
    x = rand_pose(rng, 1.1)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    m = np.r_[x[:3] + rng.normal(0, 0.2, 3), W.q_mul(x[3:], W.so3_exp(-angle * ax))]
    var = np.array([1e-2, 1e-2, 0.5, 2.0, 3.0, 4.0])
    r, J = W.prior_factor(x, m, var)
    num = numeric_jac(lambda a: W.prior_factor(a, m, var)[0], [x], 0)
    assert np.abs(num - J).max() < 2e-8 * max(1.0, np.abs(J).max())
    p = x[:3] + rng.normal(0, 1, 3)
    r, J = W.gps_factor(x, p, np.array([1.0, 1.0, 4.0]))
    num = numeric_jac(lambda a: W.gps_factor(a, p, np.array([1.0, 1.0, 4.0]))[0], [x], 0)
    assert np.abs(num - J).max() < 2e-8


def test_series_are_continuous_at_their_switch():
    for t in (W.JRINV_SERIES_BELOW * (1 - 1e-9), W.JRINV_SERIES_BELOW * (1 + 1e-9)):
        phi = np.array([t, 0, 0])
        c_exact = 1.0 / (t * t) - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
        assert abs((W.jr_inv(phi) - np.eye(3) - 0.5 * W.skew(phi))[1, 1] / (-t * t) - c_exact) < 1e-11
    for t in (2e-3 * (1 - 1e-9), 2e-3 * (1 + 1e-9)):          # |v| = sin(theta / 2) on either side of 1e-3
        assert abs(W.so3_log(W.so3_exp([t, 0, 0]))[0] - t) < 5e-18


def circle_spreads():
    x0, _, g = W.circle_scene()
    sols = {s: W.gauss_newton(g, x0, solver=s, max_iterations=10, fixed=True)[0] for s in ("lstsq", "cholesky", "sparse")}
    pairs = [("lstsq", "cholesky"), ("lstsq", "sparse"), ("cholesky", "sparse")]
    s_rel = np.max([W.spread(sols[a], sols[b], True) for a, b in pairs], axis=0)
    s_abs = np.max([W.spread(sols[a], sols[b], False) for a, b in pairs], axis=0)
    return x0, g, sols, s_rel, s_abs


def test_solvers_agree_on_the_circle_and_the_spreads_are_the_committed_ones():
    x0, g, sols, s_rel, s_abs = circle_spreads()
    print(f"S_rel {s_rel[0]:.2e} m {s_rel[1]:.2e} rad; S_abs {s_abs[0]:.2e} m {s_abs[1]:.2e} rad")
    assert s_rel[0] <= S_REL_BOUND[0] and s_rel[1] <= S_REL_BOUND[1], s_rel
    assert s_abs[0] <= S_ABS_BOUND[0] and s_abs[1] <= S_ABS_BOUND[1], s_abs
    gold = json.load(open(GOLDEN))
    assert gold["seed"] == W.CIRCLE_SEED and gold["nodes"] == 60 and gold["iterations"] == 10
    assert 0 < gold["S_rel_m"] <= S_REL_BOUND[0] and 0 < gold["S_rel_rad"] <= S_REL_BOUND[1]
    assert 0 < gold["S_abs_m"] <= S_ABS_BOUND[0] and 0 < gold["S_abs_rad"] <= S_ABS_BOUND[1]
    # the chain starts at its own measurements, so the initial error is the loop's alone; spreading it over the chain lowers it
    e0, e1 = g.error(x0), g.error(sols["cholesky"])
    assert 0 < e1 < e0


def test_least_squares_finds_the_same_minimum():
    """an independent minimiser (trust region reflective on the same residuals, parametrised by one global tangent at the initial poses) ends at the same relative poses"""
    from scipy.optimize import least_squares
    x0, _, g = W.circle_scene()
    n = len(x0)

    def unpack(d):
        return np.array([W.retract(x0[i], d[6 * i:6 * i + 6]) for i in range(n)])

    def res(d):
        return np.concatenate([b[0] for b in g.blocks(unpack(d))])

    def jac(d):
        # chain rule from the local tangent at x0 [+] d back to d: d_r moves the local rotation by the right Jacobian, d_t by Exp(d_r)^T
        _, J = g.linearize(unpack(d))
        for i in range(n):
            T = np.zeros((6, 6))
            T[:3, :3] = np.linalg.inv(W.jr_inv(d[6 * i:6 * i + 3]))
            T[3:, 3:] = W.q_mat(W.so3_exp(d[6 * i:6 * i + 3])).T
            J[:, 6 * i:6 * i + 6] = J[:, 6 * i:6 * i + 6] @ T
        return J

    sol = least_squares(res, np.zeros(6 * n), jac=jac, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0, max_nfev=200)
    want = W.gauss_newton(g, x0, solver="cholesky", max_iterations=10, fixed=True)[0]
    dt, da = W.spread(unpack(sol.x), want, True)
    assert abs(0.5 * float(sol.fun @ sol.fun) - g.error(want)) < 1e-9 * g.error(want)
    # a trust-region method stops on its own criteria, not at rounding: micrometres
    assert dt < 1e-6 and da < 1e-7, (dt, da)


def test_termination_is_on_the_error():
    x0, _, g = W.circle_scene()
    x, info = W.gauss_newton(g, x0, solver="cholesky")
    assert info["termination"] == W.CONVERGED and 2 <= info["iterations"] <= 8
    x2, info2 = W.gauss_newton(g, x, solver="cholesky")
    assert info2["termination"] == W.CONVERGED and info2["iterations"] == 1


def test_sparse_solver_on_a_long_graph():
    truth = W.figure_eight_truth(400)
    x0 = W.noisy_odometry(truth, np.random.default_rng(1), 1e-3, 3e-3)
    g = W.Graph()
    g.add_prior(0, x0[0])
    g.add_chain(x0)
    g.add_between(399, 0, W.between(truth[399], truth[0]), np.full(6, 0.05))
    g.add_between(300, 100, W.between(truth[300], truth[100]), np.full(6, 0.05))
    a = W.gauss_newton(g, x0, solver="sparse", max_iterations=6, fixed=True)[0]
    b = W.gauss_newton(g, x0, solver="cholesky", max_iterations=6, fixed=True)[0]
    dt, da = W.spread(a, b, True)
    assert dt < 1e-10 and da < 1e-11, (dt, da)


if __name__ == "__main__":
    _, _, _, s_rel, s_abs = circle_spreads()
    json.dump({"seed": W.CIRCLE_SEED, "nodes": 60, "iterations": 10, "S_rel_m": float(s_rel[0]), "S_rel_rad": float(s_rel[1]), "S_abs_m": float(s_abs[0]),
               "S_abs_rad": float(s_abs[1]), "what": "largest difference between the lstsq, dense Cholesky and sparse LU Gauss-Newton runs of pose_graph_restated.circle_scene()"},
              open(GOLDEN, "w"), indent=1)
    print(open(GOLDEN).read())

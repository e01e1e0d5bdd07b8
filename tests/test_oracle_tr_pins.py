"""Pins of the oracle's SOLVER semantics (what fixes iteration counts and terminations every parity test gates on) against an
independent numpy restatement of the Ceres 1.14 trust-region loop (tests/np_ceres.py, written from the bundled docs
GraphGNSSLibV1.1/docs/source/nnls_solving.rst:83-260,1056-1188 and the published Ceres sources; numpy cholesky / qr / roots
instead of the oracle's hand-written loops).  Both sides evaluate cost / H / g with the oracle's factor code (pinned separately by
tests/test_oracle_pins.py, tests/test_oracle_factors.py); what is compared here is the LOOP: per-iteration candidate cost, radius
and step norm, the termination, the returned point.  CPU only."""
import numpy as np
import pytest

import np_ceres as nc
from glio_amd import batch, synth
from glio_amd import ctypes_types as T
from oracle import pyoracle as po
# the window problem's callbacks for np_ceres.minimize live in tests/window_tr_cases.py (the trust-region branch cases use them too)
from window_tr_cases import np_opts_from as _np_opts_from
from window_tr_cases import quat_plus as _quat_plus
from window_tr_cases import window_callbacks as _window_callbacks


# ------------------------------------------------------------------ sliding-window problem (orc_solver.c)
def _compare_window(win, corr, expect_rejected=False, **prob_kw):
    prob = po.Problem(win, corr, **prob_kw)
    sol, summ, hist = prob.solve_history(win.init)
    evaluate, plus, flat = _window_callbacks(prob)
    x, info, nh = nc.minimize(win.init.copy(), evaluate, plus, flat, _np_opts_from(win.opts))
    assert info["iterations"] == summ.iterations and info["termination"] == summ.termination and info["successful_steps"] == summ.successful_steps, (info, summ.as_dict())
    nh = np.array(nh).reshape(-1, 3)
    assert len(nh) == len(hist)
    assert np.allclose(nh[:, 0], hist[:, 0], rtol=1e-9), (nh[:, 0], hist[:, 0])           # candidate cost per iteration
    assert np.allclose(nh[:, 1], hist[:, 1], rtol=1e-9)                                    # radius per iteration
    assert np.allclose(nh[:, 2], hist[:, 2], rtol=1e-6, atol=1e-12)                        # step norm per iteration
    assert np.isclose(info["final_cost"], summ.final_cost, rtol=1e-10)
    assert np.abs(flat(x) - flat(sol)).max() < 1e-9
    if expect_rejected:
        assert summ.successful_steps < summ.iterations - 1, "this case is meant to contain a rejected step"
    return summ, hist


def test_window_dogleg_history_equals_the_numpy_restatement():
    win = synth.make_window(W=4, pts_per_scan=400, with_gnss=True, with_prior=False, seed=synth.SEED_BASE + 301)
    summ, hist = _compare_window(win, synth.analytic_correspondences(win))
    assert summ.iterations >= 3


def test_window_with_prior_and_rejected_steps():
    """a badly perturbed start and a small initial radius: the first steps leave the region where the model is good"""
    win = synth.make_window(W=5, pts_per_scan=300, with_gnss=False, with_prior=True, seed=synth.SEED_BASE + 302, perturb=(8.0, 50.0, 2.0))
    win.opts.max_iterations = 40
    summ, hist = _compare_window(win, synth.analytic_correspondences(win), expect_rejected=True)


def test_window_levenberg_marquardt_history():
    win = synth.make_window(W=1, pts_per_scan=600, with_gnss=False, with_prior=False, seed=synth.SEED_BASE + 303, perturb=(0.3, 2.0, 0.0))
    win.opts.trust_region_strategy = 1
    win.opts.max_iterations = 12
    summ, hist = _compare_window(win, synth.analytic_correspondences(win), use_imu=False)
    assert summ.iterations >= 3


def test_window_invalid_steps_end_in_failure_on_both_sides():
    """an overflowing bias Jacobian of the pre-integration makes J^T J infinite, so every factorisation fails: five invalid steps,
    then FAILURE (TrustRegionMinimizer::HandleInvalidStep)"""
    win = synth.make_window(W=2, pts_per_scan=100, with_gnss=False, with_prior=False, seed=synth.SEED_BASE + 304)
    corr = synth.analytic_correspondences(win)
    win.preints[0]["jacobian"][0, 9] = 1e200
    prob = po.Problem(win, corr)
    sol, summ, hist = prob.solve_history(win.init)
    evaluate, plus, flat = _window_callbacks(prob)
    with np.errstate(all="ignore"):
        x, info, nh = nc.minimize(win.init.copy(), evaluate, plus, flat, _np_opts_from(win.opts))
    assert summ.termination == nc.FAILURE == info["termination"] and summ.iterations == info["iterations"] == 5


# ------------------------------------------------------------------ batch problem (orc_batch2.c)
def _batch_problem(K=24, band=6, per_kf=60, seed=41, with_imu=True, with_small=True, perturb=(0.08, 0.004)):
    gt, init = batch.make_poses(K, seed=seed, perturb=perturb)
    ci, cj, cp, ncent, score = batch.make_constraints(gt, 0, K, per_kf, band, seed=seed)
    dq = dd = frame = None
    if with_small:
        odo = gt.copy(); odo[:, :3] += np.random.default_rng(seed).normal(0, 0.02, (K, 3))
        dq = batch.delta_q_pairs(odo, 3)
        dd, frame = batch.make_batch_gnss(gt, seed=seed)
        for f in dd:
            f.threshold = 10.0
    imu = sb0 = None
    if with_imu:
        imu, sb_gt, sb0 = batch.make_batch_imu(K, seed=seed)
    P = po.BatchProblem(K, band, ci, cj, cp.numpy(), ncent.numpy(), score.numpy(), dq=dq, dd=dd, frame=frame, imu=imu)
    return P, gt, init, sb0


def _batch_callbacks(P):
    K, B = P.K, 15 if P.n_imu else 6

    def plus(x, d):
        poses, sb = x
        out = poses.copy()
        for k in range(K):
            out[k, :3] = poses[k, :3] + d[B * k:B * k + 3]
            out[k, 3:] = _quat_plus(poses[k, 3:], d[B * k + 3:B * k + 6])
        sbo = sb + d.reshape(K, B)[:, 6:] if B == 15 else sb
        return out, sbo

    def flat(x):
        return np.concatenate([x[0].ravel(), x[1].ravel()]) if B == 15 else x[0].ravel()

    def evaluate(x):
        H, g, c = P.linearize_dense(x[0], x[1])
        return c, H, g

    return evaluate, plus, flat


def _compare_batch(P, init, sb0, opts, np_kw):
    x, sb, summ, hist = P.solve2(init, opts, sb0, want_history=True)
    evaluate, plus, flat = _batch_callbacks(P)
    start = (init.copy(), sb0.copy() if sb0 is not None else np.zeros(0))
    o = nc.Options(max_iterations=opts.max_iterations, nonmonotonic=bool(opts.use_nonmonotonic_steps), **np_kw)
    xn, info, nh = nc.minimize(start, evaluate, plus, flat, o)
    assert info["iterations"] == summ.iterations and info["termination"] == summ.termination and info["successful_steps"] == summ.successful_steps, (info, summ.as_dict())
    nh = np.array(nh).reshape(-1, 3)
    assert np.allclose(nh[:, 0], hist[:, 0], rtol=1e-8), (nh[:, 0], hist[:, 0])
    assert np.allclose(nh[:, 1], hist[:, 1], rtol=1e-8)
    assert np.allclose(nh[:, 2], hist[:, 2], rtol=1e-5, atol=1e-12)
    assert np.isclose(info["final_cost"], summ.final_cost, rtol=1e-9)
    assert np.abs(xn[0] - x).max() < 1e-8
    if sb is not None:
        assert np.abs(xn[1] - sb).max() < 1e-7
    return summ, hist


@pytest.mark.parametrize("dogleg", ["traditional", "subspace"])
def test_batch_pose_problem_history(dogleg):
    P, gt, init, _ = _batch_problem(with_imu=False, seed=41)
    opts = T.batch_tr_opts(max_iterations=30, dogleg=T.DOGLEG_SUBSPACE if dogleg == "subspace" else T.DOGLEG_TRADITIONAL)
    summ, hist = _compare_batch(P, init, None, opts, dict(dogleg=dogleg))
    assert summ.final_cost < 0.1 * summ.initial_cost


def test_batch_problem_with_the_imu_chain_history():
    P, gt, init, sb0 = _batch_problem(with_imu=True, seed=43)
    opts = T.batch_tr_opts(max_iterations=30)
    summ, hist = _compare_batch(P, init, sb0, opts, dict(dogleg="subspace"))
    assert summ.iterations >= 3 and summ.final_cost < summ.initial_cost


def test_subspace_step_is_taken_on_the_boundary_and_cost_raising_steps_are_accepted():
    """a small initial radius forces boundary-constrained subspace minimisations (the quartic), and the non-monotonic rule accepts
    steps that raise the cost: the returned point must then be the minimum-cost iterate, not the last one (Ceres copies x to the
    user's parameters only when x_cost < minimum_cost)."""
    P, gt, init, sb0 = _batch_problem(K=20, per_kf=40, with_imu=True, seed=47, perturb=(0.4, 0.03))
    opts = T.batch_tr_opts(max_iterations=12)
    opts.initial_trust_region_radius = 0.5
    summ, hist = _compare_batch(P, init, sb0, opts, dict(dogleg="subspace", initial_radius=0.5))
    assert np.any(np.isclose(hist[:, 2] > 0, True))
    # boundary steps: the D-scaled step norm equals the radius, so the parameter step is of the radius' order and below it
    x, sb, s2, h2 = P.solve2(init, opts, sb0, want_history=True)
    costs = h2[:, 0]
    accepted_up = [i for i in range(1, len(costs)) if h2[i, 3] > opts.min_relative_decrease and costs[i] > min(costs[:i].min(), s2.initial_cost)]
    if accepted_up:      # a cost-raising step was accepted somewhere: the summary must report the minimum
        assert np.isclose(s2.final_cost, min(s2.initial_cost, min(c for c, q in zip(costs, h2[:, 3]) if q > opts.min_relative_decrease)), rtol=1e-12)


def test_quartic_roots_and_boundary_minimum_against_numpy():
    rng = np.random.default_rng(5)
    for _ in range(200):
        A = rng.normal(size=(2, 2)) * 10 ** rng.uniform(-2, 3)
        B = A @ A.T + 1e-6 * np.eye(2)
        g = rng.normal(size=2) * 10 ** rng.uniform(-2, 3)
        r = 10 ** rng.uniform(-3, 1)
        x_gn = -np.linalg.solve(B, g)
        if np.linalg.norm(x_gn) <= r:
            continue
        out = np.zeros(2)
        ok = po.lib().orc_subspace_boundary_minimum(T.dptr(np.ascontiguousarray(B.ravel())), T.dptr(g), po.C.c_double(r), T.dptr(out))
        assert ok
        # reference: the trust-region subproblem's multiplier by bisection on |x(y)| = r, y >= 0
        lo, hi = 0.0, 1.0
        nx = lambda y: np.linalg.norm(np.linalg.solve(B + y * np.eye(2), g))
        while nx(hi) > r:
            hi *= 2
        for _k in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if nx(mid) > r else (lo, mid)
        want = -np.linalg.solve(B + hi * np.eye(2), g)
        assert np.allclose(out, want, rtol=1e-6, atol=1e-9 * r), (out, want)
    coeffs = np.array([2.0, -3.0, -11.0, 3.0, 9.0])
    roots = np.zeros(8); n = po.C.c_int()
    assert po.lib().orc_poly_roots_real(T.dptr(coeffs), 4, T.dptr(roots), po.C.byref(n)) and n.value == 4
    assert np.allclose(np.sort(roots[:4]), np.sort(np.real(np.roots(coeffs))), atol=1e-10)

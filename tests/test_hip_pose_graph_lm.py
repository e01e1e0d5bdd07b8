"""GPU: glio_pgraph_solve_damped -- the damped solve of the pose graph (csrc/posegraph_kernels.hip, include/glio_pgraph_lm.h) against its numpy restatement
tests/pose_graph_lm_restated.py, which never imports the product (tests/test_pose_graph_lm_restated.py checks it against itself on the CPU).  The margins are
100 x the committed spreads between the restatement's own three linear solvers (tests/golden/pose_graph_lm_spread.json: final poses relative to node 0, and per
trial the error tried, the model decrease and the radius) -- the margin test_hip_pose_graph.py uses against its witness, for the same reason: the device and the
witness are exact eliminations in different orders.  The absolute translation is numerically a gauge under the reference's prior, and the damping releases it
only as the radius grows: absolute poses are not compared."""
import json
import os

import numpy as np
import pytest

import pose_graph_lm_restated as LM
import pose_graph_restated as W
from glio_amd import capi, posegraph
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "pose_graph_lm_spread.json")))
GN_GOLD = json.load(open(os.path.join(HERE, "golden", "pose_graph_spread.json")))
POSE_TOL = (100 * GOLD["S_rel_m"], 100 * GOLD["S_rel_rad"])
ERROR_TOL, MODEL_TOL, RADIUS_TOL = 100 * GOLD["S_error_rel"], 100 * GOLD["S_model_rel"], 100 * GOLD["S_radius_rel"]
LOOP_VAR = np.full(6, 0.09)
GPS_VAR = np.array([1.0, 1.0, 4.0])
SMALL = dict(max_nodes=256, max_loops=8, max_unary=16)
NEVER = dict(relative_error_tol=0.0, absolute_error_tol=-1e300)          # no termination on the error: the trial limit (or the radius) ends the solve


def witness(x0, loops=(), gps=(), prior=None, prior_var=W.PRIOR_VAR):
    g = W.Graph()
    g.add_prior(0, x0[0] if prior is None else prior, prior_var)
    g.add_chain(x0)
    for lp in loops:
        g.add_between(*lp)
    for gp in gps:
        g.add_gps(*gp)
    return g


def device_graph(opts, x0, loops=(), gps=(), prior=None, prior_var=None):
    pg = posegraph.PoseGraph(opts)
    pg.set_prior(x0[0] if prior is None else prior, prior_var)
    pg.append(x0)
    for lp in loops:
        pg.add_between(*lp)
    for gp in gps:
        pg.add_gps(*gp)
    return pg


def check_relative_poses(got, want, what, tol=POSE_TOL):
    rel = W.spread(got, want, True)
    print(f"{what}: relative to node 0 {rel[0]:.2e} m {rel[1]:.2e} rad (tol {tol[0]:.1e} {tol[1]:.1e}); absolute {W.spread(got, want, False)}")
    assert np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got[:, 3:], axis=1) - 1).max() < 1e-15 and (got[:, 3] >= 0).all()
    assert rel[0] <= tol[0] and rel[1] <= tol[1], (what, rel)


def check_history(info, wi, what):
    """the same accept / reject sequence, and per trial the error tried, the radius used and the model decrease within the margins"""
    h, wh = info.history, wi["history"]
    print(f"{what}: device {info.as_dict()}")
    print(f"{what}: witness verdicts {wh[:, 3].astype(int).tolist()} termination {wi['termination']} {wi['initial_error']} -> {wi['final_error']}")
    assert h[:, 3].astype(int).tolist() == wh[:, 3].astype(int).tolist(), what
    assert (info.trials, info.accepted, info.rejected, info.invalid, info.termination) == (wi["trials"], wi["accepted"], wi["rejected"], wi["invalid"], wi["termination"])
    assert info.iterations == info.trials == len(h) and info.accepted + info.rejected == info.trials
    for c, tol, name in ((0, ERROR_TOL, "error"), (1, RADIUS_TOL, "radius"), (2, MODEL_TOL, "model decrease")):
        d = np.abs(h[:, c] - wh[:, c]) / np.abs(wh[:, c]) if len(h) and (wh[:, c] != 0).all() else np.abs(h[:, c] - wh[:, c])
        print(f"{what}: {name} per trial, largest relative difference {d.max() if len(d) else 0:.2e} (tol {tol:.1e})")
        assert (d <= tol).all(), (what, name, d)
    for got, want, tol in ((info.initial_error, wi["initial_error"], ERROR_TOL), (info.final_error, wi["final_error"], ERROR_TOL), (info.final_radius, wi["final_radius"], RADIUS_TOL)):
        assert abs(got - want) <= tol * abs(want), (what, got, want)
    assert info.final_error <= info.initial_error


def against_witness(opts, x0, loops=(), gps=(), prior=None, lm_kw=None, what="", solver="cholesky", wit=None, tol=POSE_TOL, prior_var=None):
    lm_kw = dict(lm_kw or {})
    if wit is None:
        wit = LM.levenberg_marquardt(witness(x0, loops, gps, prior, W.PRIOR_VAR if prior_var is None else prior_var), x0, solver=solver, max_trials=lm_kw.get("max_trials") or opts.max_iterations,
                                     rel_tol=opts.relative_error_tol, abs_tol=opts.absolute_error_tol, **{k: v for k, v in lm_kw.items() if k != "max_trials"})
    pg = device_graph(opts, x0, loops, gps, prior, prior_var)
    info = pg.solve_damped(posegraph.default_lm_opts(**lm_kw) if lm_kw else None)
    got = pg.read_poses()
    assert pg.error() == info.final_error                      # the pose table IS the last accepted estimate
    pg.close()
    check_history(info, wit[1], what)
    check_relative_poses(got, wit[0], what, tol)
    return info, got, wit


# ------------------------------------------------------------------------------------------------------------------------------------ 1: the gap and its closure
@pytest.fixture(scope="module")
def drift():
    x0, loop, g = LM.drift_scene(150, 5e-2, 3e-2, 1)
    return dict(x0=x0, loop=loop, wit=LM.levenberg_marquardt(g, x0, solver="sparse"))


def test_gauss_newton_leaves_a_worse_estimate_on_a_drive_with_drift(drift):
    """the gap: passes without the damped solve"""
    pg = device_graph(posegraph.default_opts(**SMALL), drift["x0"], [drift["loop"]])
    e0 = pg.error()
    info = pg.solve()
    print(info.as_dict())
    assert info.termination == T.PGRAPH_CONVERGED and info.iterations == 1 and info.final_error > info.initial_error == e0
    assert pg.error() == info.final_error > e0                 # ... and the worse estimate is what the pose table holds
    pg.close()


def test_the_damped_solve_closes_it(drift):
    info, got, _ = against_witness(posegraph.default_opts(**SMALL), drift["x0"], [drift["loop"]], what="drift 150", wit=drift["wit"])
    assert info.termination == T.PGRAPH_CONVERGED and info.final_error < 0.5 * info.initial_error and info.rejected == 0
    assert info.termination_name == "CONVERGED" and info.device_ms > 0 and all(s > 0 for s in info.stage_ms) and info.segments >= 10


# ------------------------------------------------------------------------------------------------------------------------------------ 2: rejections
def test_a_rejected_trial_leaves_the_estimate_untouched():
    x0, loop, g = LM.drift_scene(80, 0.1, 0.05, 1)
    wit = LM.levenberg_marquardt(g, x0, solver="cholesky")
    v = wit[1]["history"][:, 3].astype(int).tolist()
    k = v.index(0)                                              # trial k (from 0) is the first rejected one; the witness alone decides that the scene serves
    assert 0 < k < len(v) - 1 and 1 in v[k + 1:], v
    opts = posegraph.default_opts(**SMALL)
    info, _, _ = against_witness(opts, x0, [loop], what="rejection", wit=wit)
    assert info.rejected >= 1 and info.invalid == 0 and info.termination == T.PGRAPH_CONVERGED
    tables = []
    for trials in (k, k + 1):                                   # up to the rejected trial, and through it
        pg = device_graph(opts, x0, [loop])
        i = pg.solve_damped(posegraph.default_lm_opts(max_trials=trials))
        assert i.trials == trials and i.termination == T.PGRAPH_ITERATION_LIMIT and i.history[:, 3].astype(int).tolist() == v[:trials]
        tables.append((pg.read_poses(), i))
        pg.close()
    assert np.array_equal(tables[0][0].view(np.uint64), tables[1][0].view(np.uint64))
    assert tables[0][1].final_error == tables[1][1].final_error and tables[1][1].final_radius == tables[0][1].final_radius / 2.0


# ------------------------------------------------------------------------------------------------------------------------------------ 3: the diagonal at loop endpoints
def tangent(x0, x1):
    """delta with x1 = x0 [+] delta"""
    return np.array([np.r_[W.so3_log(W.q_mul(W.q_conj(a[3:]), b[3:])), W.q_mat(a[3:]).T @ (b[:3] - a[:3])] for a, b in zip(x0, x1)])


def test_the_damping_takes_the_complete_diagonal_at_loop_endpoints():
    """9 nodes, two interior nodes per segment, loops 8 -> 0 and 8 -> 3 sharing an endpoint, a GPS factor on node 4, ONE trial at radius 1e-3: the damping
    d / rho is a thousand times the matrix, so delta_i ~ -g_i rho / d_i shows d_i itself.  A diagonal without the loops' blocks is wrong by ~1e-3 of d at nodes
    0, 3, 8 (information 11 against 1e4), without the GPS block by ~1e-4 at node 4.  The margins: delta is read back through poses of ~20 m, i.e. to
    ~1e-14 m / 1e-15 rad, on top of 1e-9 of its size (the system's condition is ~1 at this radius); m is a sum of positive terms of that accuracy."""
    truth = W.circle_truth(9, z_amp=0.5)
    x0 = W.noisy_odometry(truth, np.random.default_rng(31), 2e-2, 5e-2)
    loops = [(8, 0, W.between(truth[8], truth[0]), LOOP_VAR), (8, 3, W.between(truth[8], truth[3]), LOOP_VAR)]
    gps = [(4, truth[4, :3] + [0.6, -0.4, 0.3], GPS_VAR)]
    g = witness(x0, loops, gps)
    xw, wi = LM.levenberg_marquardt(g, x0, solver="cholesky", max_trials=1, initial_radius=1e-3)
    assert wi["accepted"] == 1
    pg = device_graph(posegraph.default_opts(segment_nodes=2, **SMALL), x0, loops, gps)
    info = pg.solve_damped(posegraph.default_lm_opts(max_trials=1, initial_radius=1e-3))
    got = pg.read_poses()
    pg.close()
    assert info.trials == 1 and info.accepted == 1 and info.termination == T.PGRAPH_ITERATION_LIMIT and info.history[0, 1] == 1e-3
    d, dw = tangent(x0, got), wi["steps"][0].reshape(-1, 6)
    err = np.abs(d - dw)
    floor = np.r_[np.full(3, 2e-15), np.full(3, 5e-14)]
    print("delta per node, largest |difference| / |delta|:", (err / np.abs(dw)).max(axis=1), "m", info.history[0, 2], wi["history"][0, 2])
    assert (err <= 1e-9 * np.abs(dw) + floor).all(), err / np.abs(dw)
    # what the bound must tell apart: the step under a diagonal from the chain / unary blocks alone
    r, J = g.linearize(x0)
    _, Jc = witness(x0, (), gps).linearize(x0)
    dmiss = LM.damping(Jc)
    wrong = LM.damped_step(J, r, dmiss, 1e-3, "cholesky").reshape(-1, 6)
    assert (np.abs(wrong - dw)[[0, 3, 8]] > 100 * (1e-9 * np.abs(dw) + floor)[[0, 3, 8]]).any(axis=1).all()
    assert abs(info.history[0, 2] - wi["history"][0, 2]) <= 1e-10 * wi["history"][0, 2]
    assert abs(info.history[0, 0] - wi["history"][0, 0]) <= ERROR_TOL * wi["history"][0, 0]


# ------------------------------------------------------------------------------------------------------------------------------------ 4: small and edge shapes
def scene24():
    truth = W.circle_truth(24, z_amp=0.5)
    return truth, W.noisy_odometry(truth, np.random.default_rng(13), 2e-3, 5e-3)


def test_one_node_at_its_prior_every_trial_invalid():
    """a pose whose prior residual is zero to the bit (no rotation, a translation that subtracts exactly): g = 0, delta = 0, m = 0 -- invalid every time, the
    radius falls 1e4 / 2^(k (k + 1) / 2) to 1e-32 in 15 trials, the estimate stays"""
    x0 = np.array([[1.5, -2.0, 0.25, 1.0, 0.0, 0.0, 0.0]])
    for lm_kw, term, trials in ((None, T.PGRAPH_MIN_RADIUS, 15), (dict(max_trials=4), T.PGRAPH_ITERATION_LIMIT, 4)):
        pg = device_graph(posegraph.default_opts(**SMALL), x0[:1])
        info = pg.solve_damped(posegraph.default_lm_opts(**lm_kw) if lm_kw else None)
        print(info.as_dict())
        assert (info.termination, info.trials, info.invalid, info.rejected, info.accepted) == (term, trials, trials, trials, 0)
        assert info.final_error == info.initial_error == 0.0 and np.array_equal(pg.read_poses(), x0[:1])
        assert info.termination_name == ("MIN_RADIUS" if lm_kw is None else "ITERATION_LIMIT")
        pg.close()


SIX, THREE = 6, 3        # trials of the edge shapes (of those with one or two nodes): short of the minimum's rounding, where a verdict is noise


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_nodes(n):
    """a prior (translation variance 1, so that it weighs) and a GPS fix that disagree -- the minimum is not zero: N = 1 has no segment launch, N = 2 one
    separator pair without an interior node"""
    truth, x0 = scene24()
    gps = [(n - 1, truth[n - 1, :3] + [0.8, -0.5, 0.4], GPS_VAR)]
    prior = W.retract(x0[0], np.array([0.02, -0.01, 0.03, 0.1, -0.2, 0.05]))
    against_witness(posegraph.default_opts(max_iterations=THREE, **NEVER, **SMALL), x0[:n], gps=gps, prior=prior, prior_var=np.r_[np.full(3, 1e-2), np.ones(3)],
                    what=f"{n} node(s)")


def edge_case(name):
    truth, x0 = scene24()
    L = lambda i, j: (i, j, W.between(truth[i], truth[j]), LOOP_VAR)
    return {"adjacent_endpoints": (x0, [L(20, 5), L(21, 6)]), "first_to_last": (x0, [L(0, 23)]), "shared_endpoint": (x0, [L(23, 3), L(15, 3)]),
            "duplicates_a_chain_edge": (x0, [L(10, 11), L(22, 2)]), "two_nodes_and_a_loop": (x0[:2], [(1, 0, W.between(truth[1], truth[0]), LOOP_VAR)]),
            "no_interior_node": (x0, [L(12, 10), L(9, 8), L(23, 22)])}[name]


EDGE_WITNESS = {}


@pytest.mark.parametrize("segment_nodes", [1, 2, 4])
@pytest.mark.parametrize("name", ["adjacent_endpoints", "first_to_last", "shared_endpoint", "duplicates_a_chain_edge", "two_nodes_and_a_loop", "no_interior_node"])
def test_segment_edge_cases(name, segment_nodes):
    x0, loops = edge_case(name)
    opts = posegraph.default_opts(max_iterations=THREE if len(x0) == 2 else SIX, segment_nodes=segment_nodes, **NEVER, **SMALL)
    _, _, EDGE_WITNESS[name] = against_witness(opts, x0, loops, what=f"{name} / {segment_nodes}", wit=EDGE_WITNESS.get(name))


@pytest.fixture(scope="module")
def eight():
    n = 3000
    truth = W.figure_eight_truth(n)
    x0 = W.noisy_odometry(truth, np.random.default_rng(14), 1e-3, 3e-3)
    loops = [(i, j, W.between(truth[i], truth[j]), LOOP_VAR) for i, j in ((750, 0), (1500, 0), (2250, 750), (2999, 1500), (2999, 3), (2250, 1497))]
    # the restatement is per-edge Python: three trials of 3 000 nodes keep the shared fixture to a few seconds
    return dict(x0=x0, loops=loops, wit=LM.levenberg_marquardt(witness(x0, loops), x0, solver="sparse", max_trials=3, rel_tol=0.0, abs_tol=-1e300))


@pytest.mark.parametrize("segment_nodes", [16, 0])
def test_many_segments(eight, segment_nodes):
    opts = posegraph.default_opts(max_iterations=3, segment_nodes=segment_nodes, max_nodes=3000, max_loops=8, max_unary=4, **NEVER)
    info, _, _ = against_witness(opts, eight["x0"], eight["loops"], what=f"figure of eight / {segment_nodes}", wit=eight["wit"])
    assert info.segments >= (3000 // 17 if segment_nodes else 40)


# ------------------------------------------------------------------------------------------------------------------------------------ 5: where Gauss-Newton converges
def test_on_the_circle_it_ends_where_gauss_newton_ends():
    """Both to rounding on the device: Gauss-Newton with a fixed iteration count, the damped solve with thirty fixed trials (the count
    tests/test_pose_graph_lm_restated.py shows the restatement needs).  The bound is the committed spread of pose_graph_spread.json itself, 1 x, not the 100 x of
    a device-against-witness comparison: both sides are the same Cholesky in the same order.  But "where glio_pgraph_solve ends" is not one point to that
    accuracy.  Undamped steps never settle: after convergence the estimate wanders over a few ulp of its 20 m poses, and the device's own Gauss-Newton after 11,
    12, 15 and 20 iterations lies up to 2.3e-14 m / 8.9e-16 rad from its estimate after 10 (measured on an MI355X) -- MORE than the committed 1.53e-14 m /
    7.84e-16 rad, so against the 10th iterate alone Gauss-Newton would fail its own comparison.  Hence the reference's own error J is measured here, from
    glio_pgraph_solve alone, and the damped estimate must lie within S + J of the 10th iterate (the triangle inequality: within S of a point Gauss-Newton ends
    at, which is within J of the 10th).  Measured: 2.47e-14 m / 6.66e-16 rad against S + J = 3.84e-14 m / 1.67e-15 rad; against the 20th iterate it is
    1.00e-14 m / 4.44e-16 rad, inside S alone."""
    x0, loop, _ = W.circle_scene()
    small = dict(max_nodes=64, max_loops=8, max_unary=16)
    gn = {}
    for k in (10, 11, 12, 15, 20):
        pg = device_graph(posegraph.fixed_iterations(k, **small), x0, [loop])
        gi = pg.solve()
        gn[k] = pg.read_poses()
        pg.close()
        assert gi.iterations == k
    wander = np.max([W.spread(gn[k], gn[10], True) for k in gn if k != 10], axis=0)
    pg = device_graph(posegraph.fixed_iterations(30, **small), x0, [loop])
    info = pg.solve_damped()
    got = pg.read_poses()
    pg.close()
    S = (GN_GOLD["S_rel_m"], GN_GOLD["S_rel_rad"])
    print(info.as_dict())
    print("Gauss-Newton against its own 10th iterate:", wander, "committed spread:", S, "damped against every iterate:", {k: W.spread(got, gn[k], True) for k in gn})
    assert info.trials == 30 and info.accepted >= 20 and abs(info.final_error - gi.final_error) <= 1e-12 * gi.final_error
    assert wander[0] <= 10 * S[0] and wander[1] <= 10 * S[1]      # the reference's own error is of the spread's size, not a licence
    check_relative_poses(got, gn[10], "circle, damped against undamped", (S[0] + wander[0], S[1] + wander[1]))


# ------------------------------------------------------------------------------------------------------------------------------------ 6: determinism
def test_two_runs_give_the_same_bits():
    x0, loop, _ = LM.drift_scene(80, 0.1, 0.05, 1)              # the scene with a rejection
    runs = []
    for k in range(3):
        pg = device_graph(posegraph.default_opts(**SMALL), x0, [loop])
        if k == 2:                                              # the same object again after another solve and a clear: every solve starts from initial_radius
            pg.solve_damped()
            pg.clear()
            pg.set_prior(x0[0]); pg.append(x0); pg.add_between(*loop)
        info = pg.solve_damped()
        runs.append((pg.read_poses(), info))
        pg.close()
    fields = lambda i: (i.iterations, i.termination, i.initial_error, i.final_error, i.separators, i.segments, i.final_radius, i.accepted, i.rejected, i.invalid, i.trials)
    for p, info in runs[1:]:
        assert np.array_equal(p.view(np.uint64), runs[0][0].view(np.uint64))
        assert np.array_equal(info.history.view(np.uint64), runs[0][1].history.view(np.uint64))
        assert fields(info) == fields(runs[0][1])
    assert runs[0][1].rejected >= 1


# ------------------------------------------------------------------------------------------------------------------------------------ 7: the monotonic contract
def test_a_contradicting_loop_never_ends_above_its_start():
    """the input of test_hip_pose_graph.py::test_a_contradicting_loop_ends_with_a_status"""
    truth = W.circle_truth(12, z_amp=0.5)
    x0 = W.noisy_odometry(truth, np.random.default_rng(18), 2e-3, 5e-3)
    wrong = W.between(truth[11], truth[1])
    wrong = np.r_[wrong[:3], W.q_mul(wrong[3:], W.so3_exp([0, 0, np.pi / 2]))]
    pg = device_graph(posegraph.default_opts(max_nodes=64, max_loops=8, max_unary=16), x0, [(11, 1, wrong, np.full(6, 1e-12))])
    e0 = pg.error()
    info = pg.solve_damped()
    print(info.as_dict())
    assert info.termination in (T.PGRAPH_CONVERGED, T.PGRAPH_ITERATION_LIMIT, T.PGRAPH_MIN_RADIUS)
    assert info.initial_error == e0 and info.final_error <= e0 and pg.error() == info.final_error
    e = np.r_[e0, info.history[info.history[:, 3] == 1, 0]]
    assert (np.diff(e) < 0).all() and e[-1] == info.final_error
    p = pg.read_poses()
    assert np.isfinite(p).all() and np.abs(np.linalg.norm(p[:, 3:], axis=1) - 1).max() < 1e-12
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 8: refusals
def refused(fn, *a, **kw):
    with pytest.raises(capi.GlioError, match="error -1"):
        fn(*a, **kw)


def test_refusals_change_nothing_and_null_options_are_the_defaults():
    truth, x0 = scene24()
    loop = (23, 2, W.between(truth[23], truth[2]), LOOP_VAR)
    empty = posegraph.PoseGraph(posegraph.default_opts(**SMALL))
    refused(empty.solve_damped)                                 # no node
    empty.append(x0[:6])
    refused(empty.solve_damped)                                 # neither a prior nor a GPS factor
    empty.close()
    pg = device_graph(posegraph.default_opts(**SMALL), x0, [loop])
    state = lambda: (pg.size(), pg.error(), pg.read_poses())
    before = state()
    bad = dict(initial_radius=[0.0, -1.0, np.inf, np.nan, 1e-40, 1e17], max_radius=[0.0, np.inf, np.nan, 1e3], min_radius=[0.0, -1e-32, np.nan, 1e5],
               min_diagonal=[0.0, -1.0, np.nan, np.inf, 1e33], max_diagonal=[0.0, np.inf, np.nan, 1e-7], min_relative_decrease=[-1e-3, 1.0, 2.0, np.nan],
               max_trials=[-1])
    for field, values in bad.items():
        for v in values:
            refused(pg.solve_damped, posegraph.default_lm_opts(**{field: v}))
            after = state()
            assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2], before[2]), (field, v)
    lib, out = capi.load(), np.zeros((4, 4))
    assert lib.glio_pgraph_lm_history(pg._h, 0, 0, None) == 0 and lib.glio_pgraph_lm_history(pg._h, 0, 1, T.dptr(out)) == capi.E_ARG      # no damped solve yet
    # the bounds themselves are allowed: equal radii, equal diagonal bounds, min_relative_decrease 0
    a = pg.solve_damped(posegraph.default_lm_opts(initial_radius=1e4, max_radius=1e4, min_radius=1e4, min_relative_decrease=0.0, max_trials=2))
    assert a.trials >= 1 and a.final_error <= a.initial_error
    assert lib.glio_pgraph_lm_history(pg._h, a.trials - 1, 1, T.dptr(out)) == 0 and np.array_equal(out[0], a.history[-1])
    assert lib.glio_pgraph_lm_history(pg._h, a.trials, 1, T.dptr(out)) == capi.E_ARG and lib.glio_pgraph_lm_history(pg._h, -1, 1, T.dptr(out)) == capi.E_ARG
    pg.close()
    runs = []
    for lm in (None, posegraph.default_lm_opts()):
        pg = device_graph(posegraph.default_opts(**SMALL), x0, [loop])
        info = pg.solve_damped(lm)
        runs.append((pg.read_poses(), info))
        pg.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1].history, runs[1][1].history)
    assert runs[0][1].history[0, 1] == 1e4 and runs[0][1].termination == T.PGRAPH_CONVERGED

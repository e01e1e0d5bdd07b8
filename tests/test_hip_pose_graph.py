"""GPU: glio_pgraph_* -- the pose graph on the device (csrc/posegraph_kernels.hip) against the numpy restatement tests/pose_graph_restated.py, which never
imports the product (tests/test_pose_graph_restated.py checks the restatement against itself on the CPU).  The tolerances on poses come from the committed
spreads between the restatement's own linear solvers (tests/golden/pose_graph_spread.json): poses relative to node 0 within 100 x S_rel (two decimal digits
over a spread that was itself measured between two CPU factorisations: different summation orders over the edges, FMA contraction, another elimination order),
absolute poses within 10 x S_abs (the absolute translation is numerically a gauge under the reference's prior)."""
import json
import os

import numpy as np
import pytest

import pose_graph_restated as W
from glio_amd import capi, posegraph
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_spread.json")))
REL_TOL = (100 * GOLD["S_rel_m"], 100 * GOLD["S_rel_rad"])
ABS_TOL = (10 * GOLD["S_abs_m"], 10 * GOLD["S_abs_rad"])
LOOP_VAR = np.full(6, 0.09)
GPS_VAR = np.array([1.0, 1.0, 4.0])
SMALL = dict(max_nodes=64, max_loops=8, max_unary=16)


def scene(n, seed, radius=20.0, turn=0.98):
    truth = W.circle_truth(n, radius=radius, turn=turn, z_amp=0.5)
    return truth, W.noisy_odometry(truth, np.random.default_rng(seed), 2e-3, 5e-3)


def witness(x0, loops=(), gps=(), prior=True):
    g = W.Graph()
    if prior:
        g.add_prior(0, x0[0])
    g.add_chain(x0)
    for lp in loops:
        g.add_between(*lp)
    for gp in gps:
        g.add_gps(*gp)
    return g


def device_graph(opts, x0, loops=(), gps=(), prior=True, chunks=None):
    pg = posegraph.PoseGraph(opts)
    fill(pg, x0, loops, gps, prior, chunks)
    return pg


def fill(pg, x0, loops=(), gps=(), prior=True, chunks=None):
    if prior:
        pg.set_prior(x0[0])
    at = 0
    for c in (chunks or [len(x0)]):
        pg.append(x0[at:at + c], prev_pose=None if at == 0 else x0[at - 1])
        at += c
    assert at == len(x0)
    for lp in loops:
        pg.add_between(*lp)
    for gp in gps:
        pg.add_gps(*gp)


def loop_of(truth, i, j, var=LOOP_VAR):
    return (i, j, W.between(truth[i], truth[j]), var)


def check_poses(got, want, what=""):
    rel, ab = W.spread(got, want, True), W.spread(got, want, False)
    print(f"{what}: relative to node 0 {rel[0]:.2e} m {rel[1]:.2e} rad (tol {REL_TOL[0]:.1e} {REL_TOL[1]:.1e}); absolute {ab[0]:.2e} m {ab[1]:.2e} rad (tol {ABS_TOL[0]:.1e} {ABS_TOL[1]:.1e})")
    assert np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got[:, 3:], axis=1) - 1).max() < 1e-15 and (got[:, 3] >= 0).all()
    assert rel[0] <= REL_TOL[0] and rel[1] <= REL_TOL[1], (what, rel)
    assert ab[0] <= ABS_TOL[0] and ab[1] <= ABS_TOL[1], (what, ab)


def check_error(got, want):
    # relative 1e-10; a graph at its own measurements has an error of rounding squared, where only the size can be compared
    assert abs(got - want) <= 1e-10 * abs(want) + 1e-24, (got, want)


def against_witness(opts_kw, x0, loops=(), gps=(), prior=True, what="", iterations=10, solver="cholesky"):
    g = witness(x0, loops, gps, prior)
    want, wi = W.gauss_newton(g, x0, solver=solver, max_iterations=iterations, fixed=True)
    pg = device_graph(posegraph.fixed_iterations(iterations, **opts_kw), x0, loops, gps, prior)
    info = pg.solve()
    got = pg.read_poses()
    # (an error of exactly zero -- a single node at its prior -- ends the run at once: E_new <= 0 is part of the termination)
    assert (info.iterations == iterations and info.termination == T.PGRAPH_ITERATION_LIMIT) or info.final_error == 0.0, info.as_dict()
    check_poses(got, want, what)
    check_error(info.final_error, wi["final_error"])
    check_error(info.initial_error, wi["initial_error"])
    pg.close()
    return info


# ------------------------------------------------------------------------------------------------------------------------------------ 1: error and gradient
def test_error_and_first_iteration():
    truth, x0 = scene(9, 11)
    loops = [loop_of(truth, 8, 1)]
    gps = [(3, truth[3, :3] + [0.3, -0.2, 0.1], GPS_VAR), (6, truth[6, :3] + [-0.1, 0.4, 0.2], GPS_VAR)]
    g = witness(x0, loops, gps)
    pg = device_graph(posegraph.fixed_iterations(1, **SMALL), x0, loops, gps)
    e, we = pg.error(), g.error(x0)
    assert abs(e - we) <= 1e-12 * we, (e, we)
    info = pg.solve()
    want, _ = W.gauss_newton(g, x0, solver="cholesky", max_iterations=1, fixed=True)
    rel = W.spread(pg.read_poses(), want, True)
    print("first iteration, relative to node 0:", rel)
    assert info.iterations == 1 and abs(info.initial_error - we) <= 1e-12 * we
    assert rel[0] <= 1e-11 and rel[1] <= 1e-11, rel
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 2: a chain at its own measurements
def test_chain_at_its_own_measurements_stays():
    _, x0 = scene(33, 12)
    pg = device_graph(posegraph.default_opts(**SMALL), x0)
    info = pg.solve()
    got = pg.read_poses()
    dt, da = W.spread(got, x0, False)
    print(info.as_dict(), dt, da)
    assert info.iterations <= 2 and info.termination == T.PGRAPH_CONVERGED
    assert dt < 1e-9 and da < 1e-11
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 3: the 60-node circle
@pytest.fixture(scope="module")
def circle():
    x0, loop, g = W.circle_scene()
    want, wi = W.gauss_newton(g, x0, solver="cholesky", max_iterations=10, fixed=True)
    return dict(x0=x0, loop=loop, g=g, want=want, wi=wi)


def test_circle_against_the_witness(circle):
    pg = device_graph(posegraph.fixed_iterations(10, **SMALL), circle["x0"], [circle["loop"]])
    info = pg.solve()
    print(info.as_dict())
    assert info.iterations == 10
    check_poses(pg.read_poses(), circle["want"], "circle")
    check_error(info.final_error, circle["wi"]["final_error"])
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 4: segment edge cases
def edge_case(name):
    truth, x0 = scene(24, 13)
    L = lambda i, j: loop_of(truth, i, j)
    return {"adjacent_endpoints": (x0, [L(20, 5), L(21, 6)]),
            "first_to_last": (x0, [L(0, 23)]),
            "shared_endpoint": (x0, [L(23, 3), L(15, 3)]),
            "duplicates_a_chain_edge": (x0, [L(10, 11), L(22, 2)]),
            "one_node": (x0[:1], []),
            "two_nodes": (x0[:2], []),
            "two_nodes_and_a_loop": (x0[:2], [loop_of(truth, 1, 0)]),
            "no_interior_node": (x0, [L(12, 10), L(9, 8), L(23, 22)])}[name]


@pytest.mark.parametrize("segment_nodes", [1, 2, 4])
@pytest.mark.parametrize("name", ["adjacent_endpoints", "first_to_last", "shared_endpoint", "duplicates_a_chain_edge", "one_node", "two_nodes",
                                  "two_nodes_and_a_loop", "no_interior_node"])
def test_segment_edge_cases(name, segment_nodes):
    x0, loops = edge_case(name)
    against_witness(dict(segment_nodes=segment_nodes, **SMALL), x0, loops, what=f"{name} / {segment_nodes}")


# ------------------------------------------------------------------------------------------------------------------------------------ 5: many segments
EIGHT_ITERATIONS = 6         # the restatement is per-edge Python: six iterations of 3 000 nodes keep the shared fixture to a few seconds


@pytest.fixture(scope="module")
def eight():
    n = 3000
    truth = W.figure_eight_truth(n)
    x0 = W.noisy_odometry(truth, np.random.default_rng(14), 1e-3, 3e-3)
    loops = [loop_of(truth, i, j) for i, j in ((750, 0), (1500, 0), (2250, 750), (2999, 1500), (2999, 3), (2250, 1497))]
    g = witness(x0, loops)
    want, wi = W.gauss_newton(g, x0, solver="sparse", max_iterations=EIGHT_ITERATIONS, fixed=True)
    return dict(x0=x0, loops=loops, want=want, wi=wi, got={})


@pytest.mark.parametrize("segment_nodes", [16, 0])
def test_many_segments(eight, segment_nodes):
    pg = device_graph(posegraph.fixed_iterations(EIGHT_ITERATIONS, segment_nodes=segment_nodes, max_nodes=3000, max_loops=8, max_unary=4), eight["x0"], eight["loops"])
    info = pg.solve()
    print(info.as_dict())
    got = pg.read_poses()
    eight["got"][segment_nodes] = got
    assert info.segments >= (3000 // 17 if segment_nodes else 40)
    check_poses(got, eight["want"], f"figure of eight / {segment_nodes}")
    check_error(info.final_error, eight["wi"]["final_error"])
    if len(eight["got"]) == 2:
        rel = W.spread(eight["got"][16], eight["got"][0], True)
        print("16 against the library's choice:", rel)
        assert rel[0] <= REL_TOL[0] and rel[1] <= REL_TOL[1], rel
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 6: determinism and increments
def test_determinism_and_increments(circle):
    x0, loops = circle["x0"], [circle["loop"]]
    runs = []
    for chunks in (None, [1, 7, 52]):
        for _ in range(2):
            pg = device_graph(posegraph.default_opts(**SMALL), x0, loops, chunks=chunks)
            info = pg.solve()
            runs.append((pg.read_poses(), info))
            if len(runs) == 1:
                again = pg.solve()                 # nothing new: one iteration finds no decrease
                assert again.iterations == 1 and again.termination == T.PGRAPH_CONVERGED, again.as_dict()
                pg.clear()
                assert pg.size() == 0
                fill(pg, x0, loops)
                pg.solve()
                assert np.array_equal(pg.read_poses().view(np.uint64), runs[0][0].view(np.uint64))
            pg.close()
    assert runs[0][1].termination == T.PGRAPH_CONVERGED and 2 <= runs[0][1].iterations <= 8
    for p, info in runs[1:]:
        assert np.array_equal(p.view(np.uint64), runs[0][0].view(np.uint64))
        assert (info.iterations, info.final_error) == (runs[0][1].iterations, runs[0][1].final_error)


# ------------------------------------------------------------------------------------------------------------------------------------ 7: the local graph
def test_local_graph_and_marginal_covariance():
    truth, x0 = scene(40, 15, radius=40.0, turn=0.6)
    rng = np.random.default_rng(16)
    gps = [(k, truth[k, :3] + rng.normal(0, [1, 1, 2]), GPS_VAR) for k in (4, 11, 18, 25, 32, 39)]
    against_witness(SMALL, x0, gps=gps, what="local graph")
    pg = device_graph(posegraph.default_opts(**SMALL), x0, gps=gps)
    pg.solve()
    x = pg.read_poses()
    cov = pg.marginal_covariance(39)
    want = W.marginal_covariance(witness(x0, gps=gps), x, 39)
    print("covariance: largest entry", np.abs(want).max(), "largest difference", np.abs(cov - want).max())
    assert np.array_equal(cov, cov.T)
    assert np.abs(cov - want).max() <= 1e-8 * np.abs(want).max()
    assert np.array_equal(pg.read_poses(), x)          # asking changes nothing
    pg.close()


def test_marginal_covariance_under_the_prior_alone(circle):
    """Entries (3,3) and (4,4), the ones addGNSSFactor gates on (Estimator.cpp:1938), are about 1e8: the prior's translation variance, reached through a pivot
    that cancellation against the odometry information 1e4 leaves with about four good digits -- hence 1 %, not rounding."""
    pg = device_graph(posegraph.default_opts(**SMALL), circle["x0"], [circle["loop"]])
    pg.solve()
    x = pg.read_poses()
    cov, want = pg.marginal_covariance(59), W.marginal_covariance(circle["g"], x, 59)
    print(cov[3, 3], want[3, 3], cov[4, 4], want[4, 4])
    for k in (3, 4):
        assert want[k, k] > 1e7 and abs(cov[k, k] - want[k, k]) <= 0.01 * want[k, k]
    assert np.array_equal(cov, cov.T)
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 8: limits and refusals
def refused(fn, *a, **kw):
    with pytest.raises(capi.GlioError, match="error -1"):
        fn(*a, **kw)


def test_limits_and_refusals():
    truth, x0 = scene(12, 17)
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=12, max_loops=2, max_unary=1))
    refused(pg.solve)                                   # no node
    pg.append(x0[:6])
    refused(pg.solve)                                   # neither a prior nor a GPS factor
    refused(pg.error)
    pg.set_prior(x0[0])
    pg.add_between(5, 1, W.between(truth[5], truth[1]), LOOP_VAR)
    state = lambda: (pg.size(), pg.error(), pg.read_poses())
    before = state()
    bad_pose, zero_q = x0[6].copy(), x0[6].copy()
    bad_pose[1] = np.nan
    zero_q[3:] = 0
    rel = W.between(truth[4], truth[0])
    seven = np.vstack([x0[6:12], x0[11:12]])
    cases = {"node outside": lambda: pg.add_between(0, 6, rel, LOOP_VAR), "negative node": lambda: pg.add_between(-1, 2, rel, LOOP_VAR),
             "i == j": lambda: pg.add_between(3, 3, rel, LOOP_VAR), "zero variance": lambda: pg.add_between(4, 0, rel, np.r_[LOOP_VAR[:5], 0.0]),
             "negative variance": lambda: pg.add_between(4, 0, rel, np.r_[LOOP_VAR[:5], -1.0]),
             "infinite variance": lambda: pg.add_between(4, 0, rel, np.r_[LOOP_VAR[:5], np.inf]),
             "nan variance": lambda: pg.add_between(4, 0, rel, np.r_[np.nan, LOOP_VAR[:5]]),
             "infinite measurement": lambda: pg.add_between(4, 0, np.r_[np.inf, rel[1:]], LOOP_VAR),
             "gps node outside": lambda: pg.add_gps(6, truth[2, :3], GPS_VAR), "gps nan": lambda: pg.add_gps(2, [0, np.nan, 0], GPS_VAR),
             "gps zero variance": lambda: pg.add_gps(2, truth[2, :3], [1, 0, 1]),
             "nan pose": lambda: pg.append(bad_pose[None]), "zero quaternion": lambda: pg.append(zero_q[None]),
             "nan prev_pose": lambda: pg.append(x0[6:8], prev_pose=bad_pose), "one node too many": lambda: pg.append(seven),
             "odometry variance": lambda: pg.append(x0[6:7], var=[1e-6, 1e-6, 1e-6, 1e-4, 0.0, 1e-4]),
             "nan prior": lambda: pg.set_prior(bad_pose), "prior variance": lambda: pg.set_prior(x0[0], [1, 1, 1, 1, 1, -2.0]),
             "covariance node outside": lambda: pg.marginal_covariance(6), "covariance negative node": lambda: pg.marginal_covariance(-1),
             "read outside": lambda: pg.read_poses(3, 4), "read negative": lambda: pg.read_poses(-1, 2)}
    for name, c in cases.items():
        refused(c)
        after = state()
        assert after[0] == before[0] and after[1] == before[1] and np.array_equal(after[2], before[2]), name
    # the tables exactly filled, then one more
    pg.append(x0[6:12], prev_pose=x0[5])
    assert pg.size() == 12
    refused(pg.append, x0[11:12])
    pg.add_between(11, 0, W.between(truth[11], truth[0]), LOOP_VAR)
    refused(pg.add_between, 10, 2, rel, LOOP_VAR)
    pg.add_gps(7, truth[7, :3], GPS_VAR)
    refused(pg.add_gps, 8, truth[8, :3], GPS_VAR)
    before = state()
    info = pg.solve()
    assert info.termination == T.PGRAPH_CONVERGED and info.final_error < before[1]
    g = witness(x0, [loop_of(truth, 5, 1), loop_of(truth, 11, 0)], [(7, truth[7, :3], GPS_VAR)])
    want, _ = W.gauss_newton(g, x0, solver="cholesky")
    rel_s = W.spread(pg.read_poses(), want, True)
    assert rel_s[0] < 1e-6 and rel_s[1] < 1e-7, rel_s      # both stopped by the same test on the error, not at rounding
    pg.close()
    refused(posegraph.PoseGraph, posegraph.default_opts(max_nodes=0))
    refused(posegraph.PoseGraph, posegraph.default_opts(max_loops=1025))
    refused(posegraph.PoseGraph, posegraph.default_opts(segment_nodes=-1))


def test_a_contradicting_loop_ends_with_a_status():
    truth, x0 = scene(12, 18)
    wrong = W.between(truth[11], truth[1])
    wrong = np.r_[wrong[:3], W.q_mul(wrong[3:], W.so3_exp([0, 0, np.pi / 2]))]
    pg = device_graph(posegraph.default_opts(**SMALL), x0, [(11, 1, wrong, np.full(6, 1e-12))])
    p0 = pg.read_poses()
    info = pg.solve()
    print(info.as_dict())
    assert info.termination in (T.PGRAPH_CONVERGED, T.PGRAPH_ITERATION_LIMIT, T.PGRAPH_NONPOSITIVE_PIVOT)
    p = pg.read_poses()
    assert np.isfinite(p).all() and np.abs(np.linalg.norm(p[:, 3:], axis=1) - 1).max() < 1e-12
    if info.termination == T.PGRAPH_NONPOSITIVE_PIVOT:
        assert np.array_equal(p, p0)
    pg.close()

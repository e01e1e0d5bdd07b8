"""GPU: glio_pgraph_covariance_all (include/glio_pgraph_cov.h, csrc/posegraph_kernels.hip) -- block (i, i) and (i, i + 1) of (J^T J)^-1 for every node of the
pose graph from one factorisation -- against np.linalg.inv of the witness's J^T J (tests/pose_graph_restated.py) at the poses read back from the device.

The gate.  Per block, the error relative to the largest entry of the diagonal blocks involved must stay within max(1e-9, 100 x floor), where the floor is
what the numpy restatement of the same block algorithm (tests/pose_graph_cov_restated.py) is away from that same dense inverse on that case (1.5e-11 ..
1.1e-10 at cond(H) = 1e8 .. 3e9, 1.5e-7 with 90 nested loops at cond(H) = 1e11): two decimal digits over the distance between two fp64 computations of the same blocks.  The 60-node circle under the
prior alone (cond(H) = 4e16, floor 3e-3) is not held to that gate: as in test_hip_pose_graph.py only the entries addGNSSFactor gates on are, to 1 %."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cov_restated as R
import pose_graph_restated as W
from glio_amd import capi, posegraph
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu

SCENES = R.scenes()
CASES = [(name, s) for name, sc in SCENES.items() for s in sc["segment_nodes"]]
SENTINEL = -7.25


def device_graph(sc, segment_nodes, opts=None, **kw):
    x0 = sc["x0"]
    o = opts or posegraph.default_opts(max_nodes=max(len(x0), 4), max_loops=max(8, len(sc["loops"])), max_unary=16, segment_nodes=segment_nodes, **kw)
    pg = posegraph.PoseGraph(o)
    pg.set_prior(x0[0])
    pg.append(x0)
    for lp in sc["loops"]:
        pg.add_between(*lp)
    for gp in sc["gps"]:
        pg.add_gps(*gp)
    return pg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def solved():
    """(name, segment_nodes) -> dict(pg: the solved device graph, x, want: the dense inverse's blocks at x, plan, gate, pivots): made once per case"""
    cache = {}

    def get(name, s):
        if (name, s) not in cache:
            sc = SCENES[name]
            pg = device_graph(sc, s)
            pg.solve()
            x = pg.read_poses()
            H = R.normal_matrix(R.witness(sc), x)
            want = R.dense_blocks(H)
            plan = R.make_plan(len(x), sc["loops"], s)
            rd, rn, piv = R.covariance_all(H, plan)
            floor = max(R.block_errors(rd, rn, *want))
            cache[(name, s)] = dict(pg=pg, x=x, want=want, plan=plan, floor=floor, gate=max(1e-9, 100 * floor), pivots=piv)
        return cache[(name, s)]
    yield get
    for c in cache.values():
        c["pg"].close()


# ------------------------------------------------------------------------------------------------------------------------------------ 1: the numbers
@pytest.mark.parametrize("name,segment_nodes", CASES)
def test_against_the_dense_inverse(solved, name, segment_nodes):
    c = solved(name, segment_nodes)
    diag, nxt, info = c["pg"].marginal_covariances(next=True, with_info=True)
    ed, en = R.block_errors(diag, nxt, *c["want"])
    print(f"{name} / {segment_nodes}: floor {c['floor']:.2e} gate {c['gate']:.2e} device diag {ed:.2e} next {en:.2e} {info}")
    assert diag.shape == (len(c["x"]), 6, 6) and nxt.shape == (len(c["x"]) - 1, 6, 6)
    assert ed <= c["gate"] and en <= c["gate"], (ed, en, c["gate"])
    assert all(np.array_equal(d, d.T) for d in diag)
    plan = c["plan"]
    assert (info["n_nodes"], info["separators"], info["full_row_separators"], info["segment_nodes"], info["bad_node"]) == \
        (len(c["x"]), len(plan["sep"]), len(plan["w_blk"]), segment_nodes, -1)
    # the factor's squared diagonal: the restatement factors the same matrix in the same order (1e-6: cond(H) x rounding, relative to the pivot itself)
    assert abs(info["min_pivot"] - c["pivots"]["min_pivot"]) <= 1e-6 * c["pivots"]["min_pivot"]
    assert abs(info["max_pivot"] - c["pivots"]["max_pivot"]) <= 1e-6 * c["pivots"]["max_pivot"]


def test_one_node_has_the_priors_variance(solved):
    diag = solved("one_node", 4)["pg"].marginal_covariances()
    # the diagonal to 1e-12 of itself; the rest (zero but for the rounding of the node's own quaternion) to 1e-12 of the two variances it couples
    assert diag.shape == (1, 6, 6) and np.all(np.abs(diag[0] - np.diag(W.PRIOR_VAR)) <= 1e-12 * np.sqrt(np.outer(W.PRIOR_VAR, W.PRIOR_VAR)))


@pytest.mark.parametrize("name,segment_nodes", [c for c in CASES if c[0] in ("local_gps", "gps_loops")])
def test_consistent_with_the_per_node_call(solved, name, segment_nodes):
    """the per-node call makes the node a separator: another plan, so the same to the gate and not to the bit"""
    c = solved(name, segment_nodes)
    diag = c["pg"].marginal_covariances()
    worst = 0.0
    for i in range(len(diag)):
        one = c["pg"].marginal_covariance(i)
        worst = max(worst, np.abs(diag[i] - one).max() / np.abs(one).max())
    print(f"{name} / {segment_nodes}: against the per-node call {worst:.2e} (gate {c['gate']:.2e})")
    assert worst <= c["gate"]


def test_the_circle_under_the_prior_alone():
    x0, loop, g = W.circle_scene()
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=64, max_loops=8, max_unary=16))
    pg.set_prior(x0[0]); pg.append(x0); pg.add_between(*loop)
    pg.solve()
    x = pg.read_poses()
    want = R.dense_blocks(R.normal_matrix(g, x))[0]
    diag = pg.marginal_covariances()
    for i in (0, 30, 59):
        print(i, diag[i][3, 3], want[i][3, 3], diag[i][4, 4], want[i][4, 4])
        for k in (3, 4):
            assert want[i][k, k] > 1e7 and abs(diag[i][k, k] - want[i][k, k]) <= 0.01 * want[i][k, k]
    assert all(np.array_equal(d, d.T) for d in diag)
    pg.close()


# ------------------------------------------------------------------------------------------------------------------------------------ 2: bits and side effects
def test_bits_and_no_side_effect():
    sc = SCENES["gps_loops"]
    seq = lambda pg: (bits(pg.read_poses()), pg.solve().final_error, bits(pg.read_poses()), pg.solve_damped().final_error, bits(pg.read_poses()),
                      bits(pg.marginal_covariance(7)), pg.error())
    a, b = device_graph(sc, 5), device_graph(sc, 5)
    p0 = a.read_poses()
    d1, n1 = a.marginal_covariances(next=True)
    d2, n2 = a.marginal_covariances(next=True)
    d3 = a.marginal_covariances()
    assert np.array_equal(bits(d1), bits(d2)) and np.array_equal(bits(n1), bits(n2)) and np.array_equal(bits(d1), bits(d3))
    assert np.array_equal(bits(a.read_poses()), bits(p0))
    with_call, without = seq(a), seq(b)
    for u, v in zip(with_call, without):
        assert np.array_equal(u, v)
    # between the entry points of a solved graph, too
    d4 = a.marginal_covariances()
    assert np.array_equal(bits(a.marginal_covariance(7)), without[5]) and a.error() == without[6]
    assert np.array_equal(bits(b.marginal_covariances()), bits(d4))
    a.close(); b.close()


def test_after_a_rejected_trial_the_call_linearises_again():
    """a drive on which the undamped step raises the error: one trial at the largest radius is rejected, the estimate stays, and the tables hold the
    linearisation at the rejected candidate.  The covariance must be the one of a fresh graph at the same poses."""
    F = 157
    truth = W.circle_truth(F)
    sc = dict(x0=W.noisy_odometry(truth, np.random.default_rng(1), 5e-2, 3e-2), gps=[],
              loops=[(148, 0, W.between(truth[148], truth[0]), np.full(6, 0.09))])
    a, b = device_graph(sc, 0), device_graph(sc, 0)
    info = a.solve_damped(posegraph.default_lm_opts(initial_radius=1e16, max_trials=1))
    assert (info.accepted, info.rejected, info.trials) == (0, 1, 1), info.as_dict()
    assert np.array_equal(bits(a.read_poses()), bits(b.read_poses()))
    da, na = a.marginal_covariances(next=True)
    db, nb = b.marginal_covariances(next=True)
    assert np.array_equal(bits(da), bits(db)) and np.array_equal(bits(na), bits(nb))
    a.close(); b.close()


def _hip():
    """the HIP runtime this process already runs on"""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def test_device_pointers_and_times(solved):
    pg = solved("gps_loops", 2)["pg"]
    diag, nxt = pg.marginal_covariances(next=True)
    pd, pn, n = pg.marginal_covariances_dev()
    assert n == 40 and pd and pn
    hip = _hip()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    gd, gn = np.zeros_like(diag), np.zeros_like(nxt)
    assert hip.hipMemcpy(gd.ctypes.data, pd, gd.nbytes, 2) == 0 and hip.hipMemcpy(gn.ctypes.data, pn, gn.nbytes, 2) == 0
    assert np.array_equal(bits(gd), bits(diag)) and np.array_equal(bits(gn), bits(nxt))
    ms, stages = pg.marginal_covariances_ms()
    print("device ms", ms, stages)
    assert ms > 0 and len(stages) == 5 and all(np.isfinite(s) and s >= 0 for s in stages) and sum(stages) <= ms * 1.001 + 1e-3


# ------------------------------------------------------------------------------------------------------------------------------------ 3: refusals
def test_refusals_leave_everything_alone():
    lib = capi.load()
    sc = SCENES["local_gps"]
    diag, nxt = np.full((40, 6, 6), SENTINEL), np.full((39, 6, 6), SENTINEL)
    untouched = lambda: bool((diag == SENTINEL).all() and (nxt == SENTINEL).all())
    info = T.GlioPgraphCovInfo()
    assert lib.glio_pgraph_covariance_all(None, T.dptr(diag), T.dptr(nxt), C.byref(info)) == capi.E_ARG and untouched()
    ms = C.c_float(0)
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=64, max_loops=8, max_unary=16, segment_nodes=4))
    assert lib.glio_pgraph_covariance_all_last_device_ms(pg._h, C.byref(ms)) == capi.E_STATE
    assert lib.glio_pgraph_covariance_all_last_stage_ms(pg._h, (C.c_float * 5)()) == capi.E_STATE
    # an empty graph; nodes without a prior or a GPS factor
    assert lib.glio_pgraph_covariance_all(pg._h, T.dptr(diag), T.dptr(nxt), C.byref(info)) == capi.E_ARG and untouched()
    with pytest.raises(capi.GlioError, match="error -1"):
        pg.marginal_covariances()
    pg.append(sc["x0"])
    assert lib.glio_pgraph_covariance_all(pg._h, T.dptr(diag), T.dptr(nxt), C.byref(info)) == capi.E_ARG and untouched()
    pg.set_prior(sc["x0"][0])
    for gp in sc["gps"]:
        pg.add_gps(*gp)
    state = lambda: (pg.size(), pg.error(), bits(pg.read_poses()), bits(pg.marginal_covariance(39)))
    before = state()
    assert lib.glio_pgraph_covariance_all(pg._h, None, T.dptr(nxt), C.byref(info)) == capi.E_ARG and untouched()
    assert lib.glio_pgraph_covariance_all_dev(pg._h, None, None, None) == capi.E_ARG
    assert lib.glio_pgraph_covariance_all_dev(None, None, None, None) == capi.E_ARG
    after = state()
    assert all(np.array_equal(u, v) for u, v in zip(before, after))
    # and with everything in place the same arrays are filled; info may be null
    assert lib.glio_pgraph_covariance_all(pg._h, T.dptr(diag), T.dptr(nxt), None) == 0
    assert not (diag == SENTINEL).any() and not (nxt == SENTINEL).any()
    assert np.array_equal(bits(diag), bits(pg.marginal_covariances()))
    pg.close()


def test_a_contradicting_loop_is_refused_with_its_node():
    """the scene of test_a_contradicting_loop_ends_with_a_status reaches a pivot of the separator system that is not positive, at the loop's later end: the
    call names that NODE (11; its separator is number 3), hands nothing over, and leaves every other entry point what a twin graph without the call gives"""
    truth, x0 = R.arc(12, 18, radius=20.0, turn=0.98)
    wrong = W.between(truth[11], truth[1])
    wrong = np.r_[wrong[:3], W.q_mul(wrong[3:], W.so3_exp([0, 0, np.pi / 2]))]
    sc = dict(x0=x0, loops=[(11, 1, wrong, np.full(6, 1e-12))], gps=[])
    pg, twin = device_graph(sc, 0), device_graph(sc, 0)
    pg.solve(); twin.solve()
    x = pg.read_poses()
    diag, nxt = np.full((12, 6, 6), SENTINEL), np.full((11, 6, 6), SENTINEL)
    info = T.GlioPgraphCovInfo()
    rc = capi.load().glio_pgraph_covariance_all(pg._h, T.dptr(diag), T.dptr(nxt), C.byref(info))
    print("rc", rc, info.as_dict())
    assert rc == capi.E_NUMERIC and info.bad_node == 11
    assert (info.n_nodes, info.separators, info.full_row_separators, info.segment_nodes) == (12, 4, 1, 4)
    assert (diag == SENTINEL).all() and (nxt == SENTINEL).all()
    with pytest.raises(capi.GlioError, match="error -4") as e:
        pg.marginal_covariances(next=True)
    assert e.value.code == capi.E_NUMERIC and e.value.info["bad_node"] == 11
    assert capi.load().glio_pgraph_covariance_all_dev(pg._h, C.byref(C.c_void_p()), None, None) == capi.E_NUMERIC
    # nothing another entry point reads has changed
    assert np.array_equal(bits(pg.read_poses()), bits(x)) and np.array_equal(bits(twin.read_poses()), bits(x))
    assert pg.error() == twin.error()
    a, b = pg.solve(), twin.solve()
    assert (a.iterations, a.termination, a.initial_error, a.final_error) == (b.iterations, b.termination, b.initial_error, b.final_error)
    assert np.array_equal(bits(pg.read_poses()), bits(twin.read_poses()))
    pg.close(); twin.close()


def test_a_pivot_that_is_not_finite_inside_a_segment_names_its_node():
    """odometry variances of 1e-308 from node 6 on are positive and finite, so the graph takes them; the information 1e308 of the two edges at node 6 sums to
    infinity in its diagonal block.  With segment_nodes = 4 the separators are 0, 5, 10, 11: node 6 is the first interior node of the second segment, the
    first pivot block in elimination order that is not finite."""
    _, x0 = R.arc(12, 18, radius=20.0, turn=0.98)
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=12, max_loops=1, max_unary=1, segment_nodes=4))
    pg.set_prior(x0[0])
    pg.append(x0[:6])
    pg.append(x0[6:], prev_pose=x0[5], var=np.full(6, 1e-308))
    x = pg.read_poses()
    diag, nxt = np.full((12, 6, 6), SENTINEL), np.full((11, 6, 6), SENTINEL)
    info = T.GlioPgraphCovInfo()
    rc = capi.load().glio_pgraph_covariance_all(pg._h, T.dptr(diag), T.dptr(nxt), C.byref(info))
    print("rc", rc, info.as_dict())
    assert rc == capi.E_NUMERIC and info.bad_node == 6 and info.separators == 4
    assert (diag == SENTINEL).all() and (nxt == SENTINEL).all()
    assert np.array_equal(bits(pg.read_poses()), bits(x))
    pg.close()

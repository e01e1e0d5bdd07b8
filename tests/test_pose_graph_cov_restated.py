"""CPU: tests/pose_graph_cov_restated.py -- the block algorithm of glio_pgraph_covariance_all in numpy -- against np.linalg.inv(J^T J) on the scenes the GPU
test uses, on every plan shape, and with one deliberate mistake at a time.

The bound.  Both sides invert the same H in fp64; the forward error of an inverse is of the order cond(H) * 2^-52 relative to its norm, so that product (no
further factor) is what the restatement is held to per block: 2.7e-8 at cond(H) = 1.2e8.  (Measured: 1.5e-11 .. 1.1e-10 on these scenes, 9e-8 with 90 nested loops at cond(H) = 1e11, where the bound is 2.4e-5.)  A wrong
recurrence is off by the size of the blocks themselves."""
import os

import numpy as np
import pytest

import pose_graph_cov_restated as R
import pose_graph_restated as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = R.scenes()
CASES = [(name, s) for name, sc in SCENES.items() for s in sc["segment_nodes"]]


@pytest.fixture(scope="module")
def dense():
    """name -> (H at the witness's estimate, its dense inverse's blocks, cond(H)): computed once"""
    out = {}
    for name, sc in SCENES.items():
        g = R.witness(sc)
        x = W.gauss_newton(g, sc["x0"], max_iterations=3, fixed=True)[0] if len(sc["x0"]) <= 40 else sc["x0"]
        H = R.normal_matrix(g, x)
        out[name] = (H, R.dense_blocks(H), float(np.linalg.cond(H)))
    return out


def accepted(diag, nxt, want, cond):
    ed, en = R.block_errors(diag, nxt, *want)
    return max(ed, en) <= cond * 2.0 ** -52, (ed, en)


@pytest.mark.parametrize("name,segment_nodes", CASES)
def test_restatement_against_the_dense_inverse(dense, name, segment_nodes):
    H, want, cond = dense[name]
    plan = R.make_plan(H.shape[0] // 6, SCENES[name]["loops"], segment_nodes)
    diag, nxt, info = R.covariance_all(H, plan)
    ok, err = accepted(diag, nxt, want, cond)
    print(f"{name} / {segment_nodes}: separators {len(plan['sep'])}, full rows {plan['w_blk']}, cond {cond:.1e}, floor diag {err[0]:.1e} next {err[1]:.1e}")
    assert np.isfinite(diag).all() and np.isfinite(nxt).all()          # Z starts as NaN: nothing outside the pattern was read
    assert ok, err
    assert all(np.array_equal(d, d.T) for d in diag)
    assert 0 < info["min_pivot"] <= info["max_pivot"]


def test_every_plan_shape():
    plan = lambda name, s: R.make_plan(len(SCENES[name]["x0"]), SCENES[name]["loops"], s)
    gaps = lambda p: set(np.diff(p["sep"]) - 1)
    live = lambda p, b: sum(1 for w, lo in zip(p["w_blk"], p["w_lo"]) if w >= b + 2 and lo <= b)
    # no full row without a loop; segments of exactly segment_nodes interior nodes and a shorter last one
    p = plan("local_gps", 7)
    assert p["sep"] == [0, 8, 16, 24, 32, 39] and not p["w_blk"] and gaps(p) == {7, 6}
    assert gaps(plan("local_gps", 1)) == {1, 0}
    # nested loops: every later end keeps a full row, and two (here three) of them are live at once between the inner loop's ends
    for s in (2, 5):
        p = plan("gps_loops", s)
        assert [p["sep"][w] for w in p["w_blk"]] == [22, 30, 39] and [p["sep"][k] for k in p["w_lo"]] == [13, 10, 3]
        assert max(live(p, b) for b in range(len(p["sep"]))) >= 2
    assert 0 in gaps(plan("neighbour_loop", 4)) and plan("neighbour_loop", 4)["sep"][3:5] == [11, 12]
    assert 1 in gaps(plan("one_interior", 4)) and 13 not in plan("one_interior", 4)["sep"]
    assert plan("two_nodes", 4)["sep"] == [0, 1] and plan("one_node", 4)["sep"] == [0]
    assert plan("long_segment", 255)["sep"] == [0, 256, 299]
    assert R.default_segment_nodes(700) == 26 and R.default_segment_nodes(3500) == 59 and R.default_segment_nodes(65536) == 255 and R.default_segment_nodes(9) == 4


def test_one_node_has_the_priors_variance(dense):
    H, want, _ = dense["one_node"]
    diag, nxt, _ = R.covariance_all(H, R.make_plan(1, [], 4))
    assert nxt.shape == (0, 6, 6) and np.allclose(diag[0], np.diag(W.PRIOR_VAR), rtol=1e-12, atol=0)


@pytest.mark.parametrize("wrong", ["no_spike", "sign", "outside_zero"])
def test_a_wrong_restatement_is_refused(dense, wrong):
    H, want, cond = dense["gps_loops"]
    plan = R.make_plan(40, SCENES["gps_loops"]["loops"], 5)
    ok, err = accepted(*R.covariance_all(H, plan, wrong)[:2], want, cond)
    print(wrong, err)
    assert not ok and min(err) > 1e-3, err
    assert accepted(*R.covariance_all(H, plan)[:2], want, cond)[0]


def test_the_circle_under_the_prior_alone():
    """cond(H) = 4e16: no digit is promised, but entries (3,3) and (4,4) -- the ones addGNSSFactor gates on -- are the prior's 1e8 to 1 %"""
    x0, loop, g = W.circle_scene()
    x = W.gauss_newton(g, x0, max_iterations=10, fixed=True)[0]
    H = R.normal_matrix(g, x)
    want = R.dense_blocks(H)[0]
    diag = R.covariance_all(H, R.make_plan(60, [loop], 0))[0]
    for i in (0, 30, 59):
        for k in (3, 4):
            assert want[i][k, k] > 1e7 and abs(diag[i][k, k] - want[i][k, k]) <= 0.01 * want[i][k, k], (i, k, diag[i][k, k], want[i][k, k])


def test_the_restatement_and_the_product_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "pose_graph_cov_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "oracle" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "pose_graph_cov_restated" not in open(os.path.join(dirpath, f)).read(), f

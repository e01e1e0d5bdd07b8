"""The numpy restatement of the loop-closure registration (tests/loop_restated.py) against answers known on paper: the known-answer case (an exact
subset of the target, moved by a small known motion), the ends of the loop (no correspondences, the iteration limit, the fitness gate, collinear
pairs), and the claim the device code rests on -- the float-rounded transform does not depend on the order of the fp64 sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_restated as lr  # noqa: E402
from glio_amd import loop  # noqa: E402


@pytest.fixture(scope="module")
def known():
    return lr.known_answer_case()


def _same(a, b):
    return np.array_equal(a["transform"].view(np.uint32), b["transform"].view(np.uint32)) and (a["iterations"], a["state"]) == (b["iterations"], b["state"])


def test_pieces_on_paper():
    # 1-NN: float32 d2, ties to the lowest index
    tgt = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 5, 0, 0]], np.float32)
    idx, d2 = lr.nn_brute(np.array([[1, 0, 0, 0], [0.25, 0, 0, 0], [1, 4, 0, 0]], np.float32), tgt)
    assert list(idx) == [0, 1, 3] and list(d2) == [1.0, 0.0625, 1.0]
    idx, _ = lr.correspondences(np.array([[1, 0, 0, 0], [2, 36, 0, 0]], np.float32), tgt, 30.0)
    assert list(idx) == [0, -1]
    # Umeyama: an exact rotation about z plus a shift is recovered; a reflected cloud still gives a rotation (det +1)
    rng = np.random.default_rng(1)
    s = np.c_[rng.uniform(-5, 5, (200, 3)), np.zeros(200)].astype(np.float32)
    M = lr.known_motion(0.3, -0.1, 0.05, (1.0, 2.0, -0.5))
    t = s.copy(); t[:, :3] = (s[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    T = lr.fit_rigid(s, t)
    dt, dr = lr.pose_error(T, M)
    assert dt < 2e-5 and dr < 2e-6
    mirror = s.copy(); mirror[:, 2] *= -1.0
    Tm = lr.fit_rigid(s, mirror)
    assert abs(np.linalg.det(Tm[:3, :3].astype(np.float64)) - 1.0) < 1e-5
    # collinear pairs determine no rotation
    line = np.zeros((20, 4), np.float32); line[:, 0] = np.arange(20)
    assert lr.fit_rigid(line, line) is None
    # float application and composition: the stated operation order
    T = np.array([[0.5, 0.25, 0.125, 1.0], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]], np.float32)
    p = np.array([[2.0, 4.0, 8.0, 7.0]], np.float32)
    assert list(lr.apply_T(T, p)[0]) == [4.0, 6.0, 11.0, 7.0]
    assert np.array_equal(lr.compose(T, np.eye(4, dtype=np.float32)), T)
    # the convergence test, in its order
    I = np.eye(4, dtype=np.float32)
    o = lr.DEFAULTS
    assert lr.convergence_state(I, 100, 1.0, 2.0, o) == lr.ITERATIONS
    assert lr.convergence_state(I, 3, 1.0, 2.0, o) == lr.TRANSFORM
    far = I.copy(); far[0, 3] = 0.5
    assert lr.convergence_state(far, 3, 1.0, 1.0 + 1e-13, o) == lr.ABS_MSE
    assert lr.convergence_state(far, 3, 1.0, 1.0 + 1e-8, o) == lr.REL_MSE
    assert lr.convergence_state(far, 3, 1.0, lr.DBL_MAX, o) == lr.NOT_CONVERGED


def test_accelerated_search_is_the_brute_force_search(known):
    src, tgt, _ = known
    a, b = lr.nn_brute(src, tgt), lr.nn_exact(src, tgt, lr.make_tree(tgt))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    rng = np.random.default_rng(2)                      # a lattice: more exact ties than candidates
    tgt = np.c_[rng.integers(-3, 4, (4000, 3)), np.zeros(4000)].astype(np.float32)
    src = (np.c_[rng.integers(-4, 5, (500, 3)), np.zeros(500)] + np.array([0.5, 0.5, 0.5, 0])).astype(np.float32)
    a, b = lr.nn_brute(src, tgt), lr.nn_exact(src, tgt, lr.make_tree(tgt))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("seed", [20261017, 20261019, 20261020])
def test_known_answer(seed):
    """~10 k target points, the source an exact subset within 15 m moved by yaw 0.03 / pitch 0.01 / roll -0.005 about the centre plus (0.5, -0.3, 0.1):
    ends TRANSFORM after 12-13 rounds with a fitness of ~1.7e-10 m^2 and the known motion inside the project's pose gates (1e-4 m, 1e-5 rad)."""
    src, tgt, known_T = lr.known_answer_case(seed)
    assert 9000 < len(tgt) < 11500 and 3000 < len(src) < 4500
    r = lr.icp(src, tgt)
    dt, dr = lr.pose_error(r["transform"], known_T)
    print(f"seed {seed}: {r['iterations']} rounds, state {r['state']}, fitness {r['fitness']:.3e}, |dt| {dt:.3e} m, |dR| {dr:.3e} rad")
    assert r["converged"] and r["state"] == lr.TRANSFORM and 5 <= r["iterations"] <= 30
    assert dt < 1e-4 and dr < 1e-5
    assert r["fitness"] < 1e-8 and r["last_n_corr"] == len(src)
    assert _same(r, lr.icp(src, tgt, reverse=True))                      # the order of the fp64 sums does not reach the float transform
    con = loop.loop_constraint(loop.LoopResult(_as_struct(r)), np.r_[0, 0, 0, 1, 0, 0, 0.0], np.r_[1, 0, 0, 1, 0, 0, 0.0], 0.3)
    assert con is not None and np.all(con[1] == r["fitness"])


def _as_struct(r):
    from glio_amd import ctypes_types as T
    s = T.GlioLoopResult()
    s.converged, s.state, s.iterations, s.fitness, s.last_mse, s.last_n_corr = int(r["converged"]), r["state"], r["iterations"], r["fitness"], r["last_mse"], r["last_n_corr"]
    for k, v in enumerate(np.asarray(r["transform"], np.float32).ravel()):
        s.transform[k] = float(v)
    return s


def test_ends(known):
    src, tgt, _ = known
    away = src.copy(); away[:, 2] += 100.0
    r = lr.icp(away, tgt)
    assert (r["converged"], r["state"], r["iterations"]) == (False, lr.NO_CORRESPONDENCES, 0) and np.array_equal(r["transform"], np.eye(4, dtype=np.float32))
    assert r["fitness"] > 80.0 ** 2                                          # getFitnessScore has no distance cap
    assert _same(r, lr.icp(away, tgt, reverse=True))
    r = lr.icp(src, tgt, max_iterations=2)
    assert (r["converged"], r["state"], r["iterations"]) == (True, lr.ITERATIONS, 2)
    assert _same(r, lr.icp(src, tgt, max_iterations=2, reverse=True))
    # the fitness gate of :5210: converged, but the fitness after two rounds is far above what a closed loop shows
    assert r["fitness"] > 1e-6
    st = _as_struct(r)
    res = loop.LoopResult(st)
    assert loop.loop_constraint(res, np.r_[0, 0, 0, 1, 0, 0, 0.0], np.r_[0, 0, 0, 1, 0, 0, 0.0], r["fitness"] * 0.5) is None
    assert loop.loop_constraint(res, np.r_[0, 0, 0, 1, 0, 0, 0.0], np.r_[0, 0, 0, 1, 0, 0, 0.0], r["fitness"] * 2.0) is not None
    line = np.zeros((50, 4), np.float32); line[:, 0] = np.arange(50)
    r = lr.icp(line + np.array([0.25, 0, 0, 0], np.float32), line)
    assert r["rank_deficient"] and not r["converged"] and r["state"] == lr.NOT_CONVERGED and r["iterations"] == 0


def test_summation_order_does_not_reach_the_float_transform_on_the_independent_pair():
    """the ~9 k / ~33 k independently sampled pair the GPU test aligns: forward and reversed fp64 sums give the same float transform, rounds and state"""
    src, tgt = lr.independent_pair()
    assert 8000 < len(src) < 10500 and 30000 < len(tgt) < 36000
    a, b = lr.icp(src, tgt), lr.icp(src, tgt, reverse=True)
    print(f"independent pair: {a['iterations']} rounds, state {a['state']}, fitness {a['fitness']:.4f}")
    assert a["converged"] and _same(a, b)

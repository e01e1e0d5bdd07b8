"""CPU: the numpy restatement of the every-frame trajectory (tests/trajectory_restated.py) held to the reference's own functor, to central differences and
to known answers, and the shared case builder's margins."""
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

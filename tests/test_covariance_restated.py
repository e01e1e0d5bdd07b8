"""CPU: the numpy restatement of the covariance (tests/covariance_restated.py) against np.linalg.inv of the oracle's H on synthetic windows and against the
closed-form inverse of the SPD family, the conditioning the GPU tests rely on (tests/golden/covariance_cases.json), and pose3_covariance against finite
differences of the two retractions.

W = 2 without prior and without GNSS is left out on purpose: 12 LiDAR + 15 IMU rows for 30 unknowns, H is singular and has no inverse to compare with."""
import numpy as np
import pytest

import covariance_cases as cases
import covariance_restated as restated
from glio_amd import sliding, synth

EPS = np.finfo(np.float64).eps
WINDOWS = [(W, g, p) for W in (2, 5, 20) for g in (False, True) for p in (False, True) if (W, g, p) != (2, False, False)]


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


@pytest.mark.parametrize("W,gnss,prior", WINDOWS, ids=[f"W{W}{'-gnss' if g else ''}{'-prior' if p else ''}" for W, g, p in WINDOWS])
def test_restatement_against_numpy_on_oracle_windows(po, W, gnss, prior):
    win = synth.make_window(W=W, pts_per_scan=128, with_gnss=gnss, with_prior=prior, seed=synth.SEED_BASE + 710 + W)
    corr = synth.analytic_correspondences(win)
    st = win.init.copy()
    if not gnss:
        st.n_ddt = 0
    H = po.Problem(win, corr, use_gnss=gnss, use_prior=prior).linearize(st)[0]
    n = len(H)
    assert n == 15 * W + st.n_ddt
    full, info = restated.covariance_columns(H, np.arange(n))
    assert info["bad_pivot"] == -1 and info["n_free"] == 0 and np.array_equal(full, full.T)
    cases.assert_within_bound(full, H, f"W {W}")
    cols = np.random.default_rng(W).permutation(n)[:max(1, n // 3)]
    sub, _ = restated.covariance_columns(H, cols)
    cases.assert_within_bound(sub, H, f"W {W} scattered", cols=cols)          # (numpy's sums are not ordered: the bits are the device's promise, not this one's)
    newest, _ = restated.covariance_columns(H, np.arange(15 * (W - 1), 15 * W))
    cases.assert_within_bound(newest, H, f"W {W} newest", cols=np.arange(15 * (W - 1), 15 * W))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_gpu_cases_are_well_conditioned(po, name):
    """what tests/test_hip_covariance.py needs of its windows, checked where no GPU is needed: 8 n kappa_s eps < 1e-6 on the oracle's H, kappa_s as recorded"""
    win, corr, kw, st = cases.build(name)
    H = po.Problem(win, corr, **kw).linearize(st)[0]
    kappa, d = cases.jacobi_kappa(H)
    rec = cases.golden()[name]
    assert (len(H), int((d == 0).sum())) == (rec["n"], rec["n_free"])
    assert abs(kappa - rec["kappa_s"]) <= 1e-6 * kappa and 8 * len(H) * kappa * EPS < 1e-6
    got, info = restated.covariance_columns(H, np.arange(len(H)))
    assert info["n_free"] == rec["n_free"] == info["n_free_asked"]
    cases.assert_within_bound(got, H, name)
    free = np.flatnonzero(d == 0)
    assert np.all(np.diag(got)[free] == np.inf) and not np.isinf(got).sum() > len(free)


@pytest.mark.parametrize("n,kappa", [(1, 10.0), (17, 10.0), (75, 10.0), (75, 1e8), (75, 1e12), (200, 1e8)])
def test_restatement_against_the_closed_form(n, kappa):
    A, d, Q, lam = restated.spd_family(n, kappa, seed=n + int(np.log10(kappa)))
    got, info = restated.covariance_columns(A, np.arange(n))
    err = restated.scaled_error(got, restated.family_scaled_inverse(Q, lam), d)
    assert info["bad_pivot"] == -1 and err <= 4 * n * kappa * EPS, (n, kappa, err)


def test_restatement_free_columns_and_bad_pivots():
    A, d, Q, lam = restated.spd_family(12, 10.0, seed=3)
    B = np.zeros((15, 15))
    keep = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 14]
    B[np.ix_(keep, keep)] = A
    got, info = restated.covariance_columns(B, [3, 0, 14, 7])
    assert info["n_free"] == 3 and info["n_free_asked"] == 2 and info["bad_pivot"] == -1
    assert got[0, 0] == np.inf and got[3, 3] == np.inf and not got[0, 1:].any() and not got[3, :3].any()
    small, _ = restated.covariance_columns(A, [0, 11])
    assert np.allclose(got[np.ix_([1, 2], [1, 2])], small, rtol=1e-12, atol=0)
    B[5, 5] = -1.0
    none, info = restated.covariance_columns(B, [0])
    assert none is None and info["bad_pivot"] == 5


def test_pose3_covariance_against_finite_differences():
    """A (dt, d) -> (omega, v) is the Jacobian at zero of pose3_local(q, t, window_plus(q, t, dt, d)): central differences, step 1e-6, error O(h^2)"""
    rng = np.random.default_rng(11)
    for _ in range(4):
        q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
        t = rng.normal(0, 5, 3)
        J = np.zeros((6, 6))
        h = 1e-6
        for k in range(6):
            e = np.zeros(6); e[k] = h
            qp, tp = restated.window_plus(q, t, e[:3], e[3:])
            qm, tm = restated.window_plus(q, t, -e[:3], -e[3:])
            J[:, k] = (restated.pose3_local(q, t, qp, tp) - restated.pose3_local(q, t, qm, tm)) / (2 * h)
        M = rng.normal(0, 1, (6, 6))
        S = M @ M.T
        got = sliding.pose3_covariance(S, q)
        assert np.array_equal(got, got.T)
        assert np.abs(got - J @ S @ J.T).max() <= 1e-8 * np.abs(got).max()
        # rotation first: a covariance that only moves the translation lands in the lower right block
        only_t = np.zeros((6, 6)); only_t[:3, :3] = np.eye(3)
        g = sliding.pose3_covariance(only_t, q)
        assert np.abs(g[:3, :3]).max() == 0 and np.abs(g[3:, 3:] - np.eye(3)).max() <= 1e-15

"""The synthetic windows the covariance tests share (CPU: the oracle's H; GPU: the device's), each with the factor set it is loaded with.  Small scans
(64-128 points) and plane correspondences from the known scene: building one costs milliseconds.

W = 2 with LiDAR and one IMU edge alone has 12 + 15 = 27 residual rows for 30 unknowns: H is singular whatever the seed, so that window carries the
synthetic marginalization prior as well (speed/bias of slot 0 and the pose of slot 0: 15 more rows).  The other windows are positive definite as listed."""
import json
import os

import numpy as np

from glio_amd import synth

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covariance_cases.json")

# name: (make_window arguments, load_window arguments)
CASES = {
    "w2_lidar_imu": (dict(W=2, pts_per_scan=128, with_prior=True, seed=synth.SEED_BASE + 701), dict(use_gnss=False, use_prior=True)),
    "w3_gnss": (dict(W=3, pts_per_scan=128, with_gnss=True, seed=synth.SEED_BASE + 702), dict(use_gnss=True, use_prior=False)),
    "w20_gnss_prior": (dict(W=20, pts_per_scan=128, with_gnss=True, with_prior=True, seed=synth.SEED_BASE + 704), dict(use_gnss=True, use_prior=True)),
    "w61_gnss": (dict(W=61, pts_per_scan=64, with_gnss=True, seed=synth.SEED_BASE + 705, gnss_epoch_dt=0.4 * 60 / 13), dict(use_gnss=True, use_prior=False)),
    "w1_front_end": (dict(W=1, pts_per_scan=128, seed=synth.SEED_BASE + 706), dict(use_gnss=False, use_prior=False, use_imu=False)),
}
_BUILT = {}


def build(name):
    """(window, correspondences, load_window arguments, state to linearise at)"""
    if name not in _BUILT:
        mk, kw = CASES[name]
        win = synth.make_window(**mk)
        st = win.init.copy()
        if not kw["use_gnss"]:
            st.n_ddt = 0
        _BUILT[name] = (win, synth.analytic_correspondences(win), kw, st)
    return _BUILT[name]


def marg_pair():
    """a W = 6 drive as two W = 5 windows one keyframe apart: the first is solved and marginalized, the second inherits the prior that leaves"""
    if "pair" not in _BUILT:
        long = synth.make_window(W=6, pts_per_scan=128, seed=synth.SEED_BASE + 703)
        w0, w1 = synth.sub_window(long, 0, 5), synth.sub_window(long, 1, 5)
        _BUILT["pair"] = (w0, synth.analytic_correspondences(w0), w1, synth.analytic_correspondences(w1))
    return _BUILT["pair"]


def jacobi_kappa(H):
    """(kappa_s, sqrt(diag)): the 2-norm condition number of the Jacobi-scaled H over the columns some factor touches"""
    H = np.asarray(H, np.float64)
    d = np.sqrt(np.diag(H))
    keep = d > 0
    Hs = H[np.ix_(keep, keep)] / d[keep][:, None] / d[keep][None, :]
    return float(np.linalg.cond(0.5 * (Hs + Hs.T))), d


def golden():
    return json.load(open(GOLDEN))


def assert_within_bound(got, H, name, cols=None):
    """|| S (got - Sigma_np) S ||_F <= 8 n kappa_s eps || S Sigma_np S ||_F over the asked columns `cols` (default: all) that some factor touches:
    Sigma_np the rows and columns `cols` of np.linalg.inv(H), S = diag(sqrt(H_kk)) on them, kappa_s the condition number of the Jacobi-scaled H.  The factor is
    twice the 4 n of the dense-Cholesky limit tests because both sides carry rounding.  8 n kappa_s eps < 1e-6 is asserted too: the test cannot pass
    vacuously.  Returns (error, bound, kappa_s)."""
    n = len(H)
    cols = np.arange(n) if cols is None else np.asarray(cols)
    kappa, d = jacobi_kappa(H)
    keep = np.flatnonzero(d > 0)
    where = np.full(n, -1)
    where[keep] = np.arange(len(keep))
    full = np.linalg.inv(H[np.ix_(keep, keep)])
    sel = np.flatnonzero(where[cols] >= 0)                 # positions in `cols` of the columns kept
    want = full[np.ix_(where[cols[sel]], where[cols[sel]])]
    S = d[cols[sel]]
    num = np.linalg.norm(S[:, None] * (got[np.ix_(sel, sel)] - want) * S[None, :])
    den = np.linalg.norm(S[:, None] * want * S[None, :])
    bound = 8 * n * kappa * EPS
    print(f"{name}: n {n}, {len(cols)} columns, kappa_s {kappa:.4e}, scaled error {num / den:.2e}, bound {bound:.2e}")
    assert bound < 1e-6, (name, kappa, bound)
    assert num <= bound * den, (name, num / den, bound)
    return num / den, bound, kappa

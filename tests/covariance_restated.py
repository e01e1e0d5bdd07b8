"""The marginal covariance of the window (include/glio_cov.h) said again in numpy, from the header's contract alone: drop the free columns, Cholesky,
one forward substitution per asked column, the Gram product.  Knows nothing of the library; the tests hold both to the same references and bounds."""
import numpy as np

EPS = np.finfo(np.float64).eps


def spd_family(n, kappa, seed):
    """A = D Q diag(lam) Q^T D with log-spaced lam (condition number kappa) and a graded diagonal D (10^-3 .. 10^3, shuffled), the spread of the diagonal of
    a window's H: the family of the dense-Cholesky limit tests.  Returns A, D, Q and lam."""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.normal(0, 1, (n, n)))
    Q *= np.sign(np.diag(R))
    lam = np.logspace(0, -np.log10(kappa), n)
    A0 = (Q * lam) @ Q.T
    A0 = 0.5 * (A0 + A0.T)
    d = 10.0 ** rng.uniform(-3, 3, n)
    A = d[:, None] * A0 * d[None, :]
    return 0.5 * (A + A.T), d, Q, lam


def family_scaled_inverse(Q, lam):
    """D Sigma* D = Q diag(1 / lam) Q^T of the family, formed in long double (Sigma* = D^-1 Q diag(1 / lam) Q^T D^-1 is the exact inverse of the family's
    matrix up to the rounding of A itself, which the bound's kappa covers)"""
    Ql = Q.astype(np.longdouble)
    return (Ql / lam.astype(np.longdouble)) @ Ql.T


def cholesky_lower(A):
    """left looking, column by column; returns (L, bad, pmin, pmax): bad is -1 or the first column whose pivot is not positive and finite"""
    n = len(A)
    L = np.zeros((n, n))
    pmin, pmax = np.inf, 0.0
    for k in range(n):
        s = A[k:, k] - L[k:, :k] @ L[k, :k]
        p = s[0]
        if not (p > 0.0 and np.isfinite(p)):
            return L, k, pmin, pmax
        pmin, pmax = min(pmin, p), max(pmax, p)
        r = np.sqrt(p)
        L[k:, k] = s / r
        L[k, k] = r
    return L, -1, (pmin if n else 0.0), pmax


def forward_substitute(L, B):
    Y = np.zeros_like(B)
    for i in range(len(L)):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def covariance_columns(H, cols):
    """(out [m][m] or None, info): rows and columns `cols` of the inverse of H (only its lower triangle is read)"""
    H = np.asarray(H, np.float64)
    H = np.tril(H) + np.tril(H, -1).T
    n, cols = len(H), np.asarray(cols, np.int64)
    assert 1 <= len(cols) <= n and len(set(cols.tolist())) == len(cols) and cols.min() >= 0 and cols.max() < n
    free = np.diag(H) == 0.0
    keep = np.flatnonzero(~free)
    nf = len(keep)
    L, bad, pmin, pmax = cholesky_lower(H[np.ix_(keep, keep)])
    info = dict(n=n, n_free=n - nf, n_free_asked=int(free[cols].sum()), bad_pivot=-1 if bad < 0 else int(keep[bad]), min_pivot=float(pmin), max_pivot=float(pmax))
    if bad >= 0:
        return None, info
    where = np.full(n, -1)
    where[keep] = np.arange(nf)
    asked = where[cols]
    E = np.zeros((nf, len(cols)))
    for c, s in enumerate(asked):
        if s >= 0:
            E[s, c] = 1.0
    Y = forward_substitute(L, E)
    out = Y.T @ Y
    out = 0.5 * (out + out.T)
    for c, s in enumerate(asked):
        if s < 0:
            out[c, :] = 0.0
            out[:, c] = 0.0
            out[c, c] = np.inf
    return out, info


def scaled_error(got, want_scaled, d):
    """||D (got - Sigma*) D||_F / ||D Sigma* D||_F with D Sigma* D given (long double)"""
    dl = d.astype(np.longdouble)
    diff = dl[:, None] * got.astype(np.longdouble) * dl[None, :] - want_scaled
    return float(np.sqrt((diff * diff).sum()) / np.sqrt((want_scaled * want_scaled).sum()))


# ---- Pose3 chart (the helper of both hosts, restated for the finite-difference test)
def quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def quat_to_rot(q):
    w, x, y, z = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def window_plus(q, t, dt, d):
    """the window's retraction: t + dt, q' = (cos |d|, sin |d| d / |d|) * q"""
    nrm = np.linalg.norm(d)
    dq = np.array([1.0, 0, 0, 0]) if nrm == 0 else np.r_[np.cos(nrm), np.sin(nrm) / nrm * np.asarray(d)]
    return quat_mul(dq, q), np.asarray(t) + np.asarray(dt)


def rot_log(R):
    c = np.clip((np.trace(R) - 1) / 2, -1, 1)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return v if th < 1e-12 else v * th / np.sin(th)


def pose3_local(q0, t0, q1, t1):
    """GTSAM's Pose3 chart at (q0, t0): (omega, v) with R1 = R0 Exp(omega), t1 = t0 + R0 v"""
    R0, R1 = quat_to_rot(q0), quat_to_rot(q1)
    return np.r_[rot_log(R0.T @ R1), R0.T @ (np.asarray(t1) - np.asarray(t0))]

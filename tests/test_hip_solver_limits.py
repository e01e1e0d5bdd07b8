"""The sliding-window solver at the largest context glio_create accepts: GLIO_MAX_UNKNOWNS = 928 unknowns (15 W + clock-drift epochs),
i.e. W <= 61 without epochs, the largest system whose dense trust-region step fits one workgroup's LDS.

- The in-kernel blocked Cholesky + back substitution (chol_left_looking, back_substitute) from n = 421 up to n = 928 on three families:
  well conditioned, ill conditioned (kappa 1e8 and 1e12, then a graded diagonal scaling as a Jacobi-scaled window has), and not positive
  definite (a negative last pivot must come back as GLIO_E_NUMERIC, not as GLIO_OK with a non-finite x).
- Whole solves and the marginalization at W = 51, 56, 61 (and W = 61 with 13 epochs: n = 928) in every factorisation the library has,
  each against the oracle at the C2 bar and each asserting which path ran.
- The window limit itself: every W up to the limit creates, the next one is refused with GLIO_E_ARG and an error naming the unknown count."""
import ctypes as C

import numpy as np
import pytest

from glio_amd import synth

pytestmark = pytest.mark.gpu

N_MAX = 928                      # GLIO_MAX_UNKNOWNS (include/glio_types.h)
GLIO_OK, GLIO_E_ARG, GLIO_E_NUMERIC = 0, -1, -4
EPS = np.finfo(np.float64).eps
SIZES = [421, 431, 447, 448, 449, 463, 479, 480, 512, 513, 600, 799, 800, 801, 911, 927, 928]


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def big_ctx(hip):
    """the largest context there is: W = 61 with 13 clock-drift epochs, n_max = 15 * 61 + 13 = 928"""
    ctx = hip.Context(synth.default_opts(W=61, pts=64, map_pts=64, n_ddt=13))
    yield ctx
    ctx.close()


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chol_solve(hip, ctx, A, b):
    n = len(b)
    L = np.ascontiguousarray(np.tril(A))
    b = np.ascontiguousarray(b, np.float64)
    x = np.full(n, np.nan)
    rc = hip.load().glio_debug_chol_solve(ctx._h, n, _dp(L), _dp(b), _dp(x))
    return rc, x


def _spd_family(n, kappa, seed):
    """A = D Q diag(lam) Q^T D with log-spaced lam (condition number kappa) and a graded diagonal D (10^-3 .. 10^3, shuffled), the spread of
    the diagonal of a window's H.  Returns A and D."""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.normal(0, 1, (n, n)))
    Q *= np.sign(np.diag(R))
    lam = np.logspace(0, -np.log10(kappa), n)
    A0 = (Q * lam) @ Q.T
    A0 = 0.5 * (A0 + A0.T)
    d = 10.0 ** rng.uniform(-3, 3, n)
    A = d[:, None] * A0 * d[None, :]
    return 0.5 * (A + A.T), d


@pytest.mark.parametrize("n", SIZES)
def test_dense_cholesky_up_to_the_limit(hip, big_ctx, n):
    """Well conditioned (A = B B^T / n + I): forward error <= 1e-11, as below n = 420.  Ill conditioned (kappa 1e8, 1e12 before the grading):
    b = A x* formed in long double and rounded, then the normwise backward error ||b - A x||_inf <= 4 n eps (||A||_inf ||x||_inf + ||b||_inf)
    evaluated in long double, and the forward error in the variables the grading acts on, ||D (x - x*)|| <= 4 n kappa eps ||D x*|| (Cholesky is
    invariant under the diagonal scaling, so kappa is that of the ungraded matrix: van der Sluis)."""
    rng = np.random.default_rng(n)
    B = rng.normal(0, 1, (n, n))
    A = B @ B.T / n + np.eye(n)
    b = rng.normal(0, 1, n)
    rc, x = _chol_solve(hip, big_ctx, A, b)
    assert rc == GLIO_OK
    xs = np.linalg.solve(A, b)
    assert np.linalg.norm(x - xs) <= 1e-11 * np.linalg.norm(xs)
    for kappa in (1e8, 1e12):
        A, d = _spd_family(n, kappa, seed=n + int(np.log10(kappa)))
        xstar = np.random.default_rng(n + 7).normal(0, 1, n) / d          # x* of unit size in the scaled variables D x
        Al = A.astype(np.longdouble)
        b = (Al @ xstar.astype(np.longdouble)).astype(np.float64)
        rc, x = _chol_solve(hip, big_ctx, A, b)
        assert rc == GLIO_OK and np.all(np.isfinite(x)), (n, kappa, rc)
        r = b.astype(np.longdouble) - Al @ x.astype(np.longdouble)
        berr = float(np.abs(r).max())
        bbound = 4 * n * EPS * float(np.abs(Al).sum(1).max() * np.abs(x).max() + np.abs(b).max())
        assert berr <= bbound, (n, kappa, berr, bbound)
        ferr = np.linalg.norm(d * (x - xstar))
        assert ferr <= 4 * n * kappa * EPS * np.linalg.norm(d * xstar), (n, kappa, ferr / np.linalg.norm(d * xstar))
        print(f"n {n} kappa {kappa:.0e} (graded: {np.linalg.cond(A):.1e}): backward error / bound {berr / bbound:.1e}, "
              f"scaled forward error {ferr / np.linalg.norm(d * xstar):.2e}")
    # not positive definite: the last pivot a_nn - a^T A11^-1 a made -1 (relative to the diagonal)
    A = B @ B.T / n + np.eye(n)
    a = A[:-1, -1]
    A[-1, -1] = a @ np.linalg.solve(A[:-1, :-1], a) - 1.0
    rc, x = _chol_solve(hip, big_ctx, A, rng.normal(0, 1, n))
    assert rc == GLIO_E_NUMERIC, rc


def test_dense_cholesky_refuses_past_the_limit(hip, big_ctx):
    A = np.eye(N_MAX + 1)
    rc, _ = _chol_solve(hip, big_ctx, A, np.ones(N_MAX + 1))
    assert rc == GLIO_E_ARG


def test_window_limit(hip):
    """glio_create: every W <= 61 (no epochs) creates; 15 W + epochs = 929 and every W = 62 .. 64 (within GLIO_MAX_WINDOW) is refused with
    GLIO_E_ARG and an error that names the unknown count; an in-range W with too many epochs likewise."""
    lib = hip.load()

    def create(W, nd):
        h = C.c_void_p()
        rc = lib.glio_create(0, C.byref(synth.default_opts(W=W, pts=64, map_pts=64, n_ddt=nd)), C.byref(h))
        if rc == GLIO_OK:
            lib.glio_destroy(h)
        return rc, lib.glio_last_error().decode()

    for W in range(1, 62):
        assert create(W, 0)[0] == GLIO_OK, W
    for W, nd in ((61, 13), (60, 28), (50, 178), (2, 898)):
        assert 15 * W + nd == N_MAX and create(W, nd)[0] == GLIO_OK, (W, nd)
    for W, nd in ((62, 0), (63, 0), (64, 0), (61, 14), (60, 29), (2, 899)):
        rc, err = create(W, nd)
        assert rc == GLIO_E_ARG, (W, nd, rc)
        assert f"{15 * W + nd} unknowns" in err and "GLIO_MAX_UNKNOWNS" in err, err
    rc, err = create(1, 914)                   # the epochs alone leave no room for a keyframe: the message says so, not "W <= 0"
    assert rc == GLIO_E_ARG and "929 unknowns" in err and "no room" in err and "W <= " not in err, err
    assert create(65, 0)[0] == GLIO_E_ARG


# ---- whole solves at the limit: every factorisation the library has, each against the oracle
_ORACLE = {}
WINDOWS = {"W51": (51, False), "W56": (56, False), "W61": (61, False), "W61_gnss": (61, True)}


def _window(key):
    W, gnss = WINDOWS[key]
    if key not in _ORACLE:
        # W = 61 over 24 s of keyframes: an epoch every 24/13 s gives 13 clock-drift unknowns, n = 928
        win = synth.make_window(W=W, pts_per_scan=256, with_gnss=gnss, seed=synth.SEED_BASE + 500 + W, gnss_epoch_dt=(0.4 * (W - 1) / 13) if gnss else 0.1)
        if gnss:
            assert 15 * W + win.init.n_ddt == N_MAX, win.init.n_ddt
        _ORACLE[key] = (win, synth.analytic_correspondences(win), {})
    return _ORACLE[key]


def _oracle_solve(po, key):
    win, corr, memo = _window(key)
    if "solve" not in memo:
        memo["solve"] = po.Problem(win, corr, use_prior=False).solve(win.init.copy())
    return memo["solve"]


# (mode of glio_debug_set_solver, the path glio_debug_solver_path must report, the chain kernel glio_debug_chain_kind must report, whether the
# chain factorisation breaks down).  1 = the graph's own pick: a chain of this length takes chain kind 3 (k_chain_solve<true>, the keyframe
# blocks in global memory); 4 = the arrow factorisation although the graph is a chain; 0 = dense only; 2 = the same chain kernel reports a
# breakdown every step, and the dense fallback (Ceres' mu retries on the generic blocked Cholesky) takes over.  glio_debug_solver_path is the
# path a step was launched with, so the breakdowns themselves are read from the chain kernels' counter (glio_debug_arrow_stamps, slot 301).
FORMS = {"own": (1, 2, 3, False), "arrow": (4, 1, 0, False), "dense": (0, 0, 0, False), "breakdown": (2, 2, 3, True)}
BREAKDOWN_SLOT = 301
# the arrow factorisation's workspaces fit the LDS at W = 51 but no longer at W = 56: there mode 4 ends on the dense path, the kernel "dense"
# already runs, so the arrow form is parametrised where it exists only
CASES = [(k, f) for k in WINDOWS for f in FORMS if f != "arrow" or k == "W51"]


def _breakdowns(lib, ctx):
    st = np.zeros(320, np.int64)
    assert lib.glio_debug_arrow_stamps(ctx._h, st.ctypes.data_as(C.POINTER(C.c_longlong))) == GLIO_OK
    return int(st[BREAKDOWN_SLOT])


@pytest.mark.parametrize("key,form", CASES, ids=[f"{k}-{f}" for k, f in CASES])
def test_solve_at_the_limit(hip, po, key, form):
    win, corr, _ = _window(key)
    so, mo = _oracle_solve(po, key)
    mode, path, kind, breaks = FORMS[form]
    lib = hip.load()
    ctx = hip.Context(win.opts)
    assert lib.glio_debug_set_solver(ctx._h, mode) == GLIO_OK
    ctx.load_window(win, corr, use_prior=False)
    b0 = _breakdowns(lib, ctx)
    sh, mh = ctx.solve(win.init.copy())
    nb = _breakdowns(lib, ctx) - b0
    got_path = lib.glio_debug_solver_path(ctx._h)
    got_kind = lib.glio_debug_chain_kind(ctx._h, int(win.init.n_ddt))
    ctx.close()
    print(f"{key} {form}: path {got_path}, chain kind {got_kind}, {nb} breakdowns, {mh.iterations} / {mo.iterations} iterations, "
          f"max |dt| {np.abs(sh.trans - so.trans).max():.2e} m")
    assert got_path == path and got_kind == kind, (key, form, got_path, got_kind)
    if breaks:
        assert 1 <= nb <= mh.iterations, (key, form, nb)       # every step the chain kernel ran broke down (rejected steps reuse the factor)
    else:
        assert nb == 0, (key, form, nb)
    assert mh.iterations == mo.iterations and mh.successful_steps == mo.successful_steps and mh.termination == mo.termination, (mh.as_dict(), mo.as_dict())
    assert abs(mh.final_cost - mo.final_cost) <= 1e-9 * abs(mo.final_cost)
    assert np.abs(sh.trans - so.trans).max() <= 1e-9 and np.abs(sh.quat - so.quat).max() <= 1e-10


def test_marginalize_at_the_limit(hip, po):
    """W = 61: the device's square root of the Schur complement against the oracle's, by test_hip_marg's _check_root (J0^T J0, J0^T r0,
    |r0|^2, an upper triangular root, the same parameter blocks)."""
    from parity_checks import check_root as _check_root
    win, corr, _ = _window("W61")
    so, _ = _oracle_solve(po, "W61")
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, use_prior=False)
    out_h = ctx.marginalize(so)
    ctx.close()
    _check_root(out_h, po.Problem(win, corr, use_prior=False).marginalize(so))

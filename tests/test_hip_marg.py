"""GPU parity of the on-device marginalization (glio_marginalize) against the oracle's restatement of
MarginalizationInfo (reference GLIO/src/MarginalizationFactor.cpp:128-202, Estimator.cpp:2462-2607).

The reference stores a square root (J0, r0) of the Schur complement; the HIP path takes the Cholesky root, the
reference (and the oracle) the eigen root.  What the next window consumes is J0^T J0, J0^T r0 and |r0|^2, and
those are what is compared -- to 1e-8 relative (fp64; the Schur complement loses a few digits to cancellation)."""
import numpy as np
import pytest

from glio_amd import synth
from parity_checks import check_root as _check_root
from parity_checks import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.mark.parametrize("use_prior", [False, True], ids=["first_window", "with_prior"])
def test_marginalize_matches_oracle(hip, po, small_window, small_corr, use_prior):
    win = small_window
    prob = po.Problem(win, small_corr, use_gnss=False, use_prior=use_prior)
    ctx = hip.Context(win.opts)
    ctx.load_window(win, small_corr, use_gnss=False, use_prior=use_prior)
    st = win.init.copy(); st.n_ddt = 0
    sol, _ = prob.solve(st)
    out_o = prob.marginalize(sol)
    out_h = ctx.marginalize(sol)
    _check_root(out_h, out_o)
    # marginalization must leave the window problem itself untouched
    Ho, go, co = prob.linearize(sol)
    Hh, gh, ch = ctx.linearize(sol)
    assert rel_err(Hh, Ho) <= 1e-10 and abs(ch - co) <= 1e-10 * abs(co)
    ctx.close()


@pytest.mark.parametrize("W", [3, 4], ids=["n21", "n27"])
def test_marginalize_dense_schur_small(hip, po, W):
    """A dense (not block-diagonal) prior sends the kernel through the blocked dense Cholesky (chol_left_looking<SEMI>) with
    n = 21 / 27: two panels, the LAST diagonal block stored by wavefront 0 and read straight after the call by all eight
    wavefronts for the J0 copy -- the hand-off that needs the barrier after the last panel."""
    win = synth.make_window(W=W, pts_per_scan=500, with_prior=True, seed=synth.SEED_BASE + 41 + W)
    assert np.count_nonzero(np.triu(win.prior["lin_jac"].T @ win.prior["lin_jac"], 16)) > 0      # dense information matrix
    corr = synth.analytic_correspondences(win)
    prob = po.Problem(win, corr, use_gnss=False)
    for rep in range(3):                                   # (an ordering defect shows up as a flaky compare: repeat on fresh contexts)
        ctx = hip.Context(win.opts)
        ctx.load_window(win, corr, use_gnss=False)
        st = win.init.copy(); st.n_ddt = 0
        sol, _ = ctx.solve(st)
        out_h = ctx.marginalize(sol)
        assert out_h["n"] == 6 * (W - 1) + 9
        _check_root(out_h, prob.marginalize(sol))
        ctx.close()


def test_marginalize_with_gnss_in_window(hip, po, small_window, small_corr):
    """GNSS factors are not part of the marginalization (Estimator.cpp:2462-2607 adds prior, IMU, LiDAR only)."""
    win = small_window
    prob = po.Problem(win, small_corr)
    ctx = hip.Context(win.opts)
    ctx.load_window(win, small_corr)
    sol, _ = prob.solve(win.init)
    _check_root(ctx.marginalize(sol), prob.marginalize(sol))
    ctx.close()


def test_prior_chain_next_window(hip, po, small_window, small_corr):
    """The prior produced on the device drives the next window exactly like the oracle's: same H, g, cost and
    the same solve (the window content is reused; only the prior changes)."""
    win = small_window
    prob = po.Problem(win, small_corr, use_gnss=False)
    ctx = hip.Context(win.opts)
    ctx.load_window(win, small_corr, use_gnss=False)
    st = win.init.copy(); st.n_ddt = 0
    sol, _ = ctx.solve(st)
    out_h = ctx.marginalize(sol)
    out_o = prob.marginalize(sol)
    nxt = sol.copy()
    nxt.trans += 0.03
    nxt.speed_bias[:, :3] += 0.02
    res = []
    for pr in (out_h, out_o):
        ctx.set_prior(pr)
        H, g, c = ctx.linearize(nxt)
        s2, summ = ctx.solve(nxt)
        res.append((H, g, c, s2, summ))
    (Hh, gh, ch, sh, smh), (Ho, go, co, so, smo) = res
    assert rel_err(Hh, Ho) <= 1e-8 and rel_err(gh, go) <= 1e-8 and abs(ch - co) <= 1e-8 * abs(co)
    assert smh.iterations == smo.iterations
    assert np.linalg.norm(sh.trans - so.trans, axis=1).max() <= 1e-7
    ctx.close()


def test_marginalize_c2_shape(hip, po):
    """Full-size window (W = 50): root reproduces the oracle's Schur complement."""
    win = synth.make_window(W=50, pts_per_scan=2048, with_prior=True, seed=synth.SEED_BASE + 31)
    corr = synth.analytic_correspondences(win)
    prob = po.Problem(win, corr, use_gnss=False)
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, use_gnss=False)
    st = win.init.copy(); st.n_ddt = 0
    sol, _ = ctx.solve(st)
    _check_root(ctx.marginalize(sol), prob.marginalize(sol))
    ctx.close()


def test_marginalize_keep_equals_roundtrip(hip, small_window, small_corr):
    """glio_marginalize_keep installs on the device exactly the prior that glio_marginalize + glio_set_prior would."""
    win = small_window
    st = win.init.copy(); st.n_ddt = 0
    res = []
    for keep in (False, True):
        ctx = hip.Context(win.opts)
        ctx.load_window(win, small_corr, use_gnss=False)
        sol, _ = ctx.solve(st)
        if keep:
            ctx.marginalize_keep(sol)
        else:
            ctx.set_prior(ctx.marginalize(sol))
        nxt = sol.copy(); nxt.trans += 0.02
        res.append(ctx.linearize(nxt) + (ctx.solve(nxt),))
        ctx.close()
    (Ha, ga, ca, (sa, ma)), (Hb, gb, cb, (sb, mb)) = res
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and ca == cb
    assert ma.iterations == mb.iterations and np.array_equal(sa.trans, sb.trans)


def test_marginalize_then_band_only_solve_with_dense_fallback(hip):
    """Advisor finding (round 4): the long-window chain path (chain kind 3: band-only assembly, k_chain_solve<true>) keeps both dense H buffers zero
    outside the block-tridiagonal band and remembers that in h_band_clean; glio_marginalize overwrites those buffers (its pos x pos A, its J0).  A
    solve AFTER a plain glio_marginalize -- prior untouched, so nothing else resets the flag -- whose chain kernel breaks down (debug mode 2: every step)
    falls back to the dense factorisation of the whole matrix: it must see zeros off the band, i.e. give the iterates of the dense solver."""
    W = 50
    long = synth.make_window(W=W + 1, pts_per_scan=1024, seed=synth.SEED_BASE + 33)
    first = synth.sub_window(long, 0, W)
    win = synth.sub_window(long, 1, W)
    corr0, corr = synth.analytic_correspondences(first), synth.analytic_correspondences(win)
    st0 = first.init.copy(); st0.n_ddt = 0
    st = win.init.copy(); st.n_ddt = 0
    lib = hip.load()

    def with_chain_prior(mode):
        """a context holding window 1 with the device marginalization of window 0 as its prior (block diagonal by keyframe: the chain path applies)"""
        ctx = hip.Context(win.opts)
        lib.glio_debug_set_solver(ctx._h, mode)
        ctx.load_window(first, corr0, use_gnss=False)
        s, _ = ctx.solve(st0)
        ctx.marginalize_keep(s)
        for k in range(W):                                  # window 1's factors; the resident prior stays
            ctx.set_correspondences(k, *corr[k])
        ctx.set_imu(win.preints)
        return ctx

    ref = with_chain_prior(0)
    s0, m0 = ref.solve(st)
    ref.close()
    ctx = with_chain_prior(1)
    s1, m1 = ctx.solve(st)                                   # band-only assemblies: the buffers are declared clean for this n
    assert lib.glio_debug_solver_path(ctx._h) == 2
    ctx.marginalize(s1)                                      # ... and overwritten here
    lib.glio_debug_set_solver(ctx._h, 2)                     # every chain step reports a breakdown: dense fallback on the assembled matrix
    s2, m2 = ctx.solve(st)
    ctx.close()
    assert m1.iterations == m0.iterations
    assert m2.iterations == m0.iterations and m2.termination == m0.termination
    assert np.abs(s2.trans - s0.trans).max() <= 1e-9 and np.abs(s2.quat - s0.quat).max() <= 1e-10


def test_three_launch_marginalization_equals_the_one_workgroup_form():
    """Round 6 splits k_marg_schur (everything in one workgroup over global-memory matrices: 90 us for n = 123) into k_marg_inv / k_marg_rows (n + 1
    workgroups) / k_marg_root: the same sums in the same order -- the prior is the same bit for bit, for a first window (rank-deficient Amm: Jacobi
    eigen-decomposition) and a steady-state window (fast inverse), at W = 20 and at W = 3 (smallest scratch)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for W in ("20", "3"):
        rows = []
        for split in ("1", "0"):
            env = dict(os.environ, GLIO_MARG_SPLIT=split, MS_W=W, MS_PTS="2048")
            out = subprocess.run([sys.executable, os.path.join(root, "scripts", "marg_split_ab.py")], env=env, capture_output=True, text=True, timeout=300)
            rows.append(json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("{"))))
        assert rows[0]["first_window"] == rows[1]["first_window"] and rows[0]["steady_window"] == rows[1]["steady_window"], rows

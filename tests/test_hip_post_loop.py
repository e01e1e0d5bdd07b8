"""GPU: the windows after a loop closure (glio_set_speed_bias_priors, the generalised kept layout of glio_marginalize*, glio_marginalize_size).

The oracle takes the factors as a synthetic marginalization prior (tests/marg_layout_restated.py: same residual, same Jacobian); the marginalization is
held to the numpy restatement and to the reference's own results recorded in tests/golden/post_loop_marg.npz.  Shapes: W = 2 .. 5 with 300-500 points
per scan -- every factor dropped / slot 1 merged with the IMU-kept block / the first extra block / two extras and a two-step shrink.  Tolerances are
those of tests/test_hip_marg.py and tests/test_hip_parity.py for the same quantities: 1e-8 on J0^T J0, J0^T r0 (against the whole vector), 1e-7 on
|r0|^2; 1e-10 on H, g, cost of a linearisation (1e-8 once a device-made prior is involved, as test_prior_chain_next_window); the same iterations and
termination; translations to 1e-7 m."""
import importlib.util
import os

import numpy as np
import pytest

import marg_layout_restated as mr
from glio_amd import ctypes_types as T
from parity_checks import rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_post_loop", os.path.join(HERE, "golden", "make_golden_post_loop.py"))
gold = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(gold)
WS = sorted(mr.SHAPES)


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
def G():
    return gold.load()


@pytest.fixture(scope="module")
def scen():
    return {W: mr.scenario_window(W) for W in WS}


@pytest.fixture(scope="module")
def restated_chain(G, scen):
    """per W: the restatement's own chain at the recorded states: out[k] = marginalization of window k with out[k - 1] as its prior (computed once)"""
    chains = {}
    for W in WS:
        win, corr = scen[W]
        outs = []
        for k in range(W):
            sol = gold.state_of(G, W, k, "sol", win.init)
            outs.append(mr.marginalize(win, corr, sol, None if k == 0 else outs[-1], W - 1 if k == 0 else 0))
        chains[W] = outs
    return chains


def fresh(hip, win, corr, prior=None):
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, use_gnss=False, use_prior=False)
    if prior is not None:
        ctx.set_prior(prior)
    return ctx


def path_of(hip, ctx):
    return hip.load().glio_debug_solver_path(ctx._h)


def same_root(got, want, label=""):
    assert got["n"] == want["n"], label
    Sg, bg = got["lin_jac"].T @ got["lin_jac"], got["lin_jac"].T @ got["lin_res"]
    e = (rel_err(Sg, want["S"]), np.linalg.norm(bg - want["bs"]) / np.linalg.norm(want["bs"]),
         abs(got["lin_res"] @ got["lin_res"] - want["lin_res"] @ want["lin_res"]) / max(want["lin_res"] @ want["lin_res"], 1e-30))
    print("root %s: n %d  J0^T J0 %.2e  J0^T r0 %.2e  |r0|^2 %.2e" % (label, got["n"], *e))
    assert e[0] <= 1e-8 and e[1] <= 1e-8 and e[2] <= 1e-7, (label, e)
    for k in ("blk_slot", "blk_kind", "blk_idx"):
        assert np.array_equal(got[k], want[k]), (label, k, got[k], want[k])
    assert np.array_equal(got["blk_x0"], want["blk_x0"]), label


def check_extras(got, W, state):
    ns = mr.std_n(W)
    S = got["lin_jac"].T @ got["lin_jac"]
    for j in range((got["n"] - ns) // 9):
        c = ns + 9 * j
        assert np.array_equal(S[c:c + 9, c:c + 9], np.diag(mr.SBP_W ** 2)), (W, j, S[c:c + 9, c:c + 9])
        assert not np.delete(S[c:c + 9], np.s_[c:c + 9], axis=1).any() and not np.delete(S[:, c:c + 9], np.s_[c:c + 9], axis=0).any()
        b = 2 * (W - 1) + 1 + j
        assert got["blk_kind"][b] == T.BLK_SPEEDBIAS and got["blk_idx"][b] == c
        assert np.array_equal(got["blk_x0"][b], state.speed_bias[got["blk_slot"][b] + 1])


def solves_agree(sh, mh, so, mo, label=""):
    dt, dsb = np.linalg.norm(sh.trans - so.trans, axis=1).max(), np.abs(sh.speed_bias - so.speed_bias).max()
    print("solve %s: iterations %d / %d, termination %d / %d, max |dt| %.2e m, max |d speed/bias| %.2e" % (label, mh.iterations, mo.iterations, mh.termination, mo.termination, dt, dsb))
    assert mh.iterations == mo.iterations and mh.termination == mo.termination, label
    assert dt <= 1e-7, label


@pytest.mark.parametrize("W", WS)
def test_linearize_and_solve_with_the_factors(hip, po, scen, W):
    """no marginalization prior beside them: the reference's sequence"""
    win, corr = scen[W]
    tg = mr.first_targets(win)
    st = win.init.copy(); st.n_ddt = 0
    moved = st.copy(); moved.speed_bias[:, :3] += 0.05; moved.trans += 0.01
    prob = po.Problem(mr.with_prior(win, mr.synthetic_prior(tg)), corr, use_gnss=False)
    ctx = fresh(hip, win, corr)
    s0, m0 = ctx.solve(st)
    path0 = path_of(hip, ctx)
    ctx.set_speed_bias_priors(tg)
    for x in (st, moved):
        Hh, gh, ch = ctx.linearize(x)
        Ho, go, co = prob.linearize(x)
        print("W %d: H %.2e g %.2e cost %.2e" % (W, rel_err(Hh, Ho), rel_err(gh, go), abs(ch - co) / abs(co)))
        assert rel_err(Hh, Ho) <= 1e-10 and rel_err(gh, go) <= 1e-10 and abs(ch - co) <= 1e-10 * abs(co)
    sh, mh = ctx.solve(st)
    assert path_of(hip, ctx) == path0                     # the factors leave the solver on the path it takes without them
    so, mo = prob.solve(st)
    solves_agree(sh, mh, so, mo, "W %d" % W)
    ms, summ = ctx.time_solve(st, reps=1)                 # the timing entry point runs the same problem
    assert summ.iterations == mh.iterations and summ.termination == mh.termination and abs(summ.final_cost - mh.final_cost) <= 1e-10 * mh.final_cost
    assert np.abs(sh.speed_bias - s0.speed_bias).max() > 1e-3      # not a no-op
    ctx.close()


def test_linearize_and_solve_with_the_factors_beside_a_prior(hip, po, small_window, small_corr):
    win, corr = small_window, small_corr
    W = win.W
    tg = win.init.speed_bias[:W - 1].copy()
    st = win.init.copy(); st.n_ddt = 0
    moved = st.copy(); moved.speed_bias[:, :3] += 0.05; moved.trans += 0.01
    prob = po.Problem(mr.with_prior(win, mr.stack_priors(win.prior, mr.synthetic_prior(tg))), corr, use_gnss=False)
    ctx = fresh(hip, win, corr, win.prior)
    s0, m0 = ctx.solve(st)
    path0 = path_of(hip, ctx)
    ctx.set_speed_bias_priors(tg)
    for x in (st, moved):
        Hh, gh, ch = ctx.linearize(x)
        Ho, go, co = prob.linearize(x)
        print("beside a prior: H %.2e g %.2e cost %.2e" % (rel_err(Hh, Ho), rel_err(gh, go), abs(ch - co) / abs(co)))
        assert rel_err(Hh, Ho) <= 1e-10 and rel_err(gh, go) <= 1e-10 and abs(ch - co) <= 1e-10 * abs(co)
    sh, mh = ctx.solve(st)
    assert path_of(hip, ctx) == path0
    so, mo = prob.solve(st)
    solves_agree(sh, mh, so, mo, "beside a prior")
    assert np.abs(sh.speed_bias - s0.speed_bias).max() > 1e-3
    ctx.close()


@pytest.mark.parametrize("W", WS)
def test_marginalize_with_the_factors(hip, G, scen, restated_chain, W):
    win, corr = scen[W]
    sol = gold.state_of(G, W, 0, "sol", win.init)
    ctx = fresh(hip, win, corr)
    ctx.set_speed_bias_priors(mr.first_targets(win))
    assert ctx.marginalize_size() == (mr.expected_n(W), 2 * (W - 1) + 1 + max(W - 3, 0))
    got = ctx.marginalize(sol)
    assert got["n"] == {2: 15, 3: 21, 4: 36, 5: 51}[W]
    same_root(got, restated_chain[W][0], "restated W %d" % W)
    same_root(got, gold.prior_of(G, W, 0), "recorded W %d" % W)
    check_extras(got, W, sol)
    again = ctx.marginalize(sol)                          # glio_marginalize leaves the context as it found it
    assert np.array_equal(again["lin_jac"], got["lin_jac"]) and np.array_equal(again["lin_res"], got["lin_res"])
    ctx.close()


@pytest.mark.parametrize("W", [4, 5])
def test_keep_equals_roundtrip_on_the_extended_layout(hip, G, scen, W):
    win, corr = scen[W]
    sol = gold.state_of(G, W, 0, "sol", win.init)
    nxt = gold.state_of(G, W, 1, "start", win.init)
    res = []
    for keep in (False, True):
        ctx = fresh(hip, win, corr)
        ctx.set_speed_bias_priors(mr.first_targets(win))
        if keep:
            ctx.marginalize_keep(sol)
        else:
            pr = ctx.marginalize(sol)
            ctx.set_speed_bias_priors(None)
            ctx.set_prior(pr)
        assert ctx.marginalize_size()[0] == mr.expected_n(W) - 9
        res.append(ctx.linearize(nxt) + (ctx.solve(nxt),))
        ctx.close()
    (Ha, ga, ca, (sa, ma)), (Hb, gb, cb, (sb, mb)) = res
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and ca == cb
    assert ma.iterations == mb.iterations and np.array_equal(sa.trans, sb.trans) and np.array_equal(sa.speed_bias, sb.speed_bias)


@pytest.mark.parametrize("W", WS)
def test_the_whole_transient(hip, po, G, scen, restated_chain, W):
    """W successive marginalize_keep windows against the restated chain: n and the block tables at each, the next window's H, g, cost and solve each time;
    after the last one the layout is the standard one again.  Every window of the transient stays on the step path of the steady state.

    The root of window k >= 1 is held to the restatement GIVEN THE SAME PRIOR (the device's own result of window k - 1, read back), not to the restated
    chain's: the windows are marginalized at their optimum, where J0^T r0 is what is left of terms that cancel (W = 2, window 1: the prior's gradient is
    2.3e4, the vector 0.76, because prior + IMU + LiDAR are ALL factors of a two-keyframe window and their gradient vanishes at the solution).  Two
    priors that agree to 2e-14 then give vectors 1.6e-8 apart -- measured on the CPU between the restatement fed with its own and with the reference's
    recorded prior of window 0, and the same 1.57e-8 between the device's chain and the restated chain.  With the same prior on both sides the check is
    the marginalization's own arithmetic again (8e-13 on the CPU).  Against the chain itself: n, the block tables, x0 and J0^T J0."""
    win, corr = scen[W]
    outs = restated_chain[W]
    ctx = fresh(hip, win, corr)
    ctx.set_speed_bias_priors(mr.first_targets(win))
    paths = []
    for k in range(W):
        start, sol = gold.state_of(G, W, k, "start", win.init), gold.state_of(G, W, k, "sol", win.init)
        prior_in = mr.synthetic_prior(mr.first_targets(win)) if k == 0 else outs[k - 1]
        prob = po.Problem(mr.with_prior(win, prior_in), corr, use_gnss=False)
        Hh, gh, ch = ctx.linearize(start)
        Ho, go, co = prob.linearize(start)
        tol = 1e-10 if k == 0 else 1e-8
        print("W %d window %d: H %.2e g %.2e cost %.2e" % (W, k, rel_err(Hh, Ho), rel_err(gh, go), abs(ch - co) / abs(co)))
        assert rel_err(Hh, Ho) <= tol and rel_err(gh, go) <= tol and abs(ch - co) <= tol * abs(co)
        sh, mh = ctx.solve(start)
        paths.append(path_of(hip, ctx))
        so, mo = prob.solve(start)
        solves_agree(sh, mh, so, mo, "W %d window %d" % (W, k))
        n_want = max(mr.expected_n(W) - 9 * k, mr.std_n(W))
        assert ctx.marginalize_size()[0] == n_want == outs[k]["n"]
        got = ctx.marginalize(sol)
        want = outs[k] if k == 0 else mr.marginalize(win, corr, sol, prev, 0)
        same_root(got, want, "W %d window %d" % (W, k))
        assert rel_err(got["lin_jac"].T @ got["lin_jac"], outs[k]["S"]) <= 1e-8
        for f in ("blk_slot", "blk_kind", "blk_idx", "blk_x0"):
            assert np.array_equal(got[f], outs[k][f]), (k, f)
        check_extras(got, W, sol)
        prev = got
        ctx.marginalize_keep(sol)
    assert ctx.marginalize_size() == (mr.std_n(W), 2 * (W - 1) + 1)
    assert len(set(paths)) == 1, paths
    ctx.close()


@pytest.mark.parametrize("W", [3, 5])
def test_cleared_factors_leave_no_trace(hip, G, scen, W):
    win, corr = scen[W]
    st = win.init.copy(); st.n_ddt = 0
    res = []
    for touched in (False, True):
        ctx = fresh(hip, win, corr)
        if touched:
            ctx.set_speed_bias_priors(mr.first_targets(win))
            ctx.solve(st)
            ctx.set_speed_bias_priors(None)
        H, g, c = ctx.linearize(st)
        sol, summ = ctx.solve(st)
        out = ctx.marginalize(sol)
        res.append((H, g, c, sol, summ, out))
        ctx.close()
    a, b = res
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[4].iterations == b[4].iterations and np.array_equal(a[3].trans, b[3].trans) and np.array_equal(a[3].speed_bias, b[3].speed_bias)
    assert a[5]["n"] == b[5]["n"] == mr.std_n(W)
    assert np.array_equal(a[5]["lin_jac"], b[5]["lin_jac"]) and np.array_equal(a[5]["lin_res"], b[5]["lin_res"])


def test_refusals(hip, scen):
    W = 4
    win, corr = scen[W]
    ctx = fresh(hip, win, corr)
    tg = np.zeros((W, 9))
    with pytest.raises(hip.GlioError, match="error -1: speed-bias priors on 4 slots"):
        ctx.set_speed_bias_priors(tg)                      # n_slots > W - 1
    bad = tg[:W - 1].copy(); bad[1, 4] = np.nan
    with pytest.raises(hip.GlioError, match="error -1: .*not finite"):
        ctx.set_speed_bias_priors(bad)
    n = max(6 * W + 9, 15 * (W - 1)) + 3                   # one translation block above the limit
    nb = n // 3
    big = dict(n=n, lin_jac=np.eye(n), lin_res=np.zeros(n), blk_slot=np.zeros(nb, np.int32), blk_kind=np.zeros(nb, np.int32),
               blk_idx=(3 * np.arange(nb)).astype(np.int32), blk_x0=np.zeros((nb, 9)))
    with pytest.raises(hip.GlioError, match="error -1: prior too large"):
        ctx.set_prior(big)
    ctx.set_speed_bias_priors(tg[:W - 1])                  # the largest legal count is taken
    ctx.set_imu(win.preints[:1])                           # ... but each factor is evaluated with the IMU edge that leaves its slot
    st = win.init.copy(); st.n_ddt = 0
    with pytest.raises(hip.GlioError, match="error -1: .*needs the IMU edge"):
        ctx.linearize(st)
    ctx.close()

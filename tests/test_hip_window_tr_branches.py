"""Every copy of the window solve's trust-region loop on the device -- tr_prepare_body<FAST> / <!FAST>, tr_factor_body, tr_dogleg_body, the LDS
fast tail of k_chain_step, finalize and finalize_lds (solver_kernels.hip) -- against the oracle on the cases of tests/window_tr_cases.py:
boundary (Cauchy) and interpolated dogleg steps, accepted steps on either side of 0.25 and 0.75, natural rejections and the `reuse` re-entry,
Levenberg-Marquardt with its doubling decrease factor, and every termination 0 .. 5.  tests/test_window_tr_cases_cpu.py shows that the cases
take those branches, that the oracle and the numpy restatement of the Ceres loop agree on them and that no decision sits near its threshold.

Forms (glio_debug_set_solver modes; the path that ran is asserted with glio_debug_solver_path / glio_debug_chain_kind):
  own (1)            k_chain_step where the graph is a chain, with the LDS front, tail and finalize_lds
  own_generic (1)    the same with glio_debug_chain_fast(0): the generic bodies inside k_chain_step
  own_old_ends (1)   the same with glio_debug_solve_ends(0): the staging launch and finalize()
  dense (0), arrow (4), breakdown (2: the chain kernel reports a bad pivot every step, the dense retry loop takes over), legacy (3)

Whole solves: iterations, successful steps and termination equal the oracle's; costs and final radius to 1e-9 relative (the radius EXACTLY where
it is a product of exact factors, window_tr_cases.exact_radius_prefix), the gradient norm to 1e-6, the state to window_tr_cases.STATE_GATES.
Prefix solves: the device keeps no history, so every case is solved again with max_iterations = k for k = 0 .. n (a context each: the
options are fixed at glio_create) and compared with the oracle's solve under the same cap -- each iterate becomes observable, and every
iteration of every case passes through the code that ends a solve on that path.  The state tolerance of a prefix is the final-state gate or
100 x S_k of tests/golden/window_tr_spread.json (two decimal digits over the spread between the two CPU witnesses), whichever is larger.

Pairs that are not run, because the graph cannot take the path:
  * far_w5_prior, far_w12_prior (synth's prior couples every pose with every other: not a chain): the chain forms own_generic, own_old_ends,
    breakdown and legacy would run the very kernels of `own` (glio_debug_chain_kind reports 0 in every mode), and mode 4 is mode 1 for
    them: the arrow factorisation.  They run own (arrow) and dense.
Every other case is a chain, lm_w1 (one keyframe, no edge) included, and runs all seven forms."""
import ctypes as C

import numpy as np
import pytest

import window_tr_cases as wc
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu
GLIO_E_NUMERIC = -4

# form: (glio_debug_set_solver mode, glio_debug_chain_fast mask or None, glio_debug_solve_ends mask or None)
FORMS = {"own": (1, None, None), "own_generic": (1, 0, None), "own_old_ends": (1, None, 0), "dense": (0, None, None), "arrow": (4, None, None),
         "breakdown": (2, None, None), "legacy": (3, None, None)}
# (path, chain kind) a chain-shaped graph must report per form: path 2 = keyframe chain, 1 = arrow, 0 = dense; kind 1 = k_chain_step, 2 = the legacy sequence
CHAIN_EXPECT = {"own": (2, 1), "own_generic": (2, 1), "own_old_ends": (2, 1), "dense": (0, 0), "arrow": (1, 0), "breakdown": (2, 1), "legacy": (2, 2)}
DENSE_PRIOR = ("far_w5_prior", "far_w12_prior")
DENSE_PRIOR_EXPECT = {"own": (1, 0), "dense": (0, 0)}
NOT_RUN = [(c, f) for c in DENSE_PRIOR for f in FORMS if f not in ("own", "dense")]
PAIRS = [(c, f) for c in wc.CASES for f in FORMS if (c, f) not in NOT_RUN]
BREAKDOWN_SLOT = 301


def _expect(case, form):
    if case in DENSE_PRIOR:
        return DENSE_PRIOR_EXPECT[form]
    return CHAIN_EXPECT[form]


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def golden():
    return wc.load_golden()


def _breakdowns(lib, ctx):
    st = np.zeros(320, np.int64)
    assert lib.glio_debug_arrow_stamps(ctx._h, st.ctypes.data_as(C.POINTER(C.c_longlong))) == 0
    return int(st[BREAKDOWN_SLOT])


def _raw_solve(lib, ctx, start):
    """glio_solve itself: a solve that ends in FAILURE returns GLIO_E_NUMERIC WITH the state and the summary filled in (Context.solve raises on it)"""
    s = start.copy()
    cs = s.c()
    m = T.GlioSummary()
    rc = lib.glio_solve(ctx._h, C.byref(cs), C.byref(m))
    assert rc == (GLIO_E_NUMERIC if m.termination == wc.TERMINATIONS["FAILURE"] else 0), (rc, lib.glio_last_error().decode(), m.as_dict())
    return s, m


def _solve(hip, opts, mode, win, corr, start, use):
    lib = hip.load()
    ctx = hip.Context(opts)
    try:
        assert lib.glio_debug_set_solver(ctx._h, mode) == 0
        ctx.load_window(win, corr, **use)
        b0 = _breakdowns(lib, ctx)
        s, m = _raw_solve(lib, ctx, start)
        info = (int(lib.glio_debug_solver_path(ctx._h)), int(lib.glio_debug_chain_kind(ctx._h, int(start.n_ddt))), _breakdowns(lib, ctx) - b0)
        if info[1] == 1:          # k_chain_step: two elimination fronts below twelve keyframes, the separator and four fronts from twelve on
            assert lib.glio_debug_chain_fronts_used(ctx._h) == (4 if win.W >= 12 else 2), (win.W, lib.glio_debug_chain_fronts_used(ctx._h))
    finally:
        ctx.close()
    return s, m, info


_DEVICE = {}


def _device_prefixes(hip, case, form):
    """[(state, summary, (path, chain kind, breakdowns))] of the device's solves with max_iterations = 0 .. n under `form`; once per pair"""
    if (case, form) in _DEVICE:
        return _DEVICE[(case, form)]
    lib = hip.load()
    win, corr, start, use = wc.build(case)
    n = len(wc.oracle_prefixes(case)) - 1
    mode, fast, ends = FORMS[form]
    old_fast = lib.glio_debug_chain_fast(3)
    lib.glio_debug_chain_fast(old_fast)
    old_ends = lib.glio_debug_solve_ends(0)
    lib.glio_debug_solve_ends(old_ends)
    assert old_fast in (-1, 3) and old_ends == 6, "the library's defaults: every fast path on"
    out = []
    try:
        if fast is not None:
            lib.glio_debug_chain_fast(fast)
        if ends is not None:
            lib.glio_debug_solve_ends(ends)
        for k in range(n + 1):
            opts = win.opts if k == n else wc.with_max_iterations(win, k).opts
            out.append(_solve(hip, opts, mode, win, corr, start, use))
    finally:
        lib.glio_debug_chain_fast(old_fast)
        lib.glio_debug_solve_ends(old_ends)
    _DEVICE[(case, form)] = out
    return out


def _check_path(case, form, info, iterations):
    path, kind, nb = info
    assert (path, kind) == _expect(case, form), (case, form, path, kind)
    if form == "breakdown":
        # every step the chain kernel factored broke down (a rejected dogleg step reuses the stored vectors: no factorisation)
        assert (1 <= nb <= iterations) if iterations else nb == 0, (case, nb, iterations)
    elif case != "failure":
        assert nb == 0, (case, form, nb)


@pytest.mark.parametrize("case,form", PAIRS, ids=[f"{c}-{f}" for c, f in PAIRS])
def test_whole_solve(hip, case, form):
    so, mo = wc.oracle_prefixes(case)[-1]
    s, m, info = _device_prefixes(hip, case, form)[-1]
    print(f"{case} {form}: path {info[0]}, chain kind {info[1]}, {info[2]} breakdowns")
    _check_path(case, form, info, m.iterations)
    wc.compare_with_oracle(s, m, so, mo, exact_radius=wc.exact_radius_prefix(case) >= mo.iterations, label=f"{case} {form}")
    want = wc.CASES[case]["expect"]
    if "termination" in want:
        assert m.termination == want["termination"]


@pytest.mark.parametrize("case,form", PAIRS, ids=[f"{c}-{f}" for c, f in PAIRS])
def test_prefix_solves(hip, golden, case, form):
    pre = wc.oracle_prefixes(case)
    dev = _device_prefixes(hip, case, form)
    tol = wc.prefix_tolerances(case, golden)
    exact = wc.exact_radius_prefix(case)
    assert len(dev) == len(pre) == len(tol)
    worst = {}
    for k, ((so, mo), (s, m, info)) in enumerate(zip(pre, dev)):
        _check_path(case, form, info, m.iterations)
        assert mo.iterations == k
        r = wc.compare_with_oracle(s, m, so, mo, state_tol=tol[k], exact_radius=k <= exact, label=f"{case} {form} k={k}")
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"{case} {form}: {len(pre)} prefixes, largest figure / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("case", list(wc.CASES))
def test_forms_agree(hip, case):
    """one case, all forms: the integer fields of the summaries are equal and the final radius agrees to 1e-9 relative -- at every prefix"""
    forms = [f for c, f in PAIRS if c == case]
    runs = {f: _device_prefixes(hip, case, f) for f in forms}
    ref = runs[forms[0]]
    for f in forms[1:]:
        for k, ((_, a, _), (_, b, _)) in enumerate(zip(ref, runs[f])):
            assert (a.iterations, a.successful_steps, a.termination) == (b.iterations, b.successful_steps, b.termination), (case, f, k, a.as_dict(), b.as_dict())
            assert abs(a.final_radius - b.final_radius) <= 1e-9 * abs(a.final_radius), (case, f, k, a.final_radius, b.final_radius)


FAILURE_FORMS = [f for c, f in PAIRS if c == "failure"]


@pytest.mark.parametrize("form", FAILURE_FORMS)
def test_failure_returns_the_start_and_leaves_the_context_usable(hip, form):
    """The reference's HandleInvalidStep: an overflowing bias Jacobian makes H non-finite, every factorisation fails, five invalid steps end the solve
    with FAILURE and the state comes back as it went in, bit for bit.
    The path of the non-finite values, as read in solver_kernels.hip: the chain fronts of k_chain_step only RECORD a bad pivot (chain_step15 sets
    `bad`, no early exit) and publish their progress counters after every step regardless; every wait inside the kernel (s_prog, the helpers'
    completion words -- the latter bounded by hpolls) is on such an integer counter, never on a computed value, so a NaN cannot stall one.  The
    flag then sends the step to tr_factor_body, whose retry loop ends on `!(mu < 1.0)` after eight failed Cholesky factorisations
    (!(djj > 0) || !isfinite(djj)), sets lin_fail, and tr_dogleg_body counts the invalid step; the dense and arrow forms enter the same loop.
    A healthy window solved next on the same context must give the bits a fresh context gives: nothing of the failed solve is left behind."""
    lib = hip.load()
    win, corr, start, use = wc.build("failure")
    good, gcorr, gstart, guse = wc.build("grad_tol_late")          # the same window without the overflow (the context keeps its own options)
    mode, fast, ends = FORMS[form]
    key = lambda s, m: (s.trans.tobytes(), s.quat.tobytes(), s.speed_bias.tobytes(), s.rcv_ddt[:s.n_ddt].tobytes(), tuple(sorted(m.as_dict().items())))
    old_fast = lib.glio_debug_chain_fast(3)
    lib.glio_debug_chain_fast(old_fast)
    old_ends = lib.glio_debug_solve_ends(0)
    lib.glio_debug_solve_ends(old_ends)
    try:
        if fast is not None:
            lib.glio_debug_chain_fast(fast)
        if ends is not None:
            lib.glio_debug_solve_ends(ends)
        ctx = hip.Context(win.opts)
        assert lib.glio_debug_set_solver(ctx._h, mode) == 0
        ctx.load_window(win, corr, **use)
        s, m = _raw_solve(lib, ctx, start)
        assert "trust-region solver failure" in lib.glio_last_error().decode()
        ctx.load_window(good, gcorr, **guse)
        after = ctx.solve(gstart)
        ctx.close()
        fresh_ctx = hip.Context(win.opts)
        assert lib.glio_debug_set_solver(fresh_ctx._h, mode) == 0
        fresh_ctx.load_window(good, gcorr, **guse)
        fresh = fresh_ctx.solve(gstart)
        fresh_ctx.close()
    finally:
        lib.glio_debug_chain_fast(old_fast)
        lib.glio_debug_solve_ends(old_ends)
    assert (m.iterations, m.successful_steps, m.termination) == (5, 0, wc.TERMINATIONS["FAILURE"]), m.as_dict()
    assert np.array_equal(wc.flat_state(s), wc.flat_state(start)) and m.final_cost == m.initial_cost
    assert after[1].iterations >= 3 and after[1].termination == wc.TERMINATIONS["FUNCTION_TOL"]
    assert key(*after) == key(*fresh), (after[1].as_dict(), fresh[1].as_dict())

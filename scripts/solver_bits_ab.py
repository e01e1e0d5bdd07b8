"""Bits of the window solver, for A/B runs of two builds of the library (GLIO_HIP_LIB selects one; a fresh process per build): one sha256 per case over
the state bytes and the summary fields of a solve, over the prior (J0, r0) of a marginalization, over the solution of the blocked Cholesky.  Two builds
that compute the same print the same lines.  Cases: the steady window of tests/test_hip_parity.py (W = 5) under solver modes 0..4 with and without GNSS
(dense, k_chain_step, breakdown, the legacy sequence, arrow with the packed Cholesky); W = 12 / 13 with two and four fronts, with and without GNSS; W = 28 (k_chain_solve<true>);
the W = 4 window after a loop closure (extended kept layout); marginalization of a first and a steady window at W = 5, of W = 61 and of W = 2 (k_marg_schur:
the split form's scratch does not fit) under the GLIO_MARG_SPLIT of the environment; glio_debug_chol_solve at n = 17, 123, 414.
SB_ONLY=marg prints the marginalization cases only (for the second GLIO_MARG_SPLIT value).
Which inverse of Amm a marginalization takes (Jacobi for the first window, whose Amm is rank deficient without a prior; the fast inverse for the steady
window) follows from how the windows are built; the library reports neither, so the script does not observe or check it."""
import ctypes as C, hashlib, importlib.util, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from glio_amd import synth, capi
lib = capi.load()
only_marg = os.environ.get("SB_ONLY") == "marg"


def sha(*parts):
    m = hashlib.sha256()
    for p in parts:
        m.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return m.hexdigest()[:16]


def solve_hash(s, m):
    fields = np.array([m.iterations, m.successful_steps, m.termination, m.initial_cost, m.final_cost, m.final_radius, m.gradient_max_norm], np.float64)
    return sha(s.trans, s.quat, s.speed_bias, s.rcv_ddt[:s.n_ddt], fields)


def prior_hash(p):
    return sha(p["lin_jac"], p["lin_res"])


def state_for(win, use_gnss):
    st = win.init.copy()
    if not use_gnss:
        st.n_ddt = 0
    return st


def solved(win, corr, mode, use_gnss=True, fronts=4, st=None, **load):
    lib.glio_debug_chain_fronts(fronts)
    ctx = capi.Context(win.opts)
    lib.glio_debug_set_solver(ctx._h, mode)
    ctx.load_window(win, corr, use_gnss=use_gnss, **load)
    s, m = ctx.solve(state_for(win, use_gnss) if st is None else st)
    info = (lib.glio_debug_solver_path(ctx._h), lib.glio_debug_chain_kind(ctx._h, int(s.n_ddt)), m.iterations)
    ctx.close()
    lib.glio_debug_chain_fronts(4)
    return solve_hash(s, m), info


def device_steady(W, pts, seed):
    """keyframes 1..W of a W+1 stream with the prior the device marginalization of keyframe 0 leaves; also the first window and that prior"""
    stream = synth.make_window(W=W + 1, pts_per_scan=pts, with_gnss=True, seed=synth.SEED_BASE + seed)
    first = synth.sub_window(stream, 0, W)
    c0 = capi.Context(first.opts); c0.load_window(first, synth.analytic_correspondences(first))
    s0, _ = c0.solve(first.init); prior = c0.marginalize(s0); c0.close()
    win = synth.sub_window(stream, 1, W); win.prior = prior
    return win, synth.analytic_correspondences(win), prior


# ---- the steady window of test_hip_parity.py: its prior comes from the CPU oracle, the same for every build
from oracle import pyoracle as po
W = 5
long = synth.make_window(W=W + 1, pts_per_scan=600, with_gnss=True, seed=synth.SEED_BASE + 91)
first = synth.sub_window(long, 0, W)
prob0 = po.Problem(first, synth.analytic_correspondences(first), use_gnss=False, use_prior=False)
st0 = first.init.copy(); st0.n_ddt = 0
sol0, _ = prob0.solve(st0)
steady = synth.sub_window(long, 1, W); steady.prior = prob0.marginalize(sol0)
steady_corr = synth.analytic_correspondences(steady)

if not only_marg:
    for use_gnss in (True, False):
        for mode in (0, 1, 2, 3, 4):
            h, info = solved(steady, steady_corr, mode, use_gnss)
            print("steady W5 %s mode %d path/kind/iterations %s: %s" % ("gnss" if use_gnss else "no_gnss", mode, info, h))
    for Wf in (12, 13):
        win, corr, _ = device_steady(Wf, 300, 300 + Wf)
        for use_gnss in (True, False):
            far = state_for(win, use_gnss)
            far.trans = far.trans + np.random.default_rng(Wf).normal(0, 0.05, far.trans.shape)
            for fronts in (2, 4):
                lib.glio_debug_chain_fronts(fronts)
                ctx = capi.Context(win.opts); lib.glio_debug_set_solver(ctx._h, 1); ctx.load_window(win, corr, use_gnss=use_gnss)
                s, m = ctx.solve(far)
                used = lib.glio_debug_chain_fronts_used(ctx._h)
                ctx.close(); lib.glio_debug_chain_fronts(4)
                assert used == fronts, (Wf, use_gnss, fronts, used)
                print("W%d %s fronts %d iterations %d: %s" % (Wf, "gnss" if use_gnss else "no_gnss", used, m.iterations, solve_hash(s, m)))
    win, corr, _ = device_steady(28, 300, 328)
    h, info = solved(win, corr, 1, True)
    assert info[1] == 3, info                   # k_chain_solve<true>: the blocks in global memory
    print("W28 path/kind/iterations %s: %s" % (info, h))
    # the W = 4 window after a loop closure (tests/test_hip_post_loop.py): speed-bias priors, extended kept layout
    import marg_layout_restated as mr
    spec = importlib.util.spec_from_file_location("make_golden_post_loop", os.path.join(ROOT, "tests", "golden", "make_golden_post_loop.py"))
    gold = importlib.util.module_from_spec(spec); spec.loader.exec_module(gold)
    G = gold.load()
    win, corr = mr.scenario_window(4)
    ctx = capi.Context(win.opts); ctx.load_window(win, corr, use_gnss=False, use_prior=False)
    ctx.set_speed_bias_priors(mr.first_targets(win))
    st = win.init.copy(); st.n_ddt = 0
    s, m = ctx.solve(st)
    p = ctx.marginalize(gold.state_of(G, 4, 0, "sol", win.init))
    ctx.close()
    print("post-loop W4 solve: %s  prior n %d: %s" % (solve_hash(s, m), p["n"], prior_hash(p)))
    for n in (17, 123, 414):
        ctx = capi.Context(synth.make_window(W=28, pts_per_scan=64, with_gnss=False).opts)
        rng = np.random.default_rng(n)
        B = rng.normal(0, 1, (n, n))
        L = np.tril(B @ B.T / n + np.eye(n)).copy()
        b = rng.normal(0, 1, n)
        x = np.zeros(n)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc = lib.glio_debug_chol_solve(ctx._h, n, dp(L), dp(b), dp(x))
        ctx.close()
        print("chol_solve n %d rc %d: %s" % (n, rc, sha(x)))

# ---- marginalization under this process's GLIO_MARG_SPLIT: first window (no prior: Amm is rank deficient by 3, the Jacobi path), steady window (fast
# inverse), W = 61 (largest kept block), W = 2 after a loop closure (n = 15: the split form's scratch does not fit behind the work matrix, k_marg_schur
# runs whatever the switch says).  The library has no hook that reports the form; marg_form restates the host's choice: it mirrors the line
# `const size_t lwork = (size_t)(n + 1) * n + 2, need = 226 + (size_t)n + 2 + 1100, have = (size_t)(c->n_max + 1) * c->n_max;` of glio_launch_marginalize
# in solver_kernels.hip and its test `lwork + need <= have`; when that line changes, this one has to follow.
split = os.environ.get("GLIO_MARG_SPLIT", "1")


def marg_form(ctx):
    n = ctx.marginalize_size()[0]
    n_max = 15 * ctx.W + max(0, ctx.opts.max_ddt_epochs)
    fits = (n + 1) * n + 2 + 226 + n + 2 + 1100 <= (n_max + 1) * n_max
    return "three launches" if split != "0" and fits else ("one workgroup" if fits else "one workgroup (scratch does not fit)")


win, corr, p_first = device_steady(5, 600, 91)
ctx = capi.Context(win.opts); ctx.load_window(win, corr)
sol, _ = ctx.solve(win.init)
form = marg_form(ctx)
p_steady = ctx.marginalize(sol); ctx.close()
print("marg split %s W5 (%s) first window: %s  steady window: %s" % (split, form, prior_hash(p_first), prior_hash(p_steady)))
win = synth.make_window(W=61, pts_per_scan=256, with_gnss=False, seed=synth.SEED_BASE + 561, gnss_epoch_dt=0.1)
ctx = capi.Context(win.opts); ctx.load_window(win, synth.analytic_correspondences(win), use_prior=False)
sol, _ = ctx.solve(win.init.copy())
form = marg_form(ctx)
p = ctx.marginalize(sol); ctx.close()
print("marg split %s W61 (%s) n %d: %s" % (split, form, p["n"], prior_hash(p)))
import marg_layout_restated as mr
win, corr = mr.scenario_window(2)
ctx = capi.Context(win.opts); ctx.load_window(win, corr, use_gnss=False, use_prior=False)
ctx.set_speed_bias_priors(mr.first_targets(win))
st = win.init.copy(); st.n_ddt = 0
sol, _ = ctx.solve(st)
form = marg_form(ctx)
assert form == "one workgroup (scratch does not fit)", form
p = ctx.marginalize(sol); ctx.close()
print("marg split %s post-loop W2 (%s) n %d: %s" % (split, form, p["n"], prior_hash(p)))

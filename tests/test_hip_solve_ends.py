"""The two ends of glio_solve on the keyframe-chain path (GLIO_SOLVE_ENDS / glio_debug_solve_ends): the first k_linearize_all reads status and state
from the mapped host block instead of waiting for a staging launch, and a solve that ends in k_chain_step's state machine is published from the
LDS copies (finalize_lds).  Neither may change a bit: every case is solved with the new paths and with the old ones (mask 0: k_stage_in,
finalize()) in the same process and compared with == on the state arrays and every summary field.  256 points per keyframe: the paths under test
do not depend on the number of points."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from glio_amd import synth
from parity_checks import assert_pose_parity

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTS = 256


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def new_mask(hip):
    """the library's default: every new path on"""
    lib = hip.load()
    m = lib.glio_debug_solve_ends(0)
    lib.glio_debug_solve_ends(m)
    assert m != 0
    return m


def _steady(hip, W, seed):
    """keyframes 1..W of a W+1 stream with the prior the DEVICE marginalization of keyframe 0 leaves (block diagonal by keyframe: the chain step)"""
    stream = synth.make_window(W=W + 1, pts_per_scan=PTS, with_gnss=True, seed=synth.SEED_BASE + seed)
    first = synth.sub_window(stream, 0, W)
    c0 = hip.Context(first.opts)
    c0.load_window(first, synth.analytic_correspondences(first))
    s0, _ = c0.solve(first.init)
    prior = c0.marginalize(s0)
    c0.close()
    win = synth.sub_window(stream, 1, W)
    win.prior = prior
    return win, synth.analytic_correspondences(win)


@pytest.fixture(scope="module")
def steady20(hip):
    return _steady(hip, 20, 320)


@pytest.fixture(scope="module")
def steady12(hip):
    return _steady(hip, 12, 312)


def _start(win, use_gnss):
    st = win.init.copy()
    if not use_gnss:
        st.n_ddt = 0
    return st


def _far(st, sigma=0.4, seed=5):
    far = st.copy()
    far.trans = far.trans + np.random.default_rng(seed).normal(0, sigma, far.trans.shape)
    far.speed_bias = far.speed_bias + np.random.default_rng(seed + 1).normal(0, sigma / 2, far.speed_bias.shape)
    return far


def _key(s, m):
    return (s.trans.tobytes(), s.quat.tobytes(), s.speed_bias.tobytes(), s.rcv_ddt[:s.n_ddt].tobytes(), tuple(sorted(m.as_dict().items())))


def _fat_steps(hip, ctx):
    st = (C.c_longlong * 320)()
    hip.load().glio_debug_arrow_stamps(ctx._h, st)
    return int(st[300])


def _both(hip, new_mask, opts, win, corr, states, use_gnss=True, use_prior=True, before_solve=None):
    """the solves of `states`, one context per mask: [(state, summary)] under the new paths and under the old ones, and what the new run recorded"""
    lib = hip.load()
    res, info = {}, {}
    try:
        for name, mask in (("new", new_mask), ("old", 0)):
            lib.glio_debug_solve_ends(mask)
            ctx = hip.Context(opts)
            ctx.load_window(win, corr, use_gnss=use_gnss, use_prior=use_prior)
            out = []
            for k, st in enumerate(states):
                if before_solve:
                    before_solve(ctx, k)
                out.append(ctx.solve(st))
            res[name] = out
            info[name] = dict(path=int(lib.glio_debug_solver_path(ctx._h)), fat_steps=_fat_steps(hip, ctx), kind=int(lib.glio_debug_chain_kind(ctx._h, states[0].n_ddt)))
            ctx.close()
    finally:
        lib.glio_debug_solve_ends(new_mask)
    for k, (a, b) in enumerate(zip(res["new"], res["old"])):
        assert _key(*a) == _key(*b), (k, a[1].as_dict(), b[1].as_dict())
    return res["new"], info


@pytest.mark.parametrize("which,use_gnss", [("steady12", True), ("steady20", True), ("steady20", False)], ids=["W12_gnss", "W20_gnss", "W20_no_gnss"])
def test_device_prior_windows(hip, new_mask, request, which, use_gnss):
    """W = 12 is the smallest window with four fronts.  Every step of these solves is accepted and takes the fat helpers' products (slot 300 of the
    stamps counts them): the fast path is the one compared.  One solve against the oracle at test_hip_parity.py's tolerances."""
    win, corr = request.getfixturevalue(which)
    st = _start(win, use_gnss)
    assert st.n_ddt == (win.init.n_ddt if use_gnss else 0) and (st.n_ddt > 0) == use_gnss
    got, info = _both(hip, new_mask, win.opts, win, corr, [st, st], use_gnss=use_gnss)
    assert info["new"]["path"] == 2 and info["new"]["kind"] == 1, info          # k_chain_step: the launches this file is about
    (s, m), (s2, m2) = got
    assert _key(s, m) == _key(s2, m2)
    assert info["new"]["fat_steps"] == m.iterations + m2.iterations, info      # every group's step took the helpers' products
    assert info["old"]["fat_steps"] == info["new"]["fat_steps"]
    if which == "steady20" and use_gnss:
        from oracle import pyoracle as po
        so, mo = po.Problem(win, corr, use_gnss=use_gnss).solve(st)
        assert m.termination == mo.termination and m.iterations == mo.iterations and m.successful_steps == mo.successful_steps
        assert abs(m.final_cost - mo.final_cost) <= 1e-8 * abs(mo.final_cost)
        assert_pose_parity(s, so)
        assert np.abs(s.speed_bias - so.speed_bias).max() <= 1e-6 and np.abs(s.rcv_ddt[:st.n_ddt] - so.rcv_ddt[:st.n_ddt]).max() <= 1e-6


@pytest.mark.parametrize("use_gnss", [True, False], ids=["gnss", "no_gnss"])
def test_windows_without_a_prior(hip, new_mask, use_gnss):
    win = synth.make_window(W=20, pts_per_scan=PTS, with_gnss=True, with_prior=False, seed=synth.SEED_BASE + 321)
    corr = synth.analytic_correspondences(win)
    st = _start(win, use_gnss)
    got, info = _both(hip, new_mask, win.opts, win, corr, [st, _far(st), st], use_gnss=use_gnss, use_prior=False)
    assert _key(*got[0]) == _key(*got[2])


def test_rejected_steps(hip, new_mask, steady20):
    """A far start under a relative-decrease threshold above what this nearly quadratic problem reaches (the far start alone is never rejected with the
    default threshold -- the oracle says so for perturbations up to 50 m and 3 rad): most steps are rejected, the stored vectors are reused with the
    halved radius (`reuse`), and the step finds the helpers' speculative products built for a candidate that did not become the current point."""
    win, corr = steady20
    opts2 = copy.copy(win.opts)
    opts2.min_relative_decrease, opts2.max_iterations = 1.05, 30
    far = _far(_start(win, True))
    got, info = _both(hip, new_mask, opts2, win, corr, [far])
    m = got[0][1]
    assert info["new"]["path"] == 2
    assert m.successful_steps < m.iterations and m.iterations - m.successful_steps >= 2, m.as_dict()
    assert info["new"]["fat_steps"] < m.iterations, (info, m.as_dict())
    # ... and the whole solve is the oracle's: counts, termination, costs, final radius, gradient norm, state (tests/window_tr_cases.py's gates)
    import window_tr_cases as wc
    from oracle import pyoracle as po
    w2 = copy.copy(win)
    w2.opts = opts2
    so, mo = po.Problem(w2, corr).solve(far)
    wc.compare_with_oracle(got[0][0], m, so, mo, label="rejected steps, W = 20")


def test_start_at_the_optimum_and_one_iteration(hip, new_mask, steady20):
    """From the solved state the solve ends in the second group, with no step accepted.  max_iterations = 1: likewise, from anywhere;
    max_iterations = 0: the FIRST group's state machine ends it -- the state it publishes from LDS is the one a workgroup of the launch just before
    it copied in from the host block."""
    win, corr = steady20
    st = _start(win, True)
    got, _ = _both(hip, new_mask, win.opts, win, corr, [st])
    opt = got[0][0]
    got, info = _both(hip, new_mask, win.opts, win, corr, [opt, st, opt])
    m = got[0][1]
    assert m.iterations <= 1 and m.successful_steps == 0, m.as_dict()
    assert _key(*got[0]) == _key(*got[2])
    for mi in (1, 0):
        opts1 = copy.copy(win.opts)
        opts1.max_iterations = mi
        got, _ = _both(hip, new_mask, opts1, win, corr, [st, opt, _far(st)])
        assert got[0][1].iterations == mi
        if mi == 0:
            assert np.array_equal(got[2][0].trans, _far(st).trans)          # nothing moved: what came back is what the first group read


def test_back_to_back_solves_read_the_state_they_were_given(hip, new_mask, steady20):
    """40 solves alternating two initial states, nothing between them: a first group that read the previous call's block (or the result the
    previous call's reader left in it) would return the other state's solution."""
    win, corr = steady20
    a = _start(win, True)
    b = _far(a, 0.2, 11)
    got, _ = _both(hip, new_mask, win.opts, win, corr, [a, b] * 20)
    ka, kb = _key(*got[0]), _key(*got[1])
    assert ka != kb
    for k, r in enumerate(got):
        assert _key(*r) == (kb if k & 1 else ka), k


def test_solve_id_wrap(hip, new_mask, steady20):
    """the solve's tag wraps from 30000 to 1: the solves around the wrap return what the same solves returned before it"""
    win, corr = steady20
    lib = hip.load()
    a = _start(win, True)
    b = _far(a, 0.2, 11)

    def before(ctx, k):
        if k == 2:
            assert lib.glio_debug_set_solve_id(ctx._h, 29997) == 0          # the next solves carry 29998, 29999, 30000, 1, 2, 3
    got, _ = _both(hip, new_mask, win.opts, win, corr, [a, b] * 4, before_solve=before)
    for k, r in enumerate(got):
        assert _key(*r) == _key(*got[k & 1]), k


@pytest.fixture(scope="module")
def ab_script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("solve_ends_ab", os.path.join(ROOT, "scripts", "solve_ends_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("env", [{"GLIO_CHAIN_HELPERS": "0"}, {"GLIO_CHAIN_FAT": "0"}], ids=["helpers_off", "thin_helpers"])
def test_helpers_off_and_thin(hip, ab_script, env):
    """The helper switches are read once per process: scripts/solve_ends_ab.py solves under both masks in a process of its own.  Without the fat
    products the step builds its blocks itself -- the same bits under either mask, and the bits of this process, whose helpers are fat."""
    if not hasattr(test_helpers_off_and_thin, "ref"):
        test_helpers_off_and_thin.ref = ab_script.run()
    ref = test_helpers_off_and_thin.ref
    assert ref["new"]["path"] == 2 and ref["new"]["hashes"] == ref["old"]["hashes"] and ref["new"]["fat_steps"] > 0 and ref["new"]["rejected"] >= 2, ref
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "solve_ends_ab.py")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rows) == 1, out.stdout[-2000:] + out.stderr[-2000:]
    got = rows[0]
    assert got["new"]["path"] == 2 and got["new"]["fat_steps"] == 0 and got["old"]["fat_steps"] == 0, got
    assert got["new"]["hashes"] == got["old"]["hashes"] == ref["new"]["hashes"], (got, ref)

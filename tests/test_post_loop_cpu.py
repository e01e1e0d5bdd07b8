"""CPU side of the windows after a loop closure: the numpy restatement of the generalised marginalization (tests/marg_layout_restated.py) held to the
reference's own MarginalizationInfo -- live where the reference tree exists, and everywhere through tests/golden/post_loop_marg.npz -- for W = 2 .. 5: the
first window (speed-bias priors, no marginalization prior) and the chain of windows that takes the reference's extended output back as its prior.
Tolerances: what tests/test_hip_marg.py holds a marginalization root to (parity_checks.check_root: 1e-8 on J0^T J0 and J0^T r0, 1e-7 on |r0|^2)."""
import importlib.util
import os

import numpy as np
import pytest

import marg_layout_restated as mr
from glio_amd import ctypes_types as T
from oracle import pyoracle as po
from parity_checks import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_post_loop", os.path.join(HERE, "golden", "make_golden_post_loop.py"))
gold = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(gold)

SIZES = {2: 15, 3: 21, 4: 36, 5: 51}


@pytest.fixture(scope="module")
def G():
    return gold.load()


@pytest.fixture(scope="module")
def scen():
    return {W: mr.scenario_window(W) for W in mr.SHAPES}


def same_prior(a, b):
    """what the next window consumes of two roots of the same Schur complement, and the block tables"""
    assert a["n"] == b["n"]
    assert rel_err(a["S"], b["S"]) <= 1e-8
    assert np.linalg.norm(a["bs"] - b["bs"]) <= 1e-8 * np.linalg.norm(b["bs"])          # (against the whole vector: the extra blocks' share of it is zero)
    ra, rb = a["lin_res"] @ a["lin_res"], b["lin_res"] @ b["lin_res"]
    assert abs(ra - rb) <= 1e-7 * max(rb, 1e-30)
    for k in ("blk_slot", "blk_kind", "blk_idx"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["blk_x0"], b["blk_x0"])


def check_extras(out, W, state, first):
    """the kept speed-bias blocks of later keyframes: exactly diag(64, 64, 1, ..., 1), exactly uncoupled, linearised at the state's own bits; in the first
    window their share of J0^T r0 is zero (the factors are re-created at the state being marginalized)"""
    ns = mr.std_n(W)
    S = out["S"]
    for j in range((out["n"] - ns) // 9):
        c = ns + 9 * j
        blk = S[c:c + 9, c:c + 9]
        assert np.array_equal(blk, np.diag(mr.SBP_W ** 2)), (W, j, blk)
        rest = np.delete(S[c:c + 9], np.s_[c:c + 9], axis=1)
        assert not rest.any() and not np.delete(S[:, c:c + 9], np.s_[c:c + 9], axis=0).any()
        assert not (first and out["bs"][c:c + 9].any())
        b = 2 * (W - 1) + 1 + j
        assert out["blk_kind"][b] == T.BLK_SPEEDBIAS and out["blk_idx"][b] == c
        assert np.array_equal(out["blk_x0"][b], state.speed_bias[out["blk_slot"][b] + 1])


def test_speed_bias_prior_is_a_tiny_marginalization_prior():
    rng = np.random.default_rng(11)
    tg = rng.normal(size=(3, 9))
    x = [tg[k] + rng.normal(size=9) * 0.3 for k in range(3)]
    r, J = po.eval_marg(mr.synthetic_prior(tg), x)
    assert np.array_equal(r, np.concatenate([mr.SBP_W * (x[k] - tg[k]) for k in range(3)]))
    for k in range(3):
        want = np.zeros((27, 9)); want[9 * k:9 * k + 9] = np.diag(mr.SBP_W)
        assert np.array_equal(J[k], want)


def test_stacked_priors_add_up_in_the_oracle(small_window, small_corr):
    """the oracle with an ordinary prior AND the factors (two priors side by side) = the oracle with the ordinary prior + the factors' closed form"""
    win = small_window
    W = win.W
    st = win.init.copy(); st.n_ddt = 0
    st.speed_bias[:, :3] += 0.05
    tg = win.init.speed_bias[:W - 1]
    H0, g0, c0 = po.Problem(win, small_corr, use_gnss=False).linearize(st)
    H1, g1, c1 = po.Problem(mr.with_prior(win, mr.stack_priors(win.prior, mr.synthetic_prior(tg))), small_corr, use_gnss=False).linearize(st)
    for s in range(W - 1):
        i = np.arange(15 * s + 6, 15 * s + 15)
        d = st.speed_bias[s] - tg[s]
        H0[i, i] += mr.SBP_W ** 2; g0[i] += mr.SBP_W ** 2 * d; c0 += 0.5 * np.sum((mr.SBP_W * d) ** 2)
    assert rel_err(H1, H0) <= 1e-13 and rel_err(g1, g0) <= 1e-13 and abs(c1 - c0) <= 1e-13 * c0


@pytest.mark.parametrize("W", sorted(mr.SHAPES))
def test_restatement_matches_the_recorded_reference(G, scen, W):
    """first window and the whole chain, at the recorded states, each window with the REFERENCE's previous output as its prior"""
    win, corr = scen[W]
    n_prev = None
    for k in range(W):
        ref = gold.prior_of(G, W, k)
        sol = gold.state_of(G, W, k, "sol", win.init)
        if k == 0:
            assert ref["n"] == SIZES[W] == mr.expected_n(W)
            got = mr.marginalize(win, corr, sol, None, W - 1)
        else:
            assert ref["n"] == max(n_prev - 9, mr.std_n(W))                 # one speed-bias block fewer per window, back to the standard layout
            got = mr.marginalize(win, corr, sol, gold.prior_of(G, W, k - 1), 0)
        same_prior(got, ref)
        check_extras(got, W, sol, k == 0)
        check_extras(ref, W, sol, k == 0)
        n_prev = ref["n"]
    assert n_prev == mr.std_n(W)


@pytest.mark.parametrize("W", sorted(mr.SHAPES))
def test_recorded_reference_is_reproducible(G, scen, W):
    """where the reference tree exists: the committed file is what the generator writes, and the live reference agrees with the restatement"""
    from oracle import pyref
    if not os.path.isdir(os.path.join(pyref.REFERENCE, "GLIO", "include", "factors")):
        pytest.skip("no reference tree here: the committed vectors are used as they are")
    win, corr = scen[W]
    prob = po.Problem(win, corr, use_gnss=False, use_prior=False)
    for k in range(W):
        rec = gold.prior_of(G, W, k)
        sol = gold.state_of(G, W, k, "sol", win.init)
        prior_in = mr.synthetic_prior(sol.speed_bias[:W - 1]) if k == 0 else gold.prior_of(G, W, k - 1)
        out = mr.canonical(mr.reference_marginalize(win, prob, sol, prior_in), W)
        same_prior(out, rec)
        same_prior(mr.marginalize(win, corr, sol, None if k == 0 else prior_in, W - 1 if k == 0 else 0), out)
        # the recorded states are the oracle's solves of the same windows (to rounding: its sums are not ordered across threads)
        start = gold.state_of(G, W, k, "start", win.init)
        first = mr.synthetic_prior(mr.first_targets(win))
        again, summ = po.Problem(mr.with_prior(win, first if k == 0 else prior_in), corr, use_gnss=False).solve(start)
        assert summ.iterations == int(G["W%d_k%d_iterations" % (W, k)])
        assert np.abs(again.trans - sol.trans).max() <= 1e-9 and np.abs(again.speed_bias - sol.speed_bias).max() <= 1e-9


@pytest.mark.parametrize("W", sorted(mr.SHAPES))
def test_the_factors_move_the_solution(scen, W):
    """not a small error: the first window's speed/bias solution with and without the factors (the issue measured 0.35 .. 0.047 for W = 2 .. 5)"""
    win, corr = scen[W]
    st = win.init.copy(); st.n_ddt = 0
    with_f, m1 = po.Problem(mr.with_prior(win, mr.synthetic_prior(mr.first_targets(win))), corr, use_gnss=False).solve(st)
    without, m0 = po.Problem(win, corr, use_gnss=False, use_prior=False).solve(st)
    assert np.abs(with_f.speed_bias - without.speed_bias).max() > 1e-3

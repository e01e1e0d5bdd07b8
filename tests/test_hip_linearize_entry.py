"""The merged linearisation launch's entry form (glio_debug_linearize_entry; csrc/glio_switches.h, LINEARIZE_ENTRY): bit 0 the status record, the counts and the
roles' records asked for in one first round, bit 1 the prior by keyframe on the keyframe-chain path, bit 2 the K3 workgroups per keyframe from the roles'
own count.  No bit may change a bit: every buffer a later launch reads is compared with == against mask 0 in the same process, with the number of K3
partials per keyframe pinned (glio_debug_linearize_pin_nb) so that bit 2 does not regroup them.  256 points per keyframe unless a case is about counts."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

from glio_amd import synth
from parity_checks import assert_pose_parity, rel_err

pytestmark = pytest.mark.gpu
PTS = 256
PIN_NB = 5
WHAT = {0: "K3 partials", 1: "IMU blocks", 2: "GNSS blocks", 3: "clock-drift blocks", 4: "chain slices", 5: "prior g", 6: "prior cost", 7: "prior H"}
ALL_MASKS = list(range(8))


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    lib = capi.load()
    lib.glio_debug_linearize_buffer.restype = C.c_longlong
    return capi


@pytest.fixture(scope="module")
def default_mask(hip):
    lib = hip.load()
    m = lib.glio_debug_linearize_entry(0)
    lib.glio_debug_linearize_entry(m)
    assert m == 7
    return m


@pytest.fixture(autouse=True)
def _restore_mask(hip):
    yield
    hip.load().glio_debug_linearize_entry(7)


# ---------------------------------------------------------------------------------------------- hooks
def _launch(hip, ctx, st, which, use_status=1, done=0, pending=1):
    cs = st.c()
    nb = hip.load().glio_debug_linearize_launch(ctx._h, C.byref(cs), which, use_status, done, pending)
    assert nb > 0, hip.load().glio_last_error()
    return nb


def _buffer(hip, ctx, what, which, fill=-1):
    lib = hip.load()
    n = lib.glio_debug_linearize_buffer(ctx._h, what, which, None, C.c_longlong(0), -1)
    assert n >= 0
    if fill >= 0:
        assert lib.glio_debug_linearize_buffer(ctx._h, what, which, None, C.c_longlong(0), fill) == n
        return None
    out = np.zeros(max(n, 1), np.uint8)
    assert lib.glio_debug_linearize_buffer(ctx._h, what, which, out.ctypes.data_as(C.c_void_p), C.c_longlong(n), -1) == n
    return out[:n].tobytes()


def _prior_form(hip, ctx):
    out = (C.c_int32 * 4)()
    assert hip.load().glio_debug_prior_form(ctx._h, out) == 0
    return dict(n=out[0], span_ok=out[1], jac_exact=out[2], device_made=out[3])


def _key(s, m):
    return (s.trans.tobytes(), s.quat.tobytes(), s.speed_bias.tobytes(), s.rcv_ddt[:s.n_ddt].tobytes(), tuple(sorted(m.as_dict().items())))


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


# ---------------------------------------------------------------------------------------------- windows
_STREAMS = {}


def _stream(W, pts=PTS):
    """keyframes 0..W of one drive: window 0 is solved and marginalized, window 1 is the one under test"""
    if (W, pts) not in _STREAMS:
        long = synth.make_window(W=W + 1, pts_per_scan=pts, with_gnss=True, seed=synth.SEED_BASE + 700 + W)
        first, win = synth.sub_window(long, 0, W), synth.sub_window(long, 1, W)
        _STREAMS[(W, pts)] = (first, synth.analytic_correspondences(first), win, synth.analytic_correspondences(win))
    return _STREAMS[(W, pts)]


def _context(hip, W, prior, use_gnss, pts=PTS):
    """A context holding window 1 of the stream with the prior of the given kind; returns (ctx, window, correspondences).
    none: no prior.  device: the device's own marginalization of window 0, left where glio_marginalize_keep put it (solve, marginalize, next window).
    handed: the same marginalization read back and handed to glio_set_prior (bench.py's route).  dense: synth's dense prior (the arrow path)."""
    first, corr0, win, corr = _stream(W, pts)
    win = copy.copy(win)
    if prior == "dense":
        dense = synth.make_window(W=W, pts_per_scan=pts, with_gnss=True, with_prior=True, seed=synth.SEED_BASE + 730 + W)
        ctx = hip.Context(dense.opts)
        ctx.load_window(dense, synth.analytic_correspondences(dense), use_gnss=use_gnss)
        return ctx, dense, synth.analytic_correspondences(dense)
    ctx = hip.Context(win.opts)
    if prior == "none":
        win.prior = None
        ctx.load_window(win, corr, use_gnss=use_gnss, use_prior=False)
        return ctx, win, corr
    ctx.load_window(first, corr0, use_gnss=use_gnss, use_prior=False)
    s0, _ = ctx.solve(_start(first, use_gnss))
    if prior == "device":
        win.prior = ctx.marginalize(s0)           # (what the oracle is given; the context keeps its own copy below)
        ctx.marginalize_keep(s0)
        for k in range(W):
            ctx.set_correspondences(k, *corr[k])
        ctx.set_imu(win.preints)
        if use_gnss:
            ctx.set_gnss(win.frame, win.dd, win.dop)
        else:
            ctx.set_gnss(None, [], [])
        return ctx, win, corr
    assert prior == "handed"
    win.prior = ctx.marginalize(s0)
    ctx.close()
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, use_gnss=use_gnss)
    return ctx, win, corr


def _all_buffers(hip, ctx, which, has_prior, with_pH):
    whats = [0, 1, 2, 3, 4] + ([5, 6] if has_prior else []) + ([7] if has_prior and with_pH else [])
    return {w: _buffer(hip, ctx, w, which) for w in whats}


def _fill_all(hip, ctx, has_prior, byte):
    for which in (0, 1):
        for w in [0, 1, 2, 3, 4] + ([5, 6, 7] if has_prior else []):
            _buffer(hip, ctx, w, which, fill=byte)


# ---------------------------------------------------------------------------------------------- same bits, part by part
@pytest.mark.parametrize("use_gnss", [True, False], ids=["gnss", "no_gnss"])
@pytest.mark.parametrize("prior", ["none", "device", "handed", "dense"])
@pytest.mark.parametrize("W", [2, 3, 5, 20])
def test_every_mask_leaves_the_same_buffers(hip, default_mask, W, prior, use_gnss):
    """One launch as a solve's later groups queue it (behind a status record), for both candidate buffers and every subset of the bits: every buffer a
    later launch reads equals mask 0's byte for byte.  The buffers are filled with a pattern before every launch, so an entry that a form forgot to
    write shows.  pH is compared where the launch has to write it (the dense prior: arrow path)."""
    lib = hip.load()
    ctx, win, corr = _context(hip, W, prior, use_gnss)
    st = _start(win, use_gnss)
    st2 = _far(st, 0.05, 9)
    has_prior = prior != "none"
    kind = int(lib.glio_debug_chain_kind(ctx._h, st.n_ddt))
    if prior == "dense":
        assert kind != 1 or W < 5                              # the dense assembly follows the launch: pH is read (two or three keyframes: whatever the prior, a chain)
    elif W >= 5:
        assert kind == 1, (W, prior, kind)                     # k_chain_step: the launch this file is about
    if prior in ("device", "handed"):
        f = _prior_form(hip, ctx)
        assert f["span_ok"] == 1 and f["device_made"] == (prior == "device"), f
    assert lib.glio_debug_linearize_pin_nb(ctx._h, PIN_NB) == 0
    lib.glio_debug_linearize_entry(0)
    _launch(hip, ctx, st, 0)                                   # (the chain tables and their zeroed slices go up with the first launch)
    ref = {}
    for mask in ALL_MASKS:
        lib.glio_debug_linearize_entry(mask)
        for which, state in ((0, st), (1, st2)):
            _fill_all(hip, ctx, has_prior, 0xA5)
            assert _launch(hip, ctx, state, which) == PIN_NB
            got = _all_buffers(hip, ctx, which, has_prior, with_pH=(kind != 1))
            if mask == 0:
                ref[which] = got
                assert got[0] != bytes([0xA5]) * len(got[0])
                continue
            for w, b in got.items():
                assert b == ref[which][w], (W, prior, use_gnss, mask, which, WHAT[w])
    assert ref[0][0] != ref[1][0]
    ctx.close()


@pytest.mark.parametrize("prior", ["none", "device", "handed", "dense"])
@pytest.mark.parametrize("W", [5, 20])
def test_whole_solves_are_identical(hip, default_mask, W, prior):
    """iterations, termination and every returned double under each bit alone and all together, against mask 0 (partials per keyframe pinned)"""
    lib = hip.load()
    res = {}
    for mask in (0, 1, 2, 4, 7):
        lib.glio_debug_linearize_entry(mask)
        ctx, win, corr = _context(hip, W, prior, True)
        assert lib.glio_debug_linearize_pin_nb(ctx._h, PIN_NB) == 0
        st = _start(win, True)
        res[mask] = [_key(*ctx.solve(s)) for s in (st, _far(st), st)]
        ctx.close()
    for mask, r in res.items():
        assert r == res[0], (W, prior, mask)
        assert r[0] == r[2]


def test_unpinned_solve_is_repeatable_and_the_oracles(hip, default_mask):
    """Default switches, nothing pinned (the grouping of the K3 partials follows the roles' count): run to run identity, and the oracle's solve at
    tests/test_hip_parity.py's gates."""
    from oracle import pyoracle as po
    lib = hip.load()
    ctx, win, corr = _context(hip, 20, "handed", True)
    st = _start(win, True)
    a, b = ctx.solve(st), ctx.solve(st)
    assert _key(*a) == _key(*b)
    assert lib.glio_debug_solver_path(ctx._h) == 2
    ctx.close()
    so, mo = po.Problem(win, corr).solve(st)
    s, m = a
    assert m.termination == mo.termination and m.iterations == mo.iterations and m.successful_steps == mo.successful_steps
    assert abs(m.final_cost - mo.final_cost) <= 1e-8 * abs(mo.final_cost)
    assert_pose_parity(s, so)
    assert np.abs(s.speed_bias - so.speed_bias).max() <= 1e-6 and np.abs(s.rcv_ddt[:st.n_ddt] - so.rcv_ddt[:st.n_ddt]).max() <= 1e-6


# ---------------------------------------------------------------------------------------------- a launch that must not store
@pytest.mark.parametrize("prior", ["handed", "dense"])
@pytest.mark.parametrize("mask", [7, 0])
def test_a_launch_behind_a_finished_solve_stores_nothing(hip, default_mask, prior, mask):
    lib = hip.load()
    ctx, win, corr = _context(hip, 20, prior, True)
    st = _start(win, True)
    lib.glio_debug_linearize_entry(mask)
    _launch(hip, ctx, st, 0)
    for done, pending in ((1, 1), (0, 0), (1, 0)):
        for which in (0, 1):
            _fill_all(hip, ctx, True, 0x5A)
            _launch(hip, ctx, st, which, use_status=1, done=done, pending=pending)
            for w in range(8):
                for wh in (0, 1):
                    b = _buffer(hip, ctx, w, wh)
                    assert b == bytes([0x5A]) * len(b), (mask, done, pending, which, WHAT[w], wh)
    ctx.close()


# ---------------------------------------------------------------------------------------------- rejected steps
def test_rejected_steps(hip, default_mask):
    """tests/test_hip_solve_ends.py's construction: most steps are rejected, so the candidate buffer does not alternate launch by launch"""
    lib = hip.load()
    res = {}
    for mask in (0, 7):
        lib.glio_debug_linearize_entry(mask)
        ctx, win, corr = _context(hip, 20, "handed", True)
        assert lib.glio_debug_linearize_pin_nb(ctx._h, PIN_NB) == 0
        opts2 = copy.copy(win.opts)
        opts2.min_relative_decrease, opts2.max_iterations = 1.05, 30
        ctx.close()
        ctx = hip.Context(opts2)
        ctx.load_window(win, corr)
        assert lib.glio_debug_linearize_pin_nb(ctx._h, PIN_NB) == 0
        s, m = ctx.solve(_far(_start(win, True)))
        assert lib.glio_debug_solver_path(ctx._h) == 2
        assert m.iterations - m.successful_steps >= 2, m.as_dict()
        res[mask] = _key(s, m)
        ctx.close()
    assert res[7] == res[0]


# ---------------------------------------------------------------------------------------------- counts
def _ragged(corr, counts):
    return [tuple(np.ascontiguousarray(a[:n]) for a in c) for c, n in zip(corr, counts)]


def test_counts_by_keyframe_and_between_solves(hip, default_mask):
    """Keyframes with 0 residuals, 1 residual, a count that is no multiple of the workgroups' stride, counts that differ by keyframe -- and counts changed
    between two solves of one context: the second solve works with the new ones (the counts travel in the launch's arguments)."""
    from oracle import pyoracle as po
    lib = hip.load()
    first, corr0, win, corr = _stream(5, 2048)
    win = copy.copy(win)
    win.prior = None
    n_full = [len(c[2]) for c in corr]
    counts_a = [0, 1, 256 * 4 + 3, n_full[3] - 37, n_full[4]]
    counts_b = [n_full[0], 513, 1, 0, 777]
    st = _start(win, True)
    res = {}
    for mask in (0, 7):
        lib.glio_debug_linearize_entry(mask)
        ctx = hip.Context(win.opts)
        ctx.load_window(win, _ragged(corr, counts_a), use_prior=False)
        assert lib.glio_debug_linearize_pin_nb(ctx._h, 4) == 0
        bufs = []
        _launch(hip, ctx, st, 0)
        bufs.append(_buffer(hip, ctx, 0, 0))
        Ha, ga, ca = ctx.linearize(st)
        sa = _key(*ctx.solve(st))
        for k, c in enumerate(_ragged(corr, counts_b)):
            ctx.set_correspondences(k, *c)
        _launch(hip, ctx, st, 1)
        bufs.append(_buffer(hip, ctx, 0, 1))
        Hb, gb, cb = ctx.linearize(st)
        sb = _key(*ctx.solve(st))
        ctx.close()
        fresh = hip.Context(win.opts)
        fresh.load_window(win, _ragged(corr, counts_b), use_prior=False)
        assert lib.glio_debug_linearize_pin_nb(fresh._h, 4) == 0
        assert _key(*fresh.solve(st)) == sb
        fresh.close()
        assert sa != sb
        res[mask] = (bufs, Ha.tobytes(), ga.tobytes(), ca, sa, Hb.tobytes(), gb.tobytes(), cb, sb)
        if mask == 7:
            for counts, (H, g, c) in ((counts_a, (Ha, ga, ca)), (counts_b, (Hb, gb, cb))):
                Ho, go, co = po.Problem(win, _ragged(corr, counts)).linearize(st)
                assert abs(c - co) <= 1e-10 * abs(co) and rel_err(g, go) <= 1e-10 and rel_err(H, Ho) <= 1e-10
    assert res[7] == res[0]


# ---------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("W", [5, 20])
def test_linearisation_against_the_oracle(hip, default_mask, W):
    """default switches: the glio_linearize route (dense assembly behind the launch: every factor's H, g and cost) at test_hip_parity.py's 1e-10, and of the
    chain route's launch what this change computes anew -- the prior's g, its cost and its keyframe blocks in the chain slices (diagonal and towards the
    keyframe below) -- against the oracle's prior-only problem at the same 1e-10 relative error.  The K3 partials and the IMU / GNSS slices of the chain
    route are held to the oracle through the whole solves (test_unpinned_solve_is_repeatable_and_the_oracles) and to mask 0 bit for bit."""
    from oracle import pyoracle as po
    ctx, win, corr = _context(hip, W, "handed", True)
    st = _start(win, True)
    prob = po.Problem(win, corr)
    Ho, go, co = prob.linearize(st)
    Hh, gh, ch = ctx.linearize(st)
    assert abs(ch - co) <= 1e-10 * abs(co) and rel_err(gh, go) <= 1e-10 and rel_err(Hh, Ho) <= 1e-10
    # chain route: the prior's part alone, against the oracle's prior-only problem (g and cost are what the step adds in; H's entries are the slices')
    only = po.Problem(win, [tuple(a[:0] for a in c) for c in corr], use_imu=False, use_gnss=False)
    st0 = st.copy()
    st0.n_ddt = 0
    Hp, gp, cp = only.linearize(st0)
    nb = _launch(hip, ctx, st, 0)
    assert nb >= 4
    f = _prior_form(hip, ctx)
    np_ = f["n"]
    g = np.frombuffer(_buffer(hip, ctx, 5, 0), np.float64)
    c = np.frombuffer(_buffer(hip, ctx, 6, 0), np.float64)[0]
    pr = win.prior
    idx = []
    for b in range(len(pr["blk_slot"])):
        s, k, i0 = int(pr["blk_slot"][b]), int(pr["blk_kind"][b]), int(pr["blk_idx"][b])
        off = 15 * s + (0 if k == 0 else (3 if k == 1 else 6))
        for j in range(9 if k == 2 else 3):
            idx.append((i0 + j, off + j))
    assert len(idx) == np_
    gfull = np.zeros(15 * W)
    for pj, sj in idx:
        gfull[sj] = g[pj]
    assert abs(c - cp) <= 1e-10 * abs(cp) and rel_err(gfull, gp[:15 * W]) <= 1e-10
    # ... and the chain slices' diagonal blocks of the prior (source 4): lower triangles of the keyframes' 15 x 15
    sl = np.frombuffer(_buffer(hip, ctx, 4, 0), np.float64).reshape(W, 5, -1)
    Hc = np.zeros((15 * W, 15 * W))
    for s in range(W):
        for r in range(15):
            for cc in range(r + 1):
                Hc[15 * s + r, 15 * s + cc] = Hc[15 * s + cc, 15 * s + r] = sl[s, 4, r * (r + 1) // 2 + cc]
            if s + 1 < W:                      # slice s also holds the block of keyframe s + 1's rows against keyframe s's columns
                for cc in range(15):
                    Hc[15 * (s + 1) + r, 15 * s + cc] = Hc[15 * s + cc, 15 * (s + 1) + r] = sl[s, 4, 120 + r * 15 + cc]
    Href = np.zeros_like(Hc)                   # the oracle's prior H inside the block-tridiagonal band the chain keeps
    for s in range(W):
        for s2 in (s - 1, s, s + 1):
            if 0 <= s2 < W:
                Href[15 * s:15 * s + 15, 15 * s2:15 * s2 + 15] = Hp[15 * s:15 * s + 15, 15 * s2:15 * s2 + 15]
    assert rel_err(Hc, Href) <= 1e-10
    ctx.close()

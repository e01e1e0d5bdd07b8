"""The windows after a loop closure, restated in numpy: SpeedBiasPriorFactorAutoDiff (reference GLIO/include/factors/PriorFactor.h:10-40) as a tiny
marginalization prior, and the marginalization with the generalised kept layout (Estimator.cpp:2462-2607 with the factors of :2483-2518 re-created at
the state being marginalized), built like the Schur construction of tests/test_oracle_window.py from the oracle's single-factor evaluators.

Kept layout (columns of the next prior): [T1 Q1 SB1 | T2 Q2 | ... | T(W-1) Q(W-1)] as ever, then the speed/bias of every slot s >= 2 that carries a
speed-bias prior or has a speed-bias block in the installed prior, ascending, 9 columns each; every block is named s - 1.

A helper module of the tests (no test in it): tests/test_post_loop_cpu.py holds it to the reference's own MarginalizationInfo, tests/test_hip_post_loop.py
holds the device to it."""
import copy
import ctypes as C

import numpy as np

from glio_amd import ctypes_types as T
from glio_amd import synth
from oracle import pyoracle as po

SBP_W = np.array([8.0, 8.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])        # PriorFactor.h:19-27
SHAPES = {2: 300, 3: 400, 4: 400, 5: 500}                                 # W -> points per scan: every layout branch (none kept / merged / one / two extras)


def std_n(W):
    return 6 * (W - 1) + 9


def expected_n(W, n_slots=None):
    """columns kept by the first marginalization after a loop closure (factors on slots 0 .. n_slots-1, no prior)"""
    n_slots = W - 1 if n_slots is None else n_slots
    return std_n(W) + 9 * max(n_slots - 2, 0)


def synthetic_prior(targets):
    """The factors on slots 0 .. k-1 as ONE marginalization prior: J0 = blockdiag(diag(w)), r0 = 0, x0 = target.  MarginalizationFactor::Evaluate on it
    gives w o (x - target) and diag(w): the factor's residual and Jacobian."""
    targets = np.ascontiguousarray(targets, np.float64).reshape(-1, 9)
    k = len(targets)
    return dict(n=9 * k, lin_jac=np.diag(np.tile(SBP_W, k)), lin_res=np.zeros(9 * k), blk_slot=np.arange(k, dtype=np.int32),
                blk_kind=np.full(k, T.BLK_SPEEDBIAS, np.int32), blk_idx=(9 * np.arange(k)).astype(np.int32), blk_x0=targets.copy())


def stack_priors(a, b):
    """Two priors side by side (block diagonal), for the ORACLE only: it accumulates every block into the state columns it names, so the same parameter
    block may appear in both.  (The device takes the factors through glio_set_speed_bias_priors instead.)"""
    if a is None:
        return b
    if b is None:
        return a
    na, nb = a["n"], b["n"]
    J = np.zeros((na + nb, na + nb)); J[:na, :na] = a["lin_jac"]; J[na:, na:] = b["lin_jac"]
    return dict(n=na + nb, lin_jac=J, lin_res=np.r_[a["lin_res"], b["lin_res"]], blk_slot=np.r_[a["blk_slot"], b["blk_slot"]].astype(np.int32),
                blk_kind=np.r_[a["blk_kind"], b["blk_kind"]].astype(np.int32), blk_idx=np.r_[a["blk_idx"], np.asarray(b["blk_idx"]) + na].astype(np.int32),
                blk_x0=np.vstack([a["blk_x0"], b["blk_x0"]]))


def with_prior(win, prior):
    w = copy.copy(win)
    w.prior = prior
    return w


def extra_slots(W, prior, n_slots):
    have = set(int(s) for s, k in zip(prior["blk_slot"], prior["blk_kind"]) if k == T.BLK_SPEEDBIAS) if prior is not None else set()
    return [s for s in range(2, W) if s < n_slots or s in have]


def kept_blocks(W, prior, n_slots):
    """[(slot before the shift, kind, first column)] of the kept layout, and n"""
    blocks = [(1, T.BLK_TRANS, 0), (1, T.BLK_QUAT, 3), (1, T.BLK_SPEEDBIAS, 6)]
    for s in range(2, W):
        blocks += [(s, T.BLK_TRANS, 15 + 6 * (s - 2)), (s, T.BLK_QUAT, 18 + 6 * (s - 2))]
    n = std_n(W)
    for s in extra_slots(W, prior, n_slots):
        blocks.append((s, T.BLK_SPEEDBIAS, n)); n += 9
    return blocks, n


def _param(state, slot, kind):
    return [state.trans[slot], state.quat[slot], state.speed_bias[slot]][kind]


def schur_inputs(win, corr, state, prior, n_slots):
    """A, b over [slot 0 (15) | kept layout] from the per-factor evaluators: prior, speed-bias priors (zero residual: re-created at `state`), IMU (0, 1),
    every LiDAR factor with Huber; the reference's "drop the w column" convention for quaternion blocks (quirk Q8)."""
    W = win.W
    blocks, n = kept_blocks(W, prior, n_slots)
    m = 15
    off = {(0, T.BLK_TRANS): 0, (0, T.BLK_QUAT): 3, (0, T.BLK_SPEEDBIAS): 6}
    for s, kd, c in blocks:
        off[(s, kd)] = m + c
    A = np.zeros((m + n, m + n)); b = np.zeros(m + n)

    def add(r, Js, offs):
        for Ji, oi in zip(Js, offs):
            b[oi:oi + Ji.shape[1]] += Ji.T @ r
            for Jj, oj in zip(Js, offs):
                A[oi:oi + Ji.shape[1], oj:oj + Jj.shape[1]] += Ji.T @ Jj
    if prior is not None:
        params = [_param(state, s, k) for s, k in zip(prior["blk_slot"], prior["blk_kind"])]
        r, J = po.eval_marg(prior, params)
        add(r, [j[:, -3:] if j.shape[1] == 4 else j for j in J], [off[(int(s), int(k))] for s, k in zip(prior["blk_slot"], prior["blk_kind"])])
    for s in range(n_slots):
        add(np.zeros(9), [np.diag(SBP_W)], [off[(s, T.BLK_SPEEDBIAS)]])
    ps = T.GlioPreint(); synth.fill_preint(ps, win.preints[0])
    r, J = po.eval_imu(win.opts, ps, [state.trans[0], state.quat[0], state.speed_bias[0], state.trans[1], state.quat[1], state.speed_bias[1]])
    add(r, [J[0], J[1][:, 1:], J[2], J[3], J[4][:, 1:], J[5]], [off[(0, 0)], off[(0, 1)], off[(0, 2)], off[(1, 0)], off[(1, 1)], off[(1, 2)]])
    for s in range(W):
        for cp, pl, sc in zip(*corr[s]):
            rr, Jt, Jq = po.eval_lidar_plane(win.opts, cp, pl, sc, state.trans[s], state.quat[s])
            w = 1.0 if abs(rr) <= win.opts.huber_delta else win.opts.huber_delta / abs(rr)
            sw = np.sqrt(w)
            add(np.array([sw * rr]), [sw * Jt[None, :], sw * Jq[None, 1:]], [off[(s, 0)], off[(s, 1)]])
    return A, b, blocks, n


def marginalize(win, corr, state, prior=None, n_slots=0):
    """The next window's prior as a dict (glio_prior's fields + S = J0^T J0, bs = J0^T r0): MarginalizationInfo::Marginalize's arithmetic
    (MarginalizationFactor.cpp:128-202: Amm^+ with eps = 1e-8, the eigen root of the Schur complement)."""
    A, b, blocks, n = schur_inputs(win, corr, state, prior, n_slots)
    m = 15
    Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
    wv, V = np.linalg.eigh(Amm)
    Ainv = V @ np.diag(np.where(wv > 1e-8, 1 / np.where(wv > 1e-8, wv, 1.0), 0)) @ V.T
    S = A[m:, m:] - A[m:, :m] @ Ainv @ A[:m, m:]
    bs = b[m:] - A[m:, :m] @ Ainv @ b[:m]
    lam, U = np.linalg.eigh(0.5 * (S + S.T))
    keep = lam > 1e-8
    sq = np.where(keep, np.sqrt(np.where(keep, lam, 1.0)), 0.0)
    J0 = np.ascontiguousarray(sq[:, None] * U.T)
    r0 = np.where(keep, 1 / np.where(keep, sq, 1.0), 0.0) * (U.T @ bs)
    nb = len(blocks)
    x0 = np.zeros((nb, 9))
    for i, (s, kd, _) in enumerate(blocks):
        p = _param(state, s, kd)
        x0[i, :len(p)] = p
    return dict(n=n, lin_jac=J0, lin_res=r0, S=S, bs=bs, blk_slot=np.array([s - 1 for s, _, _ in blocks], np.int32),
                blk_kind=np.array([kd for _, kd, _ in blocks], np.int32), blk_idx=np.array([c for _, _, c in blocks], np.int32), blk_x0=x0)


def canonical(out, W):
    """A prior dict in ANY block order (the reference's is its unordered_map's) with its columns brought into the kept layout's order"""
    nb = len(out["blk_slot"])
    key = lambda i: (1, int(out["blk_slot"][i]), 0) if (out["blk_kind"][i] == T.BLK_SPEEDBIAS and out["blk_slot"][i] >= 1) else (0, int(out["blk_slot"][i]), int(out["blk_kind"][i]))
    order = sorted(range(nb), key=key)
    cols, idx, c = [], [], 0
    for i in order:
        sz = 9 if out["blk_kind"][i] == T.BLK_SPEEDBIAS else 3
        cols += list(range(out["blk_idx"][i], out["blk_idx"][i] + sz)); idx.append(c); c += sz
    assert c == out["n"] and sorted(cols) == list(range(c))
    J = np.ascontiguousarray(out["lin_jac"][:, cols])
    return dict(n=c, lin_jac=J, lin_res=out["lin_res"].copy(), S=J.T @ J, bs=J.T @ out["lin_res"], blk_slot=np.array([out["blk_slot"][i] for i in order], np.int32),
                blk_kind=np.array([out["blk_kind"][i] for i in order], np.int32), blk_idx=np.array(idx, np.int32), blk_x0=np.array([out["blk_x0"][i] for i in order]))


def reference_marginalize(win, prob, state, prior):
    """The reference's own MarginalizationInfo (the library built from the reference tree) over the same factor list; `prior` carries the speed-bias priors
    as synthetic_prior blocks.  Its entry point is called directly with buffers of 15 W rows and 3 W blocks: the result may be wider than the standard layout."""
    from oracle import pyref
    W = win.W
    nmax, nbmax = 15 * W, 3 * W
    lin_jac, lin_res = np.zeros(nmax * nmax), np.zeros(nmax)
    blk_slot, blk_kind, blk_idx = np.zeros(nbmax, np.int32), np.zeros(nbmax, np.int32), np.zeros(nbmax, np.int32)
    blk_x0 = np.zeros((nbmax, 9))
    nb = C.c_int32()
    ps = synth.prior_struct(prior) if prior is not None else None
    d = lambda a: np.ascontiguousarray(a, np.float64)
    qlb, tlb = d(list(win.opts.q_lb)), d(list(win.opts.t_lb))
    tr, qu, sb = d(state.trans), d(state.quat), d(state.speed_bias)
    n = pyref.lib().ref_marginalize(W, T.dptr(tr), T.dptr(qu), T.dptr(sb), T.dptr(qlb), T.dptr(tlb), C.c_double(win.opts.huber_delta), C.c_double(win.opts.gravity),
                                    T.iptr(prob.offset), T.fptr(prob.pts), T.fptr(prob.planes), T.dptr(prob.scores), C.byref(prob.imu[0]),
                                    C.byref(ps) if ps is not None else None, T.dptr(lin_jac), T.dptr(lin_res), T.iptr(blk_slot), T.iptr(blk_kind), T.iptr(blk_idx),
                                    T.dptr(blk_x0), C.byref(nb))
    k = nb.value
    return dict(n=n, lin_jac=lin_jac[:n * n].reshape(n, n).copy(), lin_res=lin_res[:n].copy(), blk_slot=blk_slot[:k].copy(), blk_kind=blk_kind[:k].copy(),
                blk_idx=blk_idx[:k].copy(), blk_x0=blk_x0[:k].copy())


# ------------------------------------------------------------------ the scenario the CPU test, the golden file and the GPU test share
def scenario_window(W):
    win = synth.make_window(W=W, pts_per_scan=SHAPES[W], with_prior=False, seed=synth.SEED_BASE + 7)
    return win, synth.analytic_correspondences(win)


def first_targets(win):
    """tmpSpeedBias[0 .. W-2] as the first window after the loop closure finds them (Estimator.cpp:2164-2176)"""
    return win.init.speed_bias[:win.W - 1].copy()


def start_of(prev_solution, k):
    """where window k >= 1 of the transient starts: the previous solution, moved (the window's content is reused; only the prior changes)"""
    st = prev_solution.copy()
    st.trans += 0.01 * k
    st.speed_bias[:, :3] += 0.02
    return st


def run_transient(win, corr, marg, steps=None):
    """W windows: the first with the speed-bias priors and no prior, window k >= 1 with the prior window k - 1 left.  marg(state, prior, n_slots) -> prior dict
    in the kept layout's order.  Every solve is the oracle's.  Returns [(start, solution, summary, prior_in, out)]."""
    W = win.W
    rows = []
    st0 = win.init.copy(); st0.n_ddt = 0
    first = synthetic_prior(first_targets(win))
    sol, summ = po.Problem(with_prior(win, first), corr, use_gnss=False, use_prior=True).solve(st0)
    out = marg(sol, synthetic_prior(sol.speed_bias[:W - 1]), W - 1)
    rows.append((st0, sol, summ, None, out))
    for k in range(1, W if steps is None else steps):
        prior = rows[-1][4]
        st = start_of(rows[-1][1], k)
        sol, summ = po.Problem(with_prior(win, prior), corr, use_gnss=False, use_prior=True).solve(st)
        rows.append((st, sol, summ, prior, marg(sol, prior, 0)))
    return rows

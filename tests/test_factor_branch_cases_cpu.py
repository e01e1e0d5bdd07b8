"""The cases of tests/factor_branch_cases.py do what they claim, and the oracle is right on them (CPU only).

  * every case takes the branch it is about -- counted in numpy from the factor records, independently of oracle and device;
  * no DD row lies within 1e-6 m of its threshold at the linearisation point or at any iterate of the oracle's solve (the weight jumps
    there: a rounding difference between device and oracle must not be able to flip a row) -- a condition on the seeds;
  * po.Problem.linearize equals the sum over the oracle's per-factor evaluators (eval_dd_psr, eval_doppler, eval_marg: the ones pinned to
    the reference's vectors by tests/test_golden_ref.py) assembled here in numpy."""
import numpy as np
import pytest

import factor_branch_cases as fc
from glio_amd import ctypes_types as T
from glio_amd import synth


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def cases():
    return fc.gnss_cases()


@pytest.fixture(scope="module")
def prior_windows(po):
    return dict(dense=fc.dense_prior_window(), steady=fc.steady_window(po))


def _is_sorted(keys):
    return all(a <= b for a, b in zip(keys, keys[1:]))


# ------------------------------------------------------------------------------------------------ each case takes its branch
def test_yaw_lever_case(cases):
    win = cases["yaw_lever"]
    assert win.frame.yaw_enu_local == fc.YAW
    frame_R = fc.r_ecef_local(fc.YAW).ravel()
    assert np.abs(frame_R - fc.r_ecef_local(0.0).ravel()).max() > 0.1
    own = [not np.array_equal(np.array(g.R_ecef_local), frame_R) for g in win.dop]
    assert sum(own) == len(win.dop) // 2 and sum(own) > 0, "half of the Doppler rows carry their own matrix"
    for l in range(win.W - 1):                                  # ... in every pair, next to rows with the frame's
        mine = [o for o, g in zip(own, win.dop) if g.slot_i == l]
        assert any(mine) and not all(mine)
    assert all(tuple(g.lever_arm) == fc.LEVER for g in win.dop) and len(win.dop) > 0


def test_masters_sizes_case(cases):
    win = cases["masters_sizes"]
    chunks = fc.dd_chunks(win)
    assert max(sum(len(c) for c in v) for v in chunks.values()) >= 9, "one pair needs two chunks"
    two = [v for v in chunks.values() if len(v) >= 2][0]
    for c in two:
        assert len({ns for ns, _ in c}) >= 4, "different sizes side by side in one chunk"
    seen = {(ns, ("first" if m == 0 else "last" if m == ns - 1 else "middle")) for c in two for ns, m in c}
    for ns in fc.N_SAT_CYCLE:
        assert (ns, "first") in seen and (ns, "last") in seen, ns
        assert ns == 2 or (ns, "middle") in seen, ns
    n_asym = 0
    for f in win.dd:
        nw = f.n_sat - 1
        Wm = np.array(f.weight[:nw * nw]).reshape(nw, nw)
        assert np.array_equal(Wm, np.tril(Wm))
        n_asym += int(nw > 1 and np.abs(Wm - Wm.T).max() > 0.05 * np.abs(Wm).max())
    assert n_asym == sum(f.n_sat > 2 for f in win.dd) > 0, "every weight block larger than 1 x 1 is far from symmetric"


def test_thresholds_case(cases):
    win = cases["thresholds"]
    assert {f.threshold for f in win.dd} == set(fc.THRESHOLDS)
    rows = fc.threshold_rows(win, win.init)
    above, below = sum(r[0] for r in rows), sum(r[1] for r in rows)
    mixed = sum(1 for r in rows if r[0] > 0 and r[1] > 0)
    print(f"thresholds: {above} rows above, {below} at or below, {mixed} factors with both")
    assert above > 0 and below > 0 and mixed > 0
    for thr in fc.THRESHOLDS[1:]:
        assert sum(r[0] for r, f in zip(rows, win.dd) if f.threshold == thr) > 0, thr
    assert sum(r[0] for r, f in zip(rows, win.dd) if f.threshold == 1e9) == 0
    # the generators' windows never get here: every other case keeps all rows below the threshold
    for name in ("yaw_lever", "ratios", "structure_sorted"):
        assert sum(r[0] for r in fc.threshold_rows(cases[name], cases[name].init)) == 0


def test_ratios_case(cases):
    win = cases["ratios"]
    assert {f.ratio for f in win.dd} == set(fc.RATIOS) and {g.ratio for g in win.dop} == set(fc.RATIOS)


def test_structure_cases(cases):
    srt, shf = cases["structure_sorted"], cases["structure_shuffled"]
    W = srt.W
    dd_key = lambda f: f.slot_i * W + f.slot_j
    dop_key = lambda g: (g.slot_i * W + g.slot_j, g.epoch)
    assert _is_sorted([dd_key(f) for f in srt.dd]) and _is_sorted([dop_key(g) for g in srt.dop])
    assert not _is_sorted([dd_key(f) for f in shf.dd]) and not _is_sorted([dop_key(g) for g in shf.dop]), "the handover must need the sort"
    # a stable sort of the shuffled handover is the sorted handover, record for record
    assert [bytes(f) for f in sorted(shf.dd, key=dd_key)] == [bytes(f) for f in srt.dd]
    assert [bytes(g) for g in sorted(shf.dop, key=dop_key)] == [bytes(g) for g in srt.dop]
    rev = cases["structure_reversed"]
    assert sum(f.slot_i == f.slot_j + 1 for f in rev.dd) > 0 and sum(g.slot_i == g.slot_j + 1 for g in rev.dop) > 0
    skip = cases["structure_skip"]
    assert sum((f.slot_i, f.slot_j) == (0, 2) for f in skip.dd) > 0 and sum((g.slot_i, g.slot_j) == (0, 2) for g in skip.dop) > 0
    split = cases["structure_split"]
    dd_pairs, dop_pairs = {(f.slot_i, f.slot_j) for f in split.dd}, {(g.slot_i, g.slot_j) for g in split.dop}
    assert len(dd_pairs - dop_pairs) > 0 and len(dop_pairs - dd_pairs) > 0 and len(dd_pairs & dop_pairs) > 0


def test_many_epochs_case(cases):
    win = cases["many_epochs"]
    per = fc.epochs_per_pair(win)
    assert max(per.values()) > 32 and max(per.values()) == 40
    assert 15 * win.W + win.init.n_ddt < 928          # GLIO_MAX_UNKNOWNS
    assert win.opts.max_ddt_epochs == win.init.n_ddt == sum(per.values())


@pytest.mark.parametrize("kind", ["dense", "steady"])
def test_prior_sign_cases(prior_windows, kind):
    win = prior_windows[kind]
    assert fc.negative_w_blocks(win.prior, win.init) == 0, "the generators stay on the w >= 0 side"
    want = dict(state=2, x0=1, both=3)
    for v in fc.PRIOR_VARIANTS:
        w = fc.prior_signs(win, v)
        assert fc.negative_w_blocks(w.prior, w.init) == want[v] > 0, v
        for s in range(win.W):
            assert np.allclose(synth.q2R(w.init.quat[s]), synth.q2R(win.init.quat[s]), atol=1e-15), "the same rotations"


@pytest.mark.parametrize("kind", ["dense", "steady"])
def test_negated_quaternions_are_the_same_problem_for_all_but_the_imu_factor(po, prior_windows, kind):
    """What the GPU test 'a state with -q equals the state with +q' rests on, shown on the oracle: prior + LiDAR + GNSS give the same cost, g, H
    (measured: exactly equal), while the reference's ImuFactor does not -- its attitude residual 2 vec(dq^-1 q_i^-1 q_j) changes sign with q_i,
    and the 15 x 15 information matrix couples it to the position / velocity / bias rows (measured on the dense-prior window: cost 5.1e-2
    relative, g 5.0e-2, H 1.1e-2 with the IMU factors alone).  tests/test_golden_ref.py holds that factor to the reference at quaternions of
    either sign, so this is the reference's behaviour; the device is compared with the oracle at -q WITH the IMU factors in
    test_prior_sign_linearisation, and with itself at +q without them."""
    base = prior_windows[kind]
    corr = synth.analytic_correspondences(base)
    for v in fc.PRIOR_VARIANTS:
        var = fc.prior_signs(base, v)
        Hp, gp, cp = po.Problem(base, corr, use_imu=False).linearize(base.init)
        Hn, gn, cn = po.Problem(var, corr, use_imu=False).linearize(var.init)
        print(f"{kind} {v} without IMU: cost {abs(cn - cp) / cp:.1e} g {_rel(gn, gp):.1e} H {_rel(Hn, Hp):.1e}")
        assert abs(cn - cp) <= 1e-12 * cp and _rel(gn, gp) <= 1e-10 and _rel(Hn, Hp) <= 1e-10
    var = fc.prior_signs(base, "state")
    only = dict(use_prior=False, use_gnss=False)
    ci, cn = po.Problem(base, corr, **only).linearize(base.init)[2], po.Problem(var, corr, **only).linearize(var.init)[2]
    print(f"{kind} state, IMU + LiDAR only: cost {abs(cn - ci) / ci:.1e}")
    assert abs(cn - ci) > 1e-6 * ci, "if the IMU factor were invariant, the GPU test should include it"


def test_batch_case():
    P = fc.batch_problem()
    assert P["K"] == 13 and P["band"] == 3 and P["frame"].yaw_enu_local == fc.YAW
    assert {f.n_sat for f in P["dd"]} == set(fc.N_SAT_CYCLE)
    assert {("first" if f.master == 0 else "last" if f.master == f.n_sat - 1 else "middle") for f in P["dd"]} == {"first", "middle", "last"}
    above = below = 0
    margin = np.inf
    for f in P["dd"]:
        a, thr = fc.dd_raw(f, P["frame"], P["init"][f.slot_i, :3], P["init"][f.slot_j, :3])
        assert thr == fc.BATCH_THRESHOLD
        above += int((a > thr).sum()); below += int((a <= thr).sum()); margin = min(margin, np.abs(a - thr).min())
    print(f"batch: {above} rows above the threshold, {below} at or below, margin {margin:.2e} m")
    assert above > 0 and below > 0 and margin > fc.THRESHOLD_MARGIN
    di, dj, _ = P["dq"]
    assert P["init"][fc.BATCH_NEGATED, 3] < 0 and np.all(np.delete(P["init"][:, 3], fc.BATCH_NEGATED) > 0)
    assert (di == fc.BATCH_NEGATED).sum() > 0 and (dj == fc.BATCH_NEGATED).sum() > 0, "the negated keyframe is on both sides of delta_q pairs"


# ------------------------------------------------------------------------------------------------ threshold margin
def _oracle_trial_points(po, win, corr):
    """The linearisation point and every trial point of the oracle's solve.  The solve evaluates one candidate per iteration and ends on the function
    tolerance with its last candidate evaluated but not taken; with function_tolerance = 0 the same run takes it and goes on, so the state after k
    iterations of that run, k = 1 .. iterations, is the k-th candidate -- provided no step is rejected, which the candidate costs recorded by the
    run with the window's own options confirm: they are the costs at these states."""
    import copy
    _, summ, hist = po.Problem(win, corr).solve_history(win.init)
    out = [win.init]
    for k in range(1, summ.iterations + 1):
        w = copy.copy(win)
        w.opts = T.GlioOpts.from_buffer_copy(win.opts)
        w.opts.max_iterations, w.opts.function_tolerance = k, 0.0
        st, sk = po.Problem(w, corr).solve(win.init)
        assert abs(sk.final_cost - hist[k - 1, 0]) <= 1e-12 * hist[k - 1, 0], ("not the trial point of iteration", k, sk.final_cost, hist[k - 1, 0])
        out.append(st)
    return out


def test_no_dd_row_sits_on_its_threshold(po, cases, prior_windows):
    """every window the GPU file linearises or solves: the GNSS cases, the two prior windows (they carry the generator's DD factors) and their
    sign variants"""
    wins = dict(cases)
    for kind, base in prior_windows.items():
        wins[f"prior_{kind}"] = base
        for v in fc.PRIOR_VARIANTS:
            wins[f"prior_{kind}_{v}"] = fc.prior_signs(base, v)
    worst = {}
    for name, win in wins.items():
        corr = synth.analytic_correspondences(win)
        its = _oracle_trial_points(po, win, corr)
        assert len(its) >= 3, name
        worst[name] = min(r[2] for st in its for r in fc.threshold_rows(win, st))
    print("smallest distance of a DD row to its threshold over the oracle's trial points [m]:", {k: f"{v:.2e}" for k, v in worst.items()})
    for name, v in worst.items():
        assert v > fc.THRESHOLD_MARGIN, (name, v)


def test_no_batch_dd_row_sits_on_its_threshold(po):
    """the batch problem over the trial points of the oracle's trust-region solve (the options of the GPU test), found as for the windows: the run with
    function_tolerance = 0 capped at k iterations ends on the k-th candidate of the real run, whose recorded cost it must reproduce"""
    P = fc.batch_problem()
    prob = po.BatchProblem(P["K"], P["band"], *P["con"], dq=P["dq"], dd=P["dd"], frame=P["frame"])
    _, _, full, hist = prob.solve2(P["init"], T.batch_tr_opts(max_iterations=30), want_history=True)
    assert full.iterations >= 3
    its = [P["init"]]
    for k in range(1, full.iterations + 1):
        o = T.batch_tr_opts(max_iterations=k)
        o.function_tolerance = 0.0
        x = prob.solve2(P["init"], o)[0]
        c = prob.linearize(x)[2]
        assert abs(c - hist[k - 1, 0]) <= 1e-12 * hist[k - 1, 0], ("not the trial point of iteration", k, c, hist[k - 1, 0])
        its.append(x)
    worst = min(np.abs(a - thr).min() for x in its for f in P["dd"] for a, thr in [fc.dd_raw(f, P["frame"], x[f.slot_i, :3], x[f.slot_j, :3])])
    print(f"batch: smallest distance of a DD row to its threshold over {len(its)} trial points {worst:.2e} m")
    assert worst > fc.THRESHOLD_MARGIN


# ------------------------------------------------------------------------------------------------ oracle vs its per-factor evaluators
def _plus_jacobian(q):
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]])          # d(dq * q)/d(dtheta) at 0, the local parameterisation of the solve


def assemble_from_evaluators(po, win, st, use_prior=True):
    """cost = 1/2 sum |r|^2 (Huber-corrected for the Doppler rows, Estimator.cpp:2335) and H = sum J^T J, g = sum J^T r over the GNSS factors and
    the prior, from the per-factor evaluators; unknowns [t3 theta3 v3 ba3 bg3] per keyframe, then the clock drifts"""
    W = win.W
    n = 15 * W + st.n_ddt
    H, g, cost = np.zeros((n, n)), np.zeros(n), 0.0
    yaw, anc = win.frame.yaw_enu_local, np.array(win.frame.anc_ecef)

    def add(r, J, cols):
        nonlocal cost
        H[np.ix_(cols, cols)] += J.T @ J
        g[cols] += J.T @ r
        cost += 0.5 * float(r @ r)

    t_cols = lambda s: list(range(15 * s, 15 * s + 3))
    sb_cols = lambda s: list(range(15 * s + 6, 15 * s + 15))
    if use_prior and win.prior is not None:
        pr = win.prior
        params, Ps, cols = [], [], []
        for s, kind in zip(pr["blk_slot"], pr["blk_kind"]):
            params.append([st.trans[s], st.quat[s], st.speed_bias[s]][kind])
            Ps.append(_plus_jacobian(st.quat[s]) if kind == T.BLK_QUAT else None)
            cols += t_cols(s) if kind == T.BLK_TRANS else (list(range(15 * s + 3, 15 * s + 6)) if kind == T.BLK_QUAT else sb_cols(s))
        r, J = po.eval_marg(pr, params)
        add(r, np.hstack([j if P is None else j @ P for j, P in zip(J, Ps)]), cols)
    delta = win.opts.doppler_huber_delta
    for f in win.dop:
        i, j = f.slot_i, f.slot_j
        r, J = po.eval_doppler(f, st.trans[i], st.speed_bias[i], st.trans[j], st.speed_bias[j], st.rcv_ddt, yaw, anc)
        Jrow = np.concatenate([np.ravel(b) for b in J])[None, :]
        cols = t_cols(i) + sb_cols(i) + t_cols(j) + sb_cols(j) + [15 * W + f.epoch]
        if r * r > delta * delta:                      # HuberLoss: rho = 2 d |r| - d^2, rho' = d / |r|, rho'' < 0 -> r and J scaled by sqrt(rho')
            sw = np.sqrt(delta / abs(r))
            H[np.ix_(cols, cols)] += (sw * Jrow).T @ (sw * Jrow)
            g[cols] += (sw * Jrow[0]) * (sw * r)
            cost += 0.5 * (2.0 * delta * abs(r) - delta * delta)
        else:
            add(np.array([r]), Jrow, cols)
    for f in win.dd:
        i, j = f.slot_i, f.slot_j
        r, (Ji, Jj) = po.eval_dd_psr(f, st.trans[i], st.trans[j], yaw, anc)
        add(r, np.hstack([Ji, Jj]), t_cols(i) + t_cols(j))
    return H, g, cost


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _no_lidar(win):
    e = (np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros(0))
    return [e] * win.W


EVALUATOR_GATE = 1.8e-15


def test_oracle_linearisation_is_the_sum_of_its_pinned_evaluators(po, cases, prior_windows):
    """Measured on the CPU (x86-64, numpy fp64 against the C oracle): over all GNSS cases and all prior sign variants, each at two linearisation
    points, the largest disagreement is 1.73e-16 on the cost (relative), 1.46e-16 on rel_err(g) and 1.69e-16 on rel_err(H), the position /
    velocity / clock-drift blocks on their own included -- the order of the sums, nothing else.  EVALUATOR_GATE is 10 x the largest of them,
    five orders inside the project's 1e-10."""
    assert EVALUATOR_GATE <= 1e-10
    worst = dict(cost=0.0, g=0.0, H=0.0)
    wins = list(cases.items())
    for kind, w in prior_windows.items():
        wins += [(f"prior_{kind}_{v}", fc.prior_signs(w, v)) for v in fc.PRIOR_VARIANTS]
    for name, win in wins:
        prob = po.Problem(win, _no_lidar(win), use_imu=False)
        moved = win.init.copy()
        moved.trans += 0.05; moved.speed_bias[:, :3] -= 0.03; moved.rcv_ddt += 0.3
        for st in (win.init, moved):
            Ho, go, co = prob.linearize(st)
            Hn, gn, cn = assemble_from_evaluators(po, win, st)
            d = dict(cost=abs(co - cn) / abs(cn), g=_rel(go, gn), H=_rel(Ho, Hn))
            print(f"{name}: cost {d['cost']:.1e} g {d['g']:.1e} H {d['H']:.1e}")
            # the blocks the GNSS factors touch (position, velocity, clock drift), on their own
            W = win.W
            pv = [15 * s + k for s in range(W) for k in (0, 1, 2, 6, 7, 8)] + list(range(15 * W, 15 * W + st.n_ddt))
            d["H"] = max(d["H"], _rel(Ho[np.ix_(pv, pv)], Hn[np.ix_(pv, pv)])); d["g"] = max(d["g"], _rel(go[pv], gn[pv]))
            for k in worst:
                worst[k] = max(worst[k], d[k])
                assert d[k] <= EVALUATOR_GATE, (name, k, d[k])
    print("largest oracle-vs-evaluator disagreement:", {k: f"{v:.2e}" for k, v in worst.items()})

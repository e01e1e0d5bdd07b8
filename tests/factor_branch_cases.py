"""Windows and batch problems at the inputs where the reference's GNSS and prior factors branch, for the window's own factor
kernels (gnss_block, prior_dx_M / prior_rg_block / prior_H_block, k_marg_assemble) and the batch stage's (k_small_eval): the
generators of glio_amd.synth and glio_amd.batch keep yaw_enu_local = 0, a zero lever arm, the frame's matrix on every Doppler row,
the highest satellite as master, ten satellites per factor, symmetric or identity weights, a threshold nothing exceeds, interior
ratios, sorted adjacent pairs and (x0^-1 q).w >= 0, so none of those branches is ever taken by a window or batch linearisation.

A case takes a window of synth.make_window(..., with_gnss=True) and returns a copy whose dd / dop / frame (or prior / init) are
rewritten.  Measurements come from the true trajectory exactly as synth._make_gnss draws them (1 m pseudorange noise, 0.1 m/s
Doppler noise) and are consistent with the case's yaw, lever arm and per-row matrix, so the residuals stay O(1).

No GPU and no oracle in here except steady_window(), which needs the oracle's marginalization for its prior."""
import copy
import math

import numpy as np

from glio_amd import ctypes_types as T
from glio_amd import synth

SEED = synth.SEED_BASE + 500
YAW = 0.7
LEVER = (0.3, -0.2, 0.5)
ROW_YAW_OFFSET = 0.2
N_SAT_CYCLE = (2, 3, 7, 19, 20)
THRESHOLDS = (1e9, 5.0, 0.5, 0.0)
RATIOS = (0.0, 1.0, 0.37)
THRESHOLD_MARGIN = 1e-6          # metres: no DD row may sit closer than this to its threshold (the weight is discontinuous there)


def rz(yaw):
    return np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]])


def r_ecef_local(yaw, anc=synth.ANCHOR_ECEF):
    return synth.ecef2rotation(anc) @ rz(yaw)


def master_cycle(k, ns):
    return (0, ns // 2, ns - 1)[k % 3]


def constellation(rng, n_sys, n):
    """n satellites per system on the 26 560 km shell between 15 and 85 degrees of elevation, as synth._make_gnss places them"""
    Ree = synth.ecef2rotation(synth.ANCHOR_ECEF)
    up = synth.ANCHOR_ECEF / np.linalg.norm(synth.ANCHOR_ECEF)
    east, north = Ree[:, 0], Ree[:, 1]
    out = []
    for _ in range(n_sys):
        pos, vel = [], []
        for _ in range(n):
            el, az = math.radians(rng.uniform(15, 85)), rng.uniform(0, 2 * math.pi)
            d = math.cos(el) * (math.sin(az) * east + math.cos(az) * north) + math.sin(el) * up
            b, c = synth.ANCHOR_ECEF @ d, synth.ANCHOR_ECEF @ synth.ANCHOR_ECEF - 26560e3 ** 2
            p = synth.ANCHOR_ECEF + (-b + math.sqrt(b * b - c)) * d
            tang = np.cross(p, rng.normal(size=3))
            pos.append(p); vel.append(3874.0 * tang / np.linalg.norm(tang))
        out.append((np.array(pos), np.array(vel)))
    return out


def difference_matrix(ns, master):
    D = np.zeros((ns - 1, ns))
    r = 0
    for i in range(ns):
        if i == master:
            continue
        D[r, master], D[r, i] = 1, -1
        r += 1
    return D


def whitening(kind, ns, master, snr):
    """'sym': the generator's (Estimator.cpp:2350-2357, symmetric); 'tri': L^-1 of the Cholesky factor L L^T = D Q^-1 D^T, i.e. a
    lower-triangular, non-symmetric W with W^T W = (D Q^-1 D^T)^-1; 'eye': the batch generator's identity"""
    if kind == "eye":
        return np.eye(ns - 1)
    D = difference_matrix(ns, master)
    Rm = D @ np.diag(1.0 / (snr / 50.0) ** 2) @ D.T
    if kind == "sym":
        return np.linalg.inv(np.sqrt(Rm))
    assert kind == "tri"
    return np.linalg.inv(np.linalg.cholesky(Rm))


def dd_factor(rng, spos, Pe, si, sj, ratio, ns, master=None, threshold=10.0, weight="sym", outliers=None, clock=1234.5, sigma=1.0):
    """One DD pseudorange factor over the first `ns` satellites of `spos`, the receiver at ECEF position Pe.  master None = the
    highest satellite (the generators' rule); outliers = {satellite index: metres added to the user pseudorange}."""
    f = T.GlioDdPsr()
    f.slot_i, f.slot_j, f.n_sat = si, sj, ns
    if master is None:
        up = synth.ANCHOR_ECEF / np.linalg.norm(synth.ANCHOR_ECEF)
        master = int(np.argmax([(sp - synth.ANCHOR_ECEF) @ up / np.linalg.norm(sp - synth.ANCHOR_ECEF) for sp in spos[:ns]]))
    f.master = master
    f.ratio, f.threshold = ratio, threshold
    f.station[:] = list(synth.STATION_ECEF)
    snr = rng.uniform(30, 50, ns)
    for i in range(ns):
        f.user_sat_pos[i][:] = list(spos[i]); f.ref_sat_pos[i][:] = list(spos[i])
        f.user_psr[i] = np.linalg.norm(spos[i] - Pe) + clock + rng.normal(0, sigma) + (outliers or {}).get(i, 0.0)
        f.ref_psr[i] = np.linalg.norm(spos[i] - synth.STATION_ECEF) + 77.0 + rng.normal(0, 0.3)
    Wm = whitening(weight, ns, master, snr)
    f.weight[:Wm.size] = list(Wm.ravel())
    return f


def doppler_row(rng, spos, svel, p_true, v_true, ddt, si, sj, ratio, epoch, lever, Rrow):
    g = T.GlioDoppler()
    g.slot_i, g.slot_j, g.epoch = si, sj, epoch
    g.ratio, g.var = ratio, 0.2
    g.sat_pos[:] = list(spos); g.sat_vel[:] = list(svel)
    g.sv_ddt = 1e-3 * rng.normal()
    g.lamda = synth.L1_LAMBDA
    Pe = Rrow @ (p_true + np.asarray(lever, float)) + synth.ANCHOR_ECEF          # what the factor forms from this row's own matrix and lever arm
    Ve = Rrow @ v_true
    d = spos - Pe
    eh = d / np.linalg.norm(d)
    sag = synth.EARTH_OMG / synth.LIGHT_SPEED * (svel[0] * Pe[1] + spos[0] * Ve[1] - svel[1] * Pe[0] - spos[1] * Ve[0])
    est = (svel - Ve) @ eh + sag + ddt - g.sv_ddt
    g.doppler = (-est + rng.normal(0, 0.1)) / synth.L1_LAMBDA
    g.lever_arm[:] = list(lever)
    g.R_ecef_local[:] = list(Rrow.ravel())
    return g


def std_dd(ns=5, **kw):
    return dict(dict(ns=ns, master=None, threshold=10.0, weight="sym", outliers=None), **kw)


def default_epochs(W, ratios=(0.75, 0.25), dd=None, n_sys=2):
    return [dict(si=l, sj=l + 1, ratio=r, dd=[dict(dd or std_dd()) for _ in range(n_sys)], dop=True) for l in range(W - 1) for r in ratios]


def with_gnss(base, epochs, yaw=0.0, lever=(0.0, 0.0, 0.0), row_yaw_offset=0.0, seed=SEED, dop_sats=4, n_sys=2):
    """A copy of `base` whose GNSS part is `epochs`: dicts(si, sj, ratio, dd = [dict(ns, master, threshold, weight, outliers)], dop).
    ratio is the weight of keyframe si; the epoch's time follows from it.  Only epochs with Doppler rows get a clock-drift unknown.
    Every second Doppler row carries a matrix built for yaw + row_yaw_offset, and is measured through it."""
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory()
    sats = constellation(rng, n_sys, T.GLIO_DD_MAX_SAT)
    Rloc = r_ecef_local(yaw)
    Rodd = r_ecef_local(yaw + row_yaw_offset)
    win = copy.copy(base)
    win.gt, win.init = base.gt.copy(), base.init.copy()
    win.frame = T.GlioGnssFrame()
    win.frame.yaw_enu_local = yaw
    win.frame.anc_ecef[:] = list(synth.ANCHOR_ECEF)
    win.dd, win.dop, ddt_true = [], [], []
    t0 = base.kf_times[0]
    row = 0
    for ep in epochs:
        si, sj, ratio = ep["si"], ep["sj"], float(ep["ratio"])
        te = ratio * base.kf_times[si] + (1.0 - ratio) * base.kf_times[sj]
        p_true, v_true = traj.pos(te), traj.vel(te)
        Pe = Rloc @ p_true + synth.ANCHOR_ECEF
        for sysid, spec in enumerate(ep["dd"]):
            spos = sats[sysid][0] + sats[sysid][1] * (te - t0)
            win.dd.append(dd_factor(rng, spos, Pe, si, sj, ratio, spec["ns"], spec["master"], spec["threshold"], spec["weight"], spec["outliers"]))
        if ep["dop"]:
            e = len(ddt_true)
            ddt_true.append(5.0 + 0.01 * e)
            for sysid in range(min(n_sys, 2)):
                spos = sats[sysid][0] + sats[sysid][1] * (te - t0)
                for i in range(dop_sats):
                    win.dop.append(doppler_row(rng, spos[i], sats[sysid][1][i], p_true, v_true, ddt_true[e], si, sj, ratio, e, lever, Rodd if row % 2 else Rloc))
                    row += 1
    n_ddt = len(ddt_true)
    for st in (win.gt, win.init):
        st.n_ddt = n_ddt
        st.rcv_ddt = np.zeros(max(n_ddt, 1))
    win.gt.rcv_ddt[:n_ddt] = ddt_true
    win.opts = T.GlioOpts.from_buffer_copy(base.opts)
    win.opts.max_ddt_epochs = n_ddt
    return win


def base_window(W=4, seed=SEED, **kw):
    return synth.make_window(W=W, pts_per_scan=512, with_gnss=True, seed=seed, **kw)


# ------------------------------------------------------------------ the GNSS cases
def yaw_lever(base):
    return with_gnss(base, default_epochs(base.W), yaw=YAW, lever=LEVER, row_yaw_offset=ROW_YAW_OFFSET, seed=SEED + 1)


def masters_sizes(base):
    """pair (1, 2): five epochs of three factors = 15 DD factors (chunks of 8 and 7) in which every n_sat of {2, 3, 7, 19, 20} meets every
    master position of {0, middle, n_sat - 1}; the other pairs continue the two cycles.  Lower-triangular weights."""
    k = 0
    epochs = []
    for l in range(base.W - 1):
        for r in ((0.9, 0.7, 0.5, 0.3, 0.1) if l == 1 else (0.6,)):
            dd = []
            for _ in range(3):
                ns = N_SAT_CYCLE[k % 5]
                dd.append(std_dd(ns, master=master_cycle(k, ns), weight="tri"))
                k += 1
            epochs.append(dict(si=l, sj=l + 1, ratio=r, dd=dd, dop=True))
    return with_gnss(base, epochs, seed=SEED + 2, n_sys=3)


def thresholds(base):
    """factor k has threshold THRESHOLDS[k % 4] and 10-40 m on two of its non-master satellites"""
    rng = np.random.default_rng(SEED + 30)
    epochs = default_epochs(base.W, dd=std_dd(7, master=3))
    k = 0
    for ep in epochs:
        for spec in ep["dd"]:
            spec["threshold"] = THRESHOLDS[k % 4]
            spec["outliers"] = {int(i): float(rng.uniform(10, 40)) for i in rng.choice([0, 1, 2, 4, 5, 6], 2, replace=False)}
            k += 1
    return with_gnss(base, epochs, seed=SEED + 3)


def ratios(base):
    per_pair = ((0.0, 0.37), (1.0, 0.37), (0.0, 1.0))
    epochs = [dict(si=l, sj=l + 1, ratio=r, dd=[std_dd(), std_dd()], dop=True) for l in range(base.W - 1) for r in per_pair[l % 3]]
    return with_gnss(base, epochs, seed=SEED + 4)


def group_preserving_shuffle(keys, rng):
    """A seeded permutation of range(len(keys)) that scatters the groups (equal key) among each other but keeps the members of one group in their
    relative order: glio_set_gnss sorts stably, so it hands the kernels exactly the sorted list, and the sums inside a pair / an epoch are
    taken in the same order -- which is what makes 'bit-identical to the sorted handover' a fair demand."""
    perm = rng.permutation(len(keys))
    out = perm.copy()
    for key in set(keys):
        pos = [p for p in range(len(perm)) if keys[perm[p]] == key]
        out[pos] = sorted(perm[pos])
    return out


def structure(base):
    """dict: sorted / shuffled (a), reversed (b: pair 1 listed as (2, 1)), skip (c: a pair (0, 2) instead of (1, 2)), split (d: pair 0 DD only,
    pair 1 Doppler only)"""
    out = {}
    out["sorted"] = with_gnss(base, default_epochs(base.W), seed=SEED + 5)
    sh = copy.copy(out["sorted"])
    rng = np.random.default_rng(SEED + 51)
    sh.dd = [out["sorted"].dd[k] for k in group_preserving_shuffle([(f.slot_i, f.slot_j) for f in sh.dd], rng)]
    sh.dop = [out["sorted"].dop[k] for k in group_preserving_shuffle([(f.slot_i, f.slot_j, f.epoch) for f in sh.dop], rng)]
    out["shuffled"] = sh
    ep = default_epochs(base.W)
    for e in ep:
        if (e["si"], e["sj"]) == (1, 2):
            e["si"], e["sj"], e["ratio"] = 2, 1, 1.0 - e["ratio"]
    out["reversed"] = with_gnss(base, ep, seed=SEED + 6)
    ep = default_epochs(base.W)
    for e in ep:
        if (e["si"], e["sj"]) == (1, 2):
            e["si"], e["sj"] = 0, 2
    out["skip"] = with_gnss(base, ep, seed=SEED + 7)
    ep = default_epochs(base.W)
    for e in ep:
        if e["si"] == 0:
            e["dop"] = False
        elif e["si"] == 1:
            e["dd"] = []
    out["split"] = with_gnss(base, ep, seed=SEED + 8)
    return out


def many_epochs():
    """W = 3, an epoch every 0.01 s: 40 epochs per pair, more than the GN_MAX_RUNS = 32 the Doppler role keeps in LDS; three satellites per system
    (15 W + n_ddt = 125 unknowns)"""
    base = base_window(W=3, seed=SEED + 9, gnss_epoch_dt=0.01)
    kt = base.kf_times
    epochs = []
    for te in np.arange(kt[0] + 0.005, kt[-1], 0.01):
        l = min(max(int(np.searchsorted(kt, te) - 1), 0), base.W - 2)
        epochs.append(dict(si=l, sj=l + 1, ratio=(kt[l + 1] - te) / (kt[l + 1] - kt[l]), dd=[std_dd(3), std_dd(3)], dop=True))
    return with_gnss(base, epochs, seed=SEED + 10, dop_sats=3)


def gnss_cases():
    """name -> window; built once per process by the test modules"""
    base = base_window()
    out = dict(yaw_lever=yaw_lever(base), masters_sizes=masters_sizes(base), thresholds=thresholds(base), ratios=ratios(base))
    for k, w in structure(base).items():
        out["structure_" + k] = w
    out["many_epochs"] = many_epochs()
    return out


# ------------------------------------------------------------------ numpy views of a case (independent of oracle and device)
def dd_raw(f, frame, Pi, Pj):
    """|est - obs| of the n_sat - 1 double differences of one factor, in the factor's row order, and the factor's threshold"""
    R = r_ecef_local(frame.yaw_enu_local, np.array(frame.anc_ecef))
    Pe = R @ (f.ratio * np.asarray(Pi) + (1.0 - f.ratio) * np.asarray(Pj)) + np.array(frame.anc_ecef)
    ns, m = f.n_sat, f.master
    us, rs = np.array(f.user_sat_pos)[:ns], np.array(f.ref_sat_pos)[:ns]
    rng_u, rng_r = np.linalg.norm(us - Pe, axis=1), np.linalg.norm(rs - np.array(f.station), axis=1)
    sd_est, sd_obs = rng_u - rng_r, np.array(f.user_psr)[:ns] - np.array(f.ref_psr)[:ns]
    keep = np.arange(ns) != m
    return np.abs((sd_est[keep] - sd_est[m]) - (sd_obs[keep] - sd_obs[m])), f.threshold


def threshold_rows(win, state):
    """per DD factor (rows above the threshold, rows at or below it, smallest distance of a row to the threshold)"""
    out = []
    for f in win.dd:
        a, thr = dd_raw(f, win.frame, state.trans[f.slot_i], state.trans[f.slot_j])
        out.append((int((a > thr).sum()), int((a <= thr).sum()), float(np.abs(a - thr).min())))
    return out


def epochs_per_pair(win):
    per = {}
    for g in win.dop:
        per.setdefault((g.slot_i, g.slot_j), set()).add(g.epoch)
    return {k: len(v) for k, v in per.items()}


def dd_chunks(win, chunk=8):
    """the n_sat and master values that sit side by side: per keyframe pair (sorted as glio_set_gnss sorts), per chunk of DD_CHUNK = 8 factors"""
    per = {}
    for f in win.dd:
        per.setdefault((f.slot_i, f.slot_j), []).append(f)
    return {k: [[(f.n_sat, f.master) for f in v[c:c + chunk]] for c in range(0, len(v), chunk)] for k, v in sorted(per.items())}


# ------------------------------------------------------------------ the prior's sign branch
PRIOR_VARIANTS = ("state", "x0", "both")


def negative_w_blocks(prior, state):
    """quaternion blocks of the prior with (x0^-1 q).w < 0 at `state`"""
    n = 0
    for b, (s, kind) in enumerate(zip(prior["blk_slot"], prior["blk_kind"])):
        if kind == T.BLK_QUAT:
            n += int(synth.qmul(synth.qconj(prior["blk_x0"][b, :4]), state.quat[s])[0] < 0)
    return n


def prior_signs(win, variant):
    """the state's quaternion negated on slots {0, 2} ('state'), the prior's x0 quaternion negated on slot 1 ('x0'), or both: the same rotations,
    hence the same problem, through the w < 0 branch of MarginalizationFactor.cpp:246-252"""
    assert variant in PRIOR_VARIANTS
    out = copy.copy(win)
    out.gt, out.init = win.gt.copy(), win.init.copy()
    out.prior = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in win.prior.items()}
    if variant in ("state", "both"):
        out.init.quat[[0, 2]] *= -1.0
    if variant in ("x0", "both"):
        b = [b for b in range(len(out.prior["blk_slot"])) if out.prior["blk_slot"][b] == 1 and out.prior["blk_kind"][b] == T.BLK_QUAT]
        assert len(b) == 1
        out.prior["blk_x0"][b[0], :4] *= -1.0
    return out


def dense_prior_window():
    """a caller-made dense prior"""
    return synth.make_window(W=4, pts_per_scan=512, with_gnss=True, with_prior=True, seed=SEED + 20)


def steady_window(po):
    """a prior that is itself a marginalization output (block diagonal by keyframe), as steady_window of tests/test_hip_parity.py builds it"""
    W = 4
    long = synth.make_window(W=W + 1, pts_per_scan=512, with_gnss=True, seed=SEED + 21)
    first = synth.sub_window(long, 0, W)
    prob0 = po.Problem(first, synth.analytic_correspondences(first), use_gnss=False, use_prior=False)
    st0 = first.init.copy(); st0.n_ddt = 0
    sol0, _ = prob0.solve(st0)
    win = synth.sub_window(long, 1, W)
    win.prior = prob0.marginalize(sol0)
    return win


# ------------------------------------------------------------------ the batch stage
BATCH_K, BATCH_BAND, BATCH_PER_KF = 13, 3, 100
BATCH_THRESHOLD = 6.0
BATCH_NEGATED = 5


def batch_problem(seed=SEED + 40):
    """K = 13 keyframes: plane constraints and delta_q pairs of the batch generators; DD factors at yaw 0.7 with lower-triangular weights, the master
    cycle, n_sat cycling through {2, 3, 7, 19, 20}, 10-40 m outliers under threshold 6; keyframe BATCH_NEGATED's quaternion negated in the initial poses"""
    from glio_amd import batch
    K, band = BATCH_K, BATCH_BAND
    gt, init = batch.make_poses(K, seed=seed, perturb=(0.08, 0.004))
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, BATCH_PER_KF, band, seed=seed)
    rng = np.random.default_rng(seed)
    odo = gt.copy()
    odo[:, :3] += rng.normal(0, 0.02, (K, 3))
    di, dj, dc = batch.delta_q_pairs(odo, 3)
    keep = np.abs(di - dj) <= band                   # (the walk of delta_q_pairs reaches up to six keyframes away: the ones inside the band of 3)
    dq = (di[keep], dj[keep], np.ascontiguousarray(dc[keep]))
    frame = T.GlioGnssFrame()
    frame.yaw_enu_local = YAW
    frame.anc_ecef[:] = list(synth.ANCHOR_ECEF)
    Rloc = r_ecef_local(YAW)
    sats = constellation(rng, 2, T.GLIO_DD_MAX_SAT)
    dd, n = [], 0
    for k in range(K - 1):
        ratio = float(rng.uniform(0.05, 0.95))
        Pe = Rloc @ (ratio * gt[k, :3] + (1 - ratio) * gt[k + 1, :3]) + synth.ANCHOR_ECEF
        for spos, _ in sats:
            ns = N_SAT_CYCLE[n % 5]
            m = master_cycle(n, ns)
            bad = {}
            if ns > 2 and n % 2 == 0:
                bad[(m + 1) % ns] = float(rng.uniform(10, 40))
            dd.append(dd_factor(rng, spos, Pe, k, k + 1, ratio, ns, m, BATCH_THRESHOLD, "tri", bad, clock=1234.5 + 0.3 * k))
            n += 1
    init = init.copy()
    init[BATCH_NEGATED, 3:] *= -1.0
    return dict(K=K, band=band, gt=gt, init=init, con=(ci, cj, cp.numpy(), nc.numpy(), score.numpy()), dq=dq, dd=dd, frame=frame)

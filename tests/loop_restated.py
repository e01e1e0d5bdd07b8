"""numpy restatement of the loop-closure registration (include/glio_hip.h, glio_loop_*: pcl::IterativeClosestPoint of PCL 1.8.1 as this project
restates it -- UNPINNED, PCL is not in the reference tree) and the cases the loop tests share.  Test infrastructure only: brute-force 1-NN in
float32, Umeyama in float64, PCL's convergence loop, the fitness.  Every float32 expression is written operation by operation in the order the
header states, so that numpy (which never fuses) rounds like the device code compiled without contraction."""
import math

import numpy as np

from glio_amd import synth

NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DEFAULTS = dict(max_corr_dist=30.0, max_iterations=100, transformation_eps=1e-6, fitness_eps=1e-6, abs_mse_eps=1e-12, min_correspondences=3)
DBL_MAX = float(np.finfo(np.float64).max)
F32 = np.float32


def nn_brute(cur, tgt, chunk=None):
    """exact nearest target point of every cur point: float32 d2 = (dx dx + dy dy) + dz dz, ties to the lowest index.  Returns (index, d2)."""
    cur = np.ascontiguousarray(cur, F32)[:, :3]
    tgt = np.ascontiguousarray(tgt, F32)[:, :3]
    n, m = len(cur), len(tgt)
    idx, d2 = np.zeros(n, np.int64), np.zeros(n, F32)
    chunk = chunk or max(1, min(n, (1 << 24) // max(m, 1)))
    tx, ty, tz = tgt[:, 0][None, :], tgt[:, 1][None, :], tgt[:, 2][None, :]
    for a in range(0, n, chunk):
        c = cur[a:a + chunk]
        dx = c[:, 0][:, None] - tx
        acc = dx * dx
        dy = c[:, 1][:, None] - ty
        acc = acc + dy * dy
        dz = c[:, 2][:, None] - tz
        acc = acc + dz * dz
        assert acc.dtype == F32
        k = np.argmin(acc, axis=1)                # (the first minimum: the lowest index)
        idx[a:a + chunk] = k
        d2[a:a + chunk] = acc[np.arange(len(c)), k]
    return idx, d2


def make_tree(tgt):
    """a k-d tree over the (fixed) target for nn_exact; None when scipy is missing (brute force then)"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    return cKDTree(np.ascontiguousarray(tgt, F32)[:, :3].astype(np.float64))


def nn_exact(cur, tgt, tree=None, k=8):
    """nn_brute's answer, bit for bit, without the n x m table: the k nearest by exact (double) distance are the candidates, the float32 rule picks among
    them, and the pick is CERTIFIED when it is below the k-th candidate's exact squared distance by more than float32 rounding can bridge (every other point
    is at least that far); whatever is not certified (more than k near-ties) goes to nn_brute."""
    cur = np.ascontiguousarray(cur, F32)
    tgt = np.ascontiguousarray(tgt, F32)
    if tree is None or len(tgt) <= k:
        return nn_brute(cur, tgt)
    dd, ii = tree.query(cur[:, :3].astype(np.float64), k=k, workers=8)
    ii = np.sort(ii, axis=1)                      # candidates by ascending index: argmin then returns the lowest index among equal d2
    t = tgt[ii]
    dx = cur[:, 0][:, None] - t[:, :, 0]
    acc = dx * dx
    dy = cur[:, 1][:, None] - t[:, :, 1]
    acc = acc + dy * dy
    dz = cur[:, 2][:, None] - t[:, :, 2]
    acc = acc + dz * dz
    assert acc.dtype == F32
    j = np.argmin(acc, axis=1)
    rows = np.arange(len(cur))
    idx, d2 = ii[rows, j].astype(np.int64), acc[rows, j]
    far = dd[:, -1] * dd[:, -1]
    bad = ~(d2.astype(np.float64) < far * (1.0 - 1e-5))
    if bad.any():
        bi, bd = nn_brute(cur[bad], tgt)
        idx[bad], d2[bad] = bi, bd
    return idx, d2


def correspondences(cur, tgt, max_corr_dist, tree=None):
    """step 1: (index or -1, d2 of the NEAREST point whatever the gate says)"""
    idx, d2 = nn_exact(cur, tgt, tree)
    keep = d2.astype(np.float64) <= float(max_corr_dist) * float(max_corr_dist)
    return np.where(keep, idx, -1).astype(np.int32), d2


def fit_rigid(s, t, reverse=False):
    """step 3: Umeyama without scale, fp64 (reverse: the same sums taken over the pairs in reverse order).  None when Sigma has rank < 2."""
    S, Tt = np.asarray(s, F32)[:, :3].astype(np.float64), np.asarray(t, F32)[:, :3].astype(np.float64)
    if reverse:
        S, Tt = S[::-1].copy(), Tt[::-1].copy()
    n = len(S)
    mu_s, mu_t = S.sum(axis=0) / n, Tt.sum(axis=0) / n
    ds, dt = S - mu_s, Tt - mu_t
    Sigma = np.array([[np.sum(dt[:, r] * ds[:, c]) for c in range(3)] for r in range(3)]) / n
    U, D, Vt = np.linalg.svd(Sigma)
    if not (D[0] > 0.0) or not (D[1] > 1e-6 * D[0]):
        return None
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    tr = mu_t - R @ mu_s
    T = np.eye(4, dtype=F32)
    T[:3, :3] = R.astype(F32)
    T[:3, 3] = tr.astype(F32)
    return T


def apply_T(T, cloud):
    """step 4 on the cloud: ((a x + b y) + c z) + d per row in float32, intensity kept"""
    T = np.asarray(T, F32)
    c = np.ascontiguousarray(cloud, F32)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    out = c.copy()
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    assert out.dtype == F32
    return out


def compose(T, F):
    """step 4 on the accumulated transform: T F in float32, ((t0 f0 + t1 f1) + t2 f2) + t3 f3"""
    T, F = np.asarray(T, F32), np.asarray(F, F32)
    out = np.zeros((4, 4), F32)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((T[r, 0] * F[0, c] + T[r, 1] * F[1, c]) + T[r, 2] * F[2, c]) + T[r, 3] * F[3, c]
    return out


def convergence_state(T, iterations, mse, prev_mse, o):
    """step 5, in DefaultConvergenceCriteria's order"""
    cosa = 0.5 * (((float(T[0, 0]) + float(T[1, 1])) + float(T[2, 2])) - 1.0)
    tsq = (float(T[0, 3]) * float(T[0, 3]) + float(T[1, 3]) * float(T[1, 3])) + float(T[2, 3]) * float(T[2, 3])
    if iterations >= o["max_iterations"]:
        return ITERATIONS
    if cosa >= 1.0 - o["transformation_eps"] and tsq <= o["transformation_eps"]:
        return TRANSFORM
    if abs(mse - prev_mse) < o["abs_mse_eps"]:
        return ABS_MSE
    if abs(mse - prev_mse) / prev_mse < o["fitness_eps"]:
        return REL_MSE
    return NOT_CONVERGED


def fitness(cur, tgt, tree=None):
    """step 6: mean squared 1-NN distance of every point, no cap, summed in double"""
    _, d2 = nn_exact(cur, tgt, tree)
    return float(d2.astype(np.float64).sum() / len(d2))


def round_of(cur, tgt, o, reverse=False, tree=None):
    """one round from `cur`: dict(idx, d2, n_corr, mse, T or None, no_corr, rank_deficient)"""
    idx, d2 = correspondences(cur, tgt, o["max_corr_dist"], tree)
    keep = idx >= 0
    n = int(keep.sum())
    kd = d2[keep].astype(np.float64)
    if reverse:
        kd = kd[::-1].copy()
    out = dict(idx=idx, d2=d2, n_corr=n, mse=float(kd.sum() / n) if n else 0.0, T=None, no_corr=n < o["min_correspondences"], rank_deficient=False)
    if out["no_corr"]:
        return out
    out["T"] = fit_rigid(cur[keep], np.asarray(tgt, F32)[idx[keep]], reverse)
    out["rank_deficient"] = out["T"] is None
    return out


def icp(src, tgt, reverse=False, keep_rounds=False, **kw):
    """the whole of glio_loop_align.  Returns dict(converged, state, iterations, fitness, transform, last_n_corr, last_mse, rank_deficient, cur[, rounds])."""
    o = dict(DEFAULTS)
    o.update(kw)
    cur = np.ascontiguousarray(src, F32).reshape(-1, 4).copy()
    tgt = np.ascontiguousarray(tgt, F32).reshape(-1, 4)
    final = np.eye(4, dtype=F32)
    tree = make_tree(tgt)
    prev_mse, iterations, state, converged, rank_def = DBL_MAX, 0, NOT_CONVERGED, False, False
    n_corr, mse, rounds = 0, 0.0, []
    while True:
        r = round_of(cur, tgt, o, reverse, tree)
        n_corr, mse = r["n_corr"], r["mse"]
        if keep_rounds:
            rounds.append(r)
        if r["no_corr"]:
            state, converged = NO_CORRESPONDENCES, False
            break
        if r["rank_deficient"]:
            state, converged, rank_def = NOT_CONVERGED, False, True
            break
        cur = apply_T(r["T"], cur)
        final = compose(r["T"], final)
        iterations += 1
        state = convergence_state(r["T"], iterations, mse, prev_mse, o)
        if state != NOT_CONVERGED:
            converged = True
            break
        prev_mse = mse
    out = dict(converged=converged, state=state, iterations=iterations, fitness=fitness(cur, tgt, tree), transform=final, last_n_corr=n_corr, last_mse=mse,
               rank_deficient=rank_def, cur=cur)
    if keep_rounds:
        out["rounds"] = rounds
    return out


# ------------------------------------------------------------------ comparing transforms: the project's pose gates
def pose_error(Ta, Tb):
    """(translation difference in m, rotation angle between the two in rad)"""
    Ta, Tb = np.asarray(Ta, np.float64), np.asarray(Tb, np.float64)
    dR = Ta[:3, :3].T @ Tb[:3, :3]
    ang = math.atan2(math.sqrt((dR[2, 1] - dR[1, 2]) ** 2 + (dR[0, 2] - dR[2, 0]) ** 2 + (dR[1, 0] - dR[0, 1]) ** 2) / 2.0, (np.trace(dR) - 1.0) / 2.0)
    return float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), abs(ang)


# ------------------------------------------------------------------ cases
CENTRE = np.array([80.0, 0.0, 2.0])


def target_cloud(seed=20261017, n_raw=15000, radius=30.0):
    """the scene within `radius` of CENTRE, voxel-averaged at 0.4 m, float32 [n][4] (intensity = a per-point number that plays no part)"""
    rng = np.random.default_rng(seed)
    pts, _ = synth.sample_scene(synth.make_scene(), n_raw, rng, centre=CENTRE, radius=radius)
    ds = synth.voxel_average(pts, 0.4).astype(F32)
    return np.ascontiguousarray(np.c_[ds, (np.arange(len(ds)) % 97).astype(F32)], F32)


def known_motion(yaw=0.03, pitch=0.01, roll=-0.005, shift=(0.5, -0.3, 0.1)):
    """the 4x4 (float64) that moves a point about CENTRE: R (p - c) + c + shift"""
    M = np.eye(4)
    M[:3, :3] = synth.euler_R(yaw, pitch, roll)
    M[:3, 3] = CENTRE - M[:3, :3] @ CENTRE + np.asarray(shift, float)
    return M


def known_answer_case(seed=20261017, n_raw=15000):
    """target; source = the EXACT subset of the target within 15 m of CENTRE, moved by known_motion (float32); the transform ICP has to find
    (the inverse of the motion, float64)"""
    tgt = target_cloud(seed, n_raw)
    sub = tgt[np.linalg.norm(tgt[:, :3].astype(np.float64) - CENTRE, axis=1) < 15.0]
    M = known_motion()
    src = sub.copy()
    src[:, :3] = (sub[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F32)
    return np.ascontiguousarray(src, F32), tgt, np.linalg.inv(M)


def independent_pair(seed=20261018):
    """independently sampled submaps of the same place, ~9 k source / ~32 k target points (point-to-point ICP slides along the corridor on these:
    no known answer, restatement against device only)"""
    rng = np.random.default_rng(seed)
    scene = synth.make_scene()
    a, _ = synth.sample_scene(scene, 45000, rng, centre=CENTRE, radius=18.0)
    b, _ = synth.sample_scene(scene, 460000, rng, centre=CENTRE, radius=52.0)
    M = known_motion(yaw=0.02, pitch=0.004, roll=-0.003, shift=(0.3, -0.2, 0.05))
    src = synth.voxel_average(a @ M[:3, :3].T + M[:3, 3], 0.4).astype(F32)
    tgt = synth.voxel_average(b, 0.4).astype(F32)
    return np.ascontiguousarray(np.c_[src, np.zeros(len(src), F32)], F32), np.ascontiguousarray(np.c_[tgt, np.zeros(len(tgt), F32)], F32)

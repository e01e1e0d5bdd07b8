"""A numpy restatement of the batch stage's selected inversion (include/glio_batch_cov.h), the fixed list of cases its tests run, and the gate both
the restatement and the device go through.  It knows nothing of the library or the oracle: a dense H comes in, blocks come out.

The recursion.  The K keyframes (B unknowns each) are grouped into super-blocks of sbk keyframes, the last one padded with identity keyframes: H is then
block tridiagonal with M x M blocks, M = sbk B.  Odd-even elimination: a level eliminates every other active node p between its active neighbours
a < p < b, A_pp = L L^T, U_a = A_ap L^-T, U_b = A_bp L^-T; the kept nodes take A_aa -= U_a U_a^T, A_bb -= U_b U_b^T and the new coupling
A_ba = -U_b U_a^T.  Down the same tree, last level first, with T_a = U_a L^-1, T_b = U_b L^-1:
    Sigma_pa = -T_a^T Sigma_aa - T_b^T Sigma_ba        Sigma_pb = -T_a^T Sigma_ab - T_b^T Sigma_bb
    Sigma_pp = L^-T L^-1 - Sigma_pa T_a - Sigma_pb T_b    (a root: L^-T L^-1)
Sigma_ab was produced when the first of a, b went: after p the two are adjacent.  (The device pre-eliminates the inner speed / bias blocks of the
15-state problem first; here they stay in their super-block -- the same matrix, another order.)"""
import numpy as np

EPS = np.finfo(np.float64).eps
GUARD = 1e-6          # 8 n kappa_s eps must stay below this for a gate to say something: the anchored problems (measured at most 2.9e-9)
GUARD_GNSS = 1e-4     # the same for the 15-state problem with DD pseudoranges and no anchor (kappa_s ~ 3.8e7, bound at most 5.1e-5)
FLOOR_FACTOR = 100    # pose-only + GNSS (kappa_s ~ 6e9): the device is held to 100 x the restatement's own scaled error against np.linalg.inv


class NotPositiveDefinite(Exception):
    def __init__(self, keyframe):
        super().__init__(f"not positive definite (keyframe {keyframe})")
        self.keyframe = keyframe


def cases():
    """family: 'pose' (planes + delta_q, B = 6) or 'imu' (+ the ImuFactor chain, B = 15); gnss: DD pseudoranges present; band 12 with the chain is the
    end-windows form of test_imu_chain_under_the_references_end_windows_band_12.  K: 5 one super-block, 7 two, 13 three with a ragged last, 48 exact,
    50 nine ragged (band 6), 61.  Anchors: 0, K - 1, inner to a super-block, in the ragged last super-block; -1 only with GNSS, or to be refused."""
    c = []
    def add(family, K, band, gnss, anchor, expect="gate"):
        c.append(dict(name=f"{family}_K{K}_b{band}_{'gnss' if gnss else 'nognss'}_a{anchor}", family=family, K=K, band=band, gnss=gnss, anchor=anchor, expect=expect))
    add("pose", 5, 6, False, 0)
    add("pose", 7, 6, False, 6)          # K - 1, the ragged last super-block
    add("pose", 13, 6, False, 3)         # inner to super-block 0
    add("pose", 48, 6, False, 47)
    add("pose", 50, 12, False, 49)       # M = 72; ragged last
    add("pose", 61, 12, False, 0)
    add("imu", 5, 6, False, 2)           # a keyframe whose speed / bias block is pre-eliminated
    add("imu", 7, 6, False, 0)
    add("imu", 13, 6, False, 12)         # ragged last
    add("imu", 48, 6, False, 20)         # inner
    add("imu", 50, 6, False, 49)
    add("imu", 50, 12, False, 0)         # 12-keyframe super-blocks, 90 x 90 nodes
    add("imu", 61, 12, False, 60)        # the one keyframe of the last super-block
    add("imu", 13, 6, True, -1, "gate_gnss")
    add("imu", 48, 6, True, -1, "gate_gnss")
    add("imu", 50, 12, True, -1, "gate_gnss")
    add("imu", 61, 6, True, 30, "gate_gnss")          # GNSS and an anchor together
    add("pose", 13, 6, True, -1, "floor")
    add("pose", 50, 6, True, -1, "floor")
    add("pose", 13, 6, False, -1, "singular")
    add("imu", 13, 6, False, -1, "singular")
    return c


def free_mask(K, B, anchor):
    free = np.ones(K * B, bool)
    if anchor >= 0:
        free[anchor * B:anchor * B + 6] = False
    return free


def selected_inverse(H, K, B, sbk, anchor=-1):
    """(diag [K][B][B], next [K-1][B][B]) of inv(H) with the anchor's six pose rows and columns left out (reported as zeros)"""
    H = np.asarray(H, np.float64)
    n = K * B
    free = free_mask(K, B, anchor)
    d = np.diag(H).copy()
    bad = free & ~((d > 0) & np.isfinite(d))
    if bad.any():
        raise NotPositiveDefinite(int(np.flatnonzero(bad)[0] // B))
    sc = np.where(free, 1.0 / np.sqrt(np.where(free, d, 1.0)), 0.0)
    S = (K + sbk - 1) // sbk
    M = sbk * B
    A = np.eye(S * M)
    A[:n, :n] = H * sc[:, None] * sc[None, :]
    fixed = np.flatnonzero(~free)
    A[fixed, fixed] = 1.0
    blk = lambda i, j: A[i * M:(i + 1) * M, j * M:(j + 1) * M].copy()
    D = [blk(i, i) for i in range(S)]
    edge = {(i, i + 1): blk(i + 1, i) for i in range(S - 1)}          # (lo, hi): A[hi][lo], rows hi
    act, levels, fac = list(range(S)), [], {}
    while act:
        gone = act[0::2]
        for pos in range(0, len(act), 2):
            p = act[pos]
            a = act[pos - 1] if pos > 0 else -1
            b = act[pos + 1] if pos + 1 < len(act) else -1
            dp = np.diag(D[p])
            try:
                L = np.linalg.cholesky(D[p])
            except np.linalg.LinAlgError:
                raise NotPositiveDefinite(min(p * sbk, K - 1))
            if not np.all(np.isfinite(L)) or not np.all(np.diag(L) > 0) or not np.all(np.isfinite(dp)):
                raise NotPositiveDefinite(min(p * sbk, K - 1))
            Ua = np.linalg.solve(L, edge[(a, p)]).T if a >= 0 else None            # A_ap L^-T = (L^-1 A_pa)^T, A_pa = edge (rows p)
            Ub = np.linalg.solve(L, edge[(p, b)].T).T if b >= 0 else None          # A_bp L^-T
            fac[p] = (L, Ua, Ub, a, b)
        for pos in range(0, len(act), 2):
            p = act[pos]
            L, Ua, Ub, a, b = fac[p]
            if a >= 0:
                D[a] = D[a] - Ua @ Ua.T
            if b >= 0:
                D[b] = D[b] - Ub @ Ub.T
            if a >= 0 and b >= 0:
                edge[(a, b)] = -Ub @ Ua.T
        levels.append(gone)
        act = act[1::2]
    Sig, cross = {}, {}          # cross[(lo, hi)]: Sigma[lo][hi], rows lo
    for gone in reversed(levels):
        for p in gone:
            L, Ua, Ub, a, b = fac[p]
            W = np.linalg.solve(L, np.eye(M))
            Spp = W.T @ W
            if a >= 0:
                Ta = Ua @ W
            if b >= 0:
                Tb = Ub @ W
            if a >= 0:
                Spa = -Ta.T @ Sig[a]
                if b >= 0:
                    Spa = Spa - Tb.T @ cross[(a, b)].T
            if b >= 0:
                Spb = -Tb.T @ Sig[b]
                if a >= 0:
                    Spb = Spb - Ta.T @ cross[(a, b)]
            if a >= 0:
                Spp = Spp - Spa @ Ta
                cross[(a, p)] = Spa.T
            if b >= 0:
                Spp = Spp - Spb @ Tb
                cross[(p, b)] = Spb
            Sig[p] = Spp
    diag = np.zeros((K, B, B)); nxt = np.zeros((max(K - 1, 0), B, B))
    for k in range(K):
        s, l = divmod(k, sbk)
        sk = sc[k * B:(k + 1) * B]
        blk_ = np.tril(Sig[s][l * B:(l + 1) * B, l * B:(l + 1) * B])
        diag[k] = (blk_ + np.tril(blk_, -1).T) * (sk[:, None] * sk[None, :])
        if k + 1 < K:
            s2, l2 = divmod(k + 1, sbk)
            src = Sig[s][l * B:(l + 1) * B, l2 * B:(l2 + 1) * B] if s2 == s else cross[(s, s2)][l * B:(l + 1) * B, l2 * B:(l2 + 1) * B]
            nxt[k] = src * (sk[:, None] * sc[(k + 1) * B:(k + 2) * B][None, :])
    return diag, nxt


def reference_blocks(H, K, B, anchor=-1):
    """the same blocks from np.linalg.inv of H with the anchor's rows and columns deleted; also (kappa_s of the Jacobi-scaled reduced H, its size)"""
    H = np.asarray(H, np.float64)
    free = np.flatnonzero(free_mask(K, B, anchor))
    Hr = H[np.ix_(free, free)]
    d = np.sqrt(np.diag(Hr))
    Hs = Hr / d[:, None] / d[None, :]
    kappa = float(np.linalg.cond(0.5 * (Hs + Hs.T)))
    full = np.zeros_like(H)
    full[np.ix_(free, free)] = np.linalg.inv(Hr)
    diag = np.stack([full[k * B:(k + 1) * B, k * B:(k + 1) * B] for k in range(K)])
    nxt = np.stack([full[k * B:(k + 1) * B, (k + 1) * B:(k + 2) * B] for k in range(K - 1)]) if K > 1 else np.zeros((0, B, B))
    return diag, nxt, kappa, len(free)


def scaled_error(got_diag, got_next, want_diag, want_next, H):
    """|| S (got - want) S ||_F / || S want S ||_F over the union of the blocks, S = diag(sqrt(H_kk))"""
    K, B = got_diag.shape[0], got_diag.shape[1]
    s = np.sqrt(np.abs(np.diag(H))).reshape(K, B)
    num = den = 0.0
    for k in range(K):
        w = s[k][:, None] * s[k][None, :]
        num += np.sum((w * (got_diag[k] - want_diag[k])) ** 2); den += np.sum((w * want_diag[k]) ** 2)
    for k in range(K - 1):
        w = s[k][:, None] * s[k + 1][None, :]
        num += np.sum((w * (got_next[k] - want_next[k])) ** 2); den += np.sum((w * want_next[k]) ** 2)
    return float(np.sqrt(num / den))


def assert_blocks_within_bound(got_diag, got_next, H, anchor, name, guard=GUARD):
    """covariance_cases.assert_within_bound's form on the union of the returned blocks: scaled error <= 8 n kappa_s eps, and the bound itself below `guard`
    (the test cannot pass vacuously).  Returns (error, bound, kappa_s)."""
    K, B = got_diag.shape[0], got_diag.shape[1]
    want_diag, want_next, kappa, n = reference_blocks(H, K, B, anchor)
    err = scaled_error(got_diag, got_next, want_diag, want_next, H)
    bound = 8 * n * kappa * EPS
    print(f"{name}: n {n}, kappa_s {kappa:.4e}, scaled error {err:.2e}, bound {bound:.2e}")
    assert bound < guard, (name, kappa, bound)
    assert err <= bound, (name, err, bound)
    return err, bound, kappa

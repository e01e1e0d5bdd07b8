"""glio_pgraph_covariance_all (include/glio_pgraph_cov.h) restated in numpy: the plan a solve makes from segment_nodes and the loops, the block elimination
in the device's order (segment interiors from the left with the spike to the left separator, then the separator system on its band + full-row pattern), and
the two recurrences of the selected inversion -- backwards over the separator factor, then down every segment.  Built on pose_graph_restated.Graph; it never
imports the product and the product never imports it.

`wrong` switches in one deliberate mistake each (tests/test_pose_graph_cov_restated.py shows that each is refused):
    "no_spike"      the down-sweep forgets the coupling to the left separator
    "sign"          Sigma_{i,N} = +Y' Sigma_{N,N}
    "outside_zero"  the separator inversion keeps the band alone: what the full rows hold of Z is read as zero"""
import math

import numpy as np


def default_segment_nodes(n_nodes):
    return min(255, max(4, int(math.floor(math.sqrt(n_nodes) + 0.5))))


def make_plan(n_nodes, loops, segment_nodes=0):
    """loops: [(i, j)].  Separators: node 0, the last node, every loop endpoint, and a node after every segment_nodes interior nodes; a separator that is the
    later end of a loop keeps a full row from the earliest separator it is linked to."""
    seg = segment_nodes if segment_nodes > 0 else default_segment_nodes(n_nodes)
    forced = sorted({0, n_nodes - 1} | {int(v) for lp in loops for v in lp[:2]})
    sep = []
    for f, node in enumerate(forced):
        if f > 0:
            sep.extend(range(forced[f - 1] + seg + 1, node, seg + 1))
        sep.append(node)
    at = {node: k for k, node in enumerate(sep)}
    lo = list(range(len(sep)))
    for lp in loops:
        a, b = at[int(lp[0])], at[int(lp[1])]
        lo[max(a, b)] = min(lo[max(a, b)], min(a, b))
    w_blk = [k for k in range(len(sep)) if lo[k] < k]
    return dict(sep=sep, w_blk=w_blk, w_lo=[lo[k] for k in w_blk], segment_nodes=seg)


def rowset(plan, b, band_only=False):
    """the scalar rows that a column of separator block b touches: block b, block b + 1, the full-row separators from b + 2 on that have begun"""
    S = len(plan["sep"])
    blocks = [b] + ([b + 1] if b + 1 < S else [])
    if not band_only:
        blocks += [w for w, lo in zip(plan["w_blk"], plan["w_lo"]) if w >= b + 2 and lo <= b]
    return np.concatenate([np.arange(6 * k, 6 * k + 6) for k in blocks])


def blk(M, i, j):
    return M[6 * i:6 * i + 6, 6 * j:6 * j + 6]


def covariance_all(H, plan, wrong=None):
    """H: the dense J^T J [6N][6N].  Returns (diag [N][6][6], next [N - 1][6][6], dict(min_pivot, max_pivot))."""
    sep = plan["sep"]
    S, N = len(sep), H.shape[0] // 6
    piv = []
    YC, YE, Dinv = {}, {}, {}
    A = np.zeros((6 * S, 6 * S))
    for a in range(S):
        for b in range(a + 1):
            blk(A, a, b)[:] = blk(H, sep[a], sep[b])
    # ---- the segments, each from the left
    for k in range(S - 1):
        sL, sR = sep[k], sep[k + 1]
        if sR - sL < 2:
            continue
        D, E = blk(H, sL + 1, sL + 1).copy(), blk(H, sL + 1, sL).copy()
        S_LL = np.zeros((6, 6))
        for i in range(sL + 1, sR):
            C = blk(H, i, i + 1)
            Lc = np.linalg.cholesky(D)
            piv.extend(np.diag(Lc) ** 2)
            solve = lambda B: np.linalg.solve(Lc.T, np.linalg.solve(Lc, B))
            YC[i], YE[i], Dinv[i] = solve(C), solve(E), solve(np.eye(6))
            S_LL -= E.T @ YE[i]
            if i + 1 < sR:
                D, E = blk(H, i + 1, i + 1) - C.T @ YC[i], -C.T @ YE[i]
            else:
                blk(A, k, k)[:] += S_LL
                blk(A, k + 1, k)[:] += (-E.T @ YC[i]).T
                blk(A, k + 1, k + 1)[:] += -C.T @ YC[i]
    # ---- the separator system: right-looking Cholesky on the pattern, then Z = A^-1 on the same pattern, columns backwards
    n = 6 * S
    band_only = wrong == "outside_zero"
    L = np.tril(A)
    ldiag = np.zeros(n)
    for k in range(n):
        b = k // 6
        I = rowset(plan, b)[k - 6 * b + 1:]
        assert L[k, k] > 0, ("pivot", k)
        ldiag[k] = math.sqrt(L[k, k])
        L[I, k] /= ldiag[k]
        L[np.ix_(I, I)] -= np.tril(np.outer(L[I, k], L[I, k]))
    assert not np.any(np.tril(L, -1)[~pattern_mask(plan)]), "fill outside the pattern"
    piv.extend(ldiag ** 2)
    Z = np.zeros((n, n)) if band_only else np.full((n, n), np.nan)           # NaN: an entry read before it was written shows
    for k in range(n - 1, -1, -1):
        b = k // 6
        I = rowset(plan, b, band_only)[k - 6 * b + 1:]
        Z[I, k] = -(Z[np.ix_(I, I)] @ L[I, k]) / ldiag[k]
        Z[k, I] = Z[I, k]
        Z[k, k] = 1.0 / ldiag[k] ** 2 - L[I, k] @ Z[I, k] / ldiag[k]
    # ---- down every segment
    diag, nxt = np.zeros((N, 6, 6)), np.zeros((max(N - 1, 0), 6, 6))
    sgn = 1.0 if wrong == "sign" else -1.0
    for k in range(S):
        diag[sep[k]] = blk(Z, k, k)
        if k + 1 >= S:
            break
        sL, sR = sep[k], sep[k + 1]
        NN, NL, LL = blk(Z, k + 1, k + 1), blk(Z, k + 1, k), blk(Z, k, k)
        for i in range(sR - 1, sL, -1):
            ye = np.zeros((6, 6)) if wrong == "no_spike" else YE[i]
            IN = sgn * (YC[i] @ NN + ye @ NL.T)
            IL = sgn * (YC[i] @ NL + ye @ LL)
            ii = Dinv[i] - IN @ YC[i].T - IL @ ye.T
            nxt[i], diag[i] = IN, np.tril(ii) + np.tril(ii, -1).T
            NN, NL = diag[i], IL
        nxt[sL] = NL.T
    return diag, nxt, dict(min_pivot=float(min(piv)), max_pivot=float(max(piv)))


def pattern_mask(plan):
    """[6S][6S] bool: the strictly lower entries the factor stores"""
    S = len(plan["sep"])
    m = np.zeros((6 * S, 6 * S), bool)
    for r in range(S):
        first = 0 if r in plan["w_blk"] else max(r - 1, 0)
        m[6 * r:6 * r + 6, 6 * first:6 * r + 6] = True
    return np.tril(m, -1)


def dense_blocks(H):
    """(diag, next) of np.linalg.inv(H)"""
    N = H.shape[0] // 6
    Hi = np.linalg.inv(H)
    return np.array([blk(Hi, i, i) for i in range(N)]), np.array([blk(Hi, i, i + 1) for i in range(N - 1)]).reshape(max(N - 1, 0), 6, 6)


def block_errors(diag, nxt, want_diag, want_next):
    """(largest error of a diagonal block, of a neighbour block), each relative to the largest entry of the diagonal blocks involved"""
    top = np.abs(want_diag).reshape(len(want_diag), -1).max(axis=1)
    ed = (np.abs(diag - want_diag).reshape(len(top), -1).max(axis=1) / top).max()
    en = 0.0
    if len(want_next):
        en = (np.abs(nxt - want_next).reshape(len(top) - 1, -1).max(axis=1) / np.maximum(top[:-1], top[1:])).max()
    return float(ed), float(en)


def normal_matrix(g, x):
    _, J = g.linearize(np.asarray(x, float))
    return J.T @ J


# ------------------------------------------------------------------------------------------------------------------------------------ the scenes of both test files
def arc(n, seed, radius=40.0, turn=0.6):
    import pose_graph_restated as W
    truth = W.circle_truth(n, radius=radius, turn=turn, z_amp=0.5)
    return truth, W.noisy_odometry(truth, np.random.default_rng(seed), 2e-3, 5e-3)


def scenes():
    """name -> dict(x0, loops [(i, j, rel, var)], gps [(node, xyz, var)], segment_nodes [...]): the 40-node arc of test_local_graph_and_marginal_covariance
    with GPS alone and with GPS and three nested loops, and the plan's edges"""
    import pose_graph_restated as W
    gps_var, loop_var = np.array([1.0, 1.0, 4.0]), np.full(6, 0.09)
    truth, x0 = arc(40, 15)
    rng = np.random.default_rng(16)
    fixes = {k: (k, truth[k, :3] + rng.normal(0, [1, 1, 2]), gps_var) for k in (4, 11, 18, 25, 32, 39)}
    lp = lambda t, i, j: (i, j, W.between(t[i], t[j]), loop_var)
    out = {"local_gps": dict(x0=x0, loops=[], gps=list(fixes.values()), segment_nodes=[1, 4, 7]),
           "gps_loops": dict(x0=x0, loops=[lp(truth, 39, 3), lp(truth, 30, 10), lp(truth, 22, 13)], gps=[fixes[4], fixes[18], fixes[32]], segment_nodes=[2, 5])}
    t24, x24 = arc(24, 13, radius=20.0, turn=0.98)
    g24 = [(k, t24[k, :3], gps_var) for k in (5, 17)]
    out["neighbour_loop"] = dict(x0=x24, loops=[lp(t24, 12, 11)], gps=g24, segment_nodes=[4])          # a segment with no interior
    out["one_interior"] = dict(x0=x24, loops=[lp(t24, 16, 14)], gps=g24, segment_nodes=[4])            # a segment with exactly one interior node
    out["two_nodes"] = dict(x0=x24[:2], loops=[], gps=[(1, t24[1, :3], gps_var)], segment_nodes=[4])      # (the fix keeps cond(H) at 1e8 as in the other scenes)
    out["one_node"] = dict(x0=x24[:1], loops=[], gps=[], segment_nodes=[4])
    t300, x300 = arc(300, 19, radius=150.0, turn=0.8)
    out["long_segment"] = dict(x0=x300, loops=[], gps=[(k, t300[k, :3], gps_var) for k in (20, 150, 280)], segment_nodes=[255])
    # 90 nested loops: 90 full rows live at once, so a column of the separator system has more than 512 rows below its diagonal
    t200, x200 = arc(200, 21, radius=100.0, turn=0.9)
    out["many_full_rows"] = dict(x0=x200, loops=[lp(t200, 199 - l, l) for l in range(90)], gps=[(k, t200[k, :3], gps_var) for k in (95, 104)], segment_nodes=[4])
    return out


def witness(sc):
    import pose_graph_restated as W
    g = W.Graph()
    g.add_prior(0, sc["x0"][0])
    g.add_chain(sc["x0"])
    for lp in sc["loops"]:
        g.add_between(*lp)
    for gp in sc["gps"]:
        g.add_gps(*gp)
    return g

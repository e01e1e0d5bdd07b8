"""The rules of include/glio_static.h restated in numpy, without the library: rule 2 (the cell of a point: float32, every product and sum rounded on its own,
the two bisections as the header spells them), rule 3 (the floor image), rules 4 - 6 (votes, decision, the kept points in order).  The tables and the relative
poses are arguments: the GPU tests hand in the library's own (glio_static_tables, glio_static_relative_pose) after tests/test_static_map_restated.py has held
those to tables() / relative_pose() here within one float ulp.

`wrong` names ONE deliberate mistake ("ge", "no_floor", "max", "edge_row_ignored", "no_wrap", "reorder"): tests/test_static_map_restated.py checks that the
cases of tests/static_map_cases.py refuse each of them."""
import math

import numpy as np

F32 = np.float32
WRONG = ("ge", "no_floor", "max", "edge_row_ignored", "no_wrap", "reorder")


class Params:
    """the options of glio_static_opts (its defaults) and the constants rule 2 and rule 4 derive from them"""

    def __init__(self, rows=44, cols_per_quadrant=90, neighbourhood=1, min_votes=2, elev_min_deg=-31.0, elev_max_deg=13.0, min_range=1.0, max_range=80.0,
                 range_gain=1.05, range_margin=0.3):
        self.rows, self.cpq, self.cols, self.nb, self.min_votes = int(rows), int(cols_per_quadrant), 4 * int(cols_per_quadrant), int(neighbourhood), int(min_votes)
        self.elev_min_deg, self.elev_max_deg = float(F32(elev_min_deg)), float(F32(elev_max_deg))
        self.min2 = F32(float(F32(min_range)) * float(F32(min_range)))
        self.max2 = F32(float(F32(max_range)) * float(F32(max_range)))
        self.g2 = F32(float(F32(range_gain)) * float(F32(range_gain)))
        self.m2 = F32(float(F32(range_margin)) * float(F32(range_margin)))


def tables(P):
    """s2 [rows + 1] = (float)(t |t|), t = tan of the k-th row edge; dir [cols][2] = ((float)cos, (float)sin)(2 pi s / cols); formed in double"""
    k = np.arange(P.rows + 1, dtype=np.float64)
    e = P.elev_min_deg + ((P.elev_max_deg - P.elev_min_deg) * k) / float(P.rows)
    t = np.tan((e * 3.141592653589793) / 180.0)
    a = (6.283185307179586 * np.arange(P.cols, dtype=np.float64)) / float(P.cols)
    return (t * np.abs(t)).astype(F32), np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)


def rotation(q):
    q = [float(v) for v in q]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    w, x, y, z = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]], np.float64)


def relative_pose(pose_v, pose_f, dtype=F32):
    """rule 1 in numpy's double: T(v, f) = pose_v^-1 o pose_f as [3][4]"""
    pv, pf = np.asarray(pose_v, np.float64), np.asarray(pose_f, np.float64)
    Rv, Rf = rotation(pv[3:]), rotation(pf[3:])
    return np.c_[Rv.T @ Rf, Rv.T @ (pf[:3] - pv[:3])].astype(dtype)


def cells(xyz, s2, dirs, P):
    """rule 2 for points [n][3] float32: (cell [n] int, -1 = skipped; r2 [n] float32)"""
    p = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        rho2 = (x * x) + (y * y)
        r2 = rho2 + (z * z)
        ok = finite & ~(rho2 == F32(0)) & (r2 >= P.min2) & (r2 < P.max2)
        a = z * np.abs(z)
        ok &= ((s2[0] * rho2) <= a) & (a < (s2[P.rows] * rho2))
        lo, hi = np.zeros(len(p), np.int64), np.full(len(p), P.rows, np.int64)
        while np.any(hi - lo > 1):
            live = hi - lo > 1
            mid = (lo + hi) >> 1
            up = (s2[mid] * rho2) <= a
            lo = np.where(live & up, mid, lo)
            hi = np.where(live & ~up, mid, hi)
        row = lo
        quad = np.where((x > 0) & (y >= 0), 0, np.where((x <= 0) & (y > 0), 1, np.where((x < 0) & (y <= 0), 2, 3)))
        lo, hi = np.zeros(len(p), np.int64), np.full(len(p), P.cpq, np.int64)
        while np.any(hi - lo > 1):
            live = hi - lo > 1
            mid = (lo + hi) >> 1
            d = dirs[quad * P.cpq + mid]
            up = ((d[:, 0] * y) - (d[:, 1] * x)) >= F32(0)
            lo = np.where(live & up, mid, lo)
            hi = np.where(live & ~up, mid, hi)
    assert r2.dtype == F32 and a.dtype == F32
    return np.where(ok, row * P.cols + quad * P.cpq + lo, -1), r2


def raw_image(cloud, s2, dirs, P, wrong=None):
    """[rows][cols] float32: the minimum r2 per cell, an empty cell +0"""
    c, r2 = cells(np.ascontiguousarray(cloud, F32)[:, :3], s2, dirs, P)
    k = c >= 0
    if wrong == "max":
        img = np.zeros(P.rows * P.cols, F32)
        np.maximum.at(img, c[k], r2[k])
    else:
        img = np.full(P.rows * P.cols, np.inf, F32)
        np.minimum.at(img, c[k], r2[k])
        img[np.isinf(img)] = F32(0)
    return img.reshape(P.rows, P.cols)


def floor_image(raw, P, wrong=None):
    """rule 3"""
    if P.nb == 0 or wrong == "no_floor":
        return raw.copy()
    out = np.zeros_like(raw)
    for r in range(P.rows):
        for c in range(P.cols):
            m, blocked = F32(np.inf), False
            for dr in (-1, 0, 1):
                rr = r + dr
                if rr < 0 or rr >= P.rows:
                    if wrong == "edge_row_ignored":
                        continue
                    blocked = True
                    break
                for dc in (-1, 0, 1):
                    cc = c + dc
                    if wrong == "no_wrap":
                        if cc < 0 or cc >= P.cols:
                            continue
                    else:
                        cc %= P.cols
                    v = raw[rr, cc]
                    if v == 0:
                        blocked = True
                        break
                    m = min(m, v)
                if blocked:
                    break
            out[r, c] = F32(0) if blocked else m
    return out


def floor_image_fast(raw, P, wrong=None):
    """rule 3, vectorised (the same bytes as floor_image: tests/test_static_map_restated.py compares them)"""
    if P.nb == 0 or wrong == "no_floor":
        return raw.copy()
    big = np.where(raw == 0, F32(-1), raw)                      # an empty cell poisons the minimum
    pad = np.full((P.rows + 2, P.cols), F32(-1) if wrong != "edge_row_ignored" else F32(np.inf), F32)
    pad[1:-1] = big
    stack = []
    for dr in (0, 1, 2):
        for dc in (-1, 0, 1):
            sh = np.roll(pad[dr:dr + P.rows], -dc, axis=1)
            if wrong == "no_wrap" and dc != 0:
                sh = sh.copy()
                sh[:, -1 if dc == 1 else 0] = F32(np.inf)
            stack.append(sh)
    m = np.min(np.stack(stack), axis=0)
    return np.where(m < 0, F32(0), m).astype(F32)


def transform(xyz, T):
    """rule 4's x' = ((T00 x + T01 y) + T02 z) + T03, float32"""
    p = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    T = np.asarray(T, F32).reshape(3, 4)
    with np.errstate(all="ignore"):
        out = [(((T[i, 0] * p[:, 0]) + (T[i, 1] * p[:, 1])) + (T[i, 2] * p[:, 2])) + T[i, 3] for i in range(3)]
    assert out[0].dtype == F32
    return np.stack(out, axis=1)


def votes(cloud, Ts, floors, s2, dirs, P, wrong=None):
    """(through [n] uint8, tested [n] uint8) of a frame's points against its views: Ts[j] = T(v_j, f), floors[j] = the floor image of v_j"""
    n = len(cloud)
    th, te = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for T, Fl in zip(Ts, floors):
        c, r2 = cells(transform(np.ascontiguousarray(cloud, F32)[:, :3], T), s2, dirs, P)
        Fv = Fl.reshape(-1)[np.maximum(c, 0)]
        t = (c >= 0) & (Fv > 0)
        with np.errstate(all="ignore"):
            bound = (P.g2 * r2) + P.m2
        s = t & ((Fv >= bound) if wrong == "ge" else (Fv > bound))
        te += t
        th += s
    return th.astype(np.uint8), te.astype(np.uint8)


def classify(clouds, rel, view_offsets, views, s2, dirs, P, wrong=None):
    """rules 2 - 6 for a call: clouds[f] [n_f][4] float32, rel[j] = T(views[j], f) for j in view_offsets[f] .. view_offsets[f + 1].
    -> list per frame of dict(through, tested, dynamic [n_f] bool, kept [m][4] float32), and the (raw, floor) images per frame"""
    images = []
    for c in clouds:
        raw = raw_image(c, s2, dirs, P, wrong)
        images.append((raw, floor_image_fast(raw, P, wrong)))
    out = []
    for f, c in enumerate(clouds):
        js = range(int(view_offsets[f]), int(view_offsets[f + 1]))
        th, te = votes(c, [rel[j] for j in js], [images[int(views[j])][1] for j in js], s2, dirs, P, wrong)
        dyn = th >= P.min_votes
        kept = np.ascontiguousarray(c, F32)[~dyn]
        if wrong == "reorder":
            kept = kept[::-1]
        out.append(dict(through=th, tested=te, dynamic=dyn, kept=np.ascontiguousarray(kept)))
    return out, images


def relative_poses(poses, view_offsets, views, fn=relative_pose):
    """rel[j] for classify from poses [n][7] with fn(pose_v, pose_f)"""
    rel = []
    for f in range(len(view_offsets) - 1):
        for j in range(int(view_offsets[f]), int(view_offsets[f + 1])):
            rel.append(fn(poses[int(views[j])], poses[f]))
    return rel


def static_views(poses, half_window, min_baseline=0.5):
    """the host helper's rule, written independently: nearest earlier frames first, then nearest later ones, each at least min_baseline away"""
    p = np.asarray(poses, np.float64).reshape(-1, 7)[:, :3]
    off, views = [0], []
    for f in range(len(p)):
        far = [j for j in range(len(p)) if np.sum((p[j] - p[f]) ** 2) >= min_baseline ** 2]
        views += [j for j in reversed(far) if j < f][:half_window] + [j for j in far if j > f][:half_window]
        off.append(len(views))
    return np.array(off, np.int32), np.array(views, np.int32)

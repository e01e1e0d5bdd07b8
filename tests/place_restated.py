"""The rules of include/glio_place.h restated in numpy, without the library: the binning of a cloud into the 20 x 60 Scan Context cells in float32,
operation by operation (every product and sum rounded on its own, so the bytes are the device's), the unit columns, the distance over all 60 shifts in float32
in the stated order, and an fp64 twin of the distance.  The two tables (rb2, dir) are arguments: the tests hand in the library's (glio_place_tables) after
checking them against tables() here to 1 ulp.  naive_scan_context is an independent, textbook Scan Context (atan2 / sqrt in fp64) to hold the binning against."""
import math

import numpy as np

RINGS, SECTORS = 20, 60
MASK60 = (1 << 60) - 1
F32 = np.float32


def tables(max_radius):
    """rb2 [21] = (float)((k max_radius / 20)^2), dir [60][2] = ((float)cos, (float)sin)(2 pi s / 60), formed in double"""
    k = np.arange(RINGS + 1, dtype=np.float64)
    r = k * float(F32(max_radius)) / 20.0
    rb2 = (r * r).astype(F32)
    a = (6.283185307179586 * np.arange(SECTORS, dtype=np.float64)) / 60.0
    return rb2, np.stack([np.cos(a), np.sin(a)], axis=1).astype(F32)


def level_matrix(q):
    """the rotation matrix of q / |q| (w first) in double, stored as float32; None: the identity"""
    w, x, y, z = 1.0, 0.0, 0.0, 0.0
    if q is not None:
        q = [float(v) for v in q]
        n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        w, x, y, z = q[0] / n, q[1] / n, q[2] / n, q[3] / n
    m = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
    return np.array(m, np.float64).astype(F32).reshape(3, 3)


def cells(points, rb2, dirs, level_q=None):
    """(kept [n] bool, ring [n], sector [n], levelled xyz [n][3] float32) of points [n][>=3] float32"""
    p = np.ascontiguousarray(points, F32).reshape(len(points), -1)[:, :3]
    R = level_matrix(level_q)
    finite = np.all(np.isfinite(p), axis=1)
    with np.errstate(all="ignore"):
        x = ((R[0, 0] * p[:, 0]) + (R[0, 1] * p[:, 1])) + (R[0, 2] * p[:, 2])
        y = ((R[1, 0] * p[:, 0]) + (R[1, 1] * p[:, 1])) + (R[1, 2] * p[:, 2])
        z = ((R[2, 0] * p[:, 0]) + (R[2, 1] * p[:, 1])) + (R[2, 2] * p[:, 2])
        r2 = (x * x) + (y * y)
        kept = finite & (r2 > F32(0)) & (r2 < rb2[RINGS])
        ring = np.sum(rb2[None, 1:RINGS] <= r2[:, None], axis=1)
        quad = np.where((x > 0) & (y >= 0), 0, np.where((x <= 0) & (y > 0), 1, np.where((x < 0) & (y <= 0), 2, 3)))
        count = np.zeros(len(p), np.int64)
        for k in range(1, 15):
            d = dirs[15 * quad + k]
            count += ((d[:, 0] * y) - (d[:, 1] * x)) >= F32(0)
    assert x.dtype == F32 and r2.dtype == F32
    return kept, ring, 15 * quad + count, np.stack([x, y, z], axis=1)


def descriptor(points, rb2, dirs, lidar_height, level_q=None):
    """(heights [20][60] float32, mask): the maximum of z' + lidar_height per cell, an empty cell +0, bit s of mask set when sector s holds a point"""
    kept, ring, sector, xyz = cells(points, rb2, dirs, level_q)
    with np.errstate(all="ignore"):
        v = xyz[:, 2] + F32(lidar_height)
    kept = kept & np.isfinite(v)
    v = np.where(v == 0, F32(0), v).astype(F32)
    h = np.full((RINGS, SECTORS), -np.inf, F32)
    np.maximum.at(h, (ring[kept], sector[kept]), v[kept])
    h[np.isinf(h)] = F32(0)
    mask = 0
    for s in np.unique(sector[kept]):
        mask |= 1 << int(s)
    return h, mask


def unit_columns(heights, mask):
    """(u [20][60] float32, present mask): fp64 sum of squares over ascending ring, fp64 square root rounded to float, float division; absent columns zero"""
    h = np.asarray(heights, F32).reshape(RINGS, SECTORS)
    s = np.zeros(SECTORS, np.float64)
    for k in range(RINGS):
        s = s + h[k].astype(np.float64) * h[k].astype(np.float64)
    nrm = np.sqrt(s).astype(F32)
    has = np.array([(int(mask) >> j) & 1 for j in range(SECTORS)], bool)
    present = has & (nrm > 0) & np.isfinite(nrm)
    u = np.zeros((RINGS, SECTORS), F32)
    u[:, present] = h[:, present] / nrm[present][None, :]
    pm = 0
    for j in np.flatnonzero(present):
        pm |= 1 << int(j)
    return u, pm


def rotated_mask(cm, s):
    """bit j = the candidate's column (j + s) mod 60"""
    return cm if s == 0 else ((cm >> s) | (cm << (SECTORS - s))) & MASK60


def shift_distances(uq, pq, uc, pc, dtype=F32):
    """distance [60] of query (uq, pq) to candidate (uc, pc) at every shift: 1 - (sum_j Q_j . C_(j+s)) / cnt(s), the dot product over ascending ring, the sum
    over ascending j, both in `dtype`; cnt(s) = 0 gives exactly 1"""
    a, b = uq.astype(dtype), uc.astype(dtype)
    G = np.zeros((SECTORS, SECTORS), dtype)
    for k in range(RINGS):
        G = G + a[k][:, None] * b[k][None, :]
    sums = np.zeros(SECTORS, dtype)
    sh = np.arange(SECTORS)
    for j in range(SECTORS):
        sums = sums + G[j, (j + sh) % SECTORS]
    cnt = np.array([bin(pq & rotated_mask(pc, s)).count("1") for s in range(SECTORS)])
    with np.errstate(all="ignore"):
        d = dtype(1) - sums / cnt.astype(dtype)
    return np.where(cnt > 0, d, dtype(1)).astype(dtype)


def pair(uq, pq, uc, pc, dtype=F32):
    """(distance, shift): the smallest over all 60 shifts, the lowest shift on a tie"""
    d = shift_distances(uq, pq, uc, pc, dtype)
    s = int(np.argmin(d))
    return d[s], s


def yaw_of_shift(s):
    return F32(float(s) * (6.283185307179586 / 60.0))


class Store:
    """places as the device keeps them: index -> (u, present mask, time), None where invalid"""

    def __init__(self, n):
        self.places = [None] * n

    def set(self, place, heights, mask, time):
        u, pm = unit_columns(heights, mask)
        self.places[place] = (u, pm, float(time))

    def candidates(self, q, min_time_gap, earlier_only=False):
        tq = self.places[q][2]
        return [c for c, p in enumerate(self.places) if p is not None and c != q and abs(p[2] - tq) > min_time_gap and (not earlier_only or p[2] < tq)]

    def all_pairs(self, q, min_time_gap, earlier_only=False, dtype=F32):
        """[(distance, place, shift)] of every candidate, sorted by (distance, place)"""
        uq, pq, _ = self.places[q]
        out = []
        for c in self.candidates(q, min_time_gap, earlier_only):
            d, s = pair(uq, pq, self.places[c][0], self.places[c][1], dtype)
            out.append((d, c, s))
        out.sort(key=lambda r: (r[0], r[1]))
        return out

    def query(self, q, min_time_gap, top_k, earlier_only=False, dtype=F32):
        return self.all_pairs(q, min_time_gap, earlier_only, dtype)[:top_k]


def naive_scan_context(points, max_radius, lidar_height):
    """a textbook Scan Context in fp64: ring = floor(r / (max_radius / 20)), sector = floor(theta / 6 deg), cell = max(z + lidar_height), empty = 0"""
    p = np.asarray(points, np.float64)[:, :3]
    r = np.hypot(p[:, 0], p[:, 1])
    th = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2.0 * np.pi)
    ring = np.floor(r / (float(max_radius) / RINGS)).astype(int)
    sector = np.minimum(np.floor(th / (2.0 * np.pi / SECTORS)).astype(int), SECTORS - 1)
    keep = (r > 0) & (ring < RINGS)
    h = np.full((RINGS, SECTORS), -np.inf)
    np.maximum.at(h, (ring[keep], sector[keep]), p[keep, 2] + float(lidar_height))
    h[np.isinf(h)] = 0.0
    return h, ring, sector, keep

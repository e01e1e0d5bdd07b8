"""The cell key, the open-addressing probe and the tile grouping of the association (csrc/assoc_kernels.hip on the key helpers of csrc/cloud_device.h),
bit for bit against the oracle (oracle/pyoracle.py) on the shapes where that code can go wrong.  A numpy restatement of the documented layout -- key =
(ix + 2^20) << 42 | (iy + 2^20) << 21 | (iz + 2^20) of the cell floor(v * inv_cell) in float, the 64-bit MurmurHash3 finaliser, home slot = (hash of the
2 x 2 x 2 block's key << 3 | the cell's three parities) & (cap - 1), linear probing -- picks the inputs and asserts each case's precondition; a case whose
precondition fails is a failure.  The table is read through glio_debug_read_map_table.  The cases:
  wrap      table of 1024 slots; several occupied cells have their home in slot 1023, so an insertion and the look-ups of the cell that lost the slot step
            from slot cap - 1 to slot 0; every occupied cell holds a planar patch of 9 points
  signs     cells -2 .. 1 on every axis (-1 and 0 side by side, both parities) and blocks at x = +-1e5 m
  tiles     two tiles of the tiled insert (512 points each): 512 distinct cells in shuffled order, then 512 points in one cell; 2800 queries, 2300 of them in
            slot 0: two full tiles and a partial third of the query grouping's 1024 per launch row (k_qbin_tile at tile0 > 0, in the per-row modes and in the
            merged window), five tiles of the presort's 512; slot 1 holds the other 500
Every case: K1's entries (key, first, count), octant prefixes and sorted map against the restatement; the records of a lone scan under GLIO_KNN_MODE
0 .. 3 and of the one-call window association (the merged grouping) against the oracle.  The batch path: three keyframes of 600 points, pairs in both
directions, tables in the frames' own frames and at the run's poses, shared query binning on and off (a child process: the switch is read once per
process) -- all equal to the oracle's pair records."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

CELL = np.float32(1.25)                      # max(1.25, sqrt(kd_max_radius = 1.5) * 1.0001)
INV_CELL = np.float32(1.0) / CELL
M64 = (1 << 64) - 1


# ---- the restatement
def cells_of(pts):
    return np.floor(pts[:, :3].astype(np.float32) * INV_CELL).astype(np.int64)


def pack_key(c):
    c = np.asarray(c, np.int64)
    return (((c[..., 0] + (1 << 20)).astype(np.uint64) << np.uint64(42)) | ((c[..., 1] + (1 << 20)).astype(np.uint64) << np.uint64(21)) |
            (c[..., 2] + (1 << 20)).astype(np.uint64))


def unpack_key(k):
    k = np.asarray(k, np.uint64)
    return np.stack([((k >> np.uint64(s)) & np.uint64(0x1fffff)).astype(np.int64) - (1 << 20) for s in (42, 21, 0)], -1)


def hash_key(k):
    k = int(k)
    k ^= k >> 33; k = (k * 0xff51afd7ed558ccd) & M64; k ^= k >> 33; k = (k * 0xc4ceb9fe1a85ec53) & M64; k ^= k >> 33
    return k & 0xffffffff


def home_slot(c, cap):
    h = hash_key(pack_key(np.asarray(c) >> 1))
    return (((h << 3) & 0xffffffff) | int((c[0] & 1) | ((c[1] & 1) << 1) | ((c[2] & 1) << 2))) & (cap - 1)


def octant_of(pts):
    h = np.floor(pts[:, :3].astype(np.float32) * (INV_CELL * np.float32(2.0))).astype(np.int64)
    return (h[:, 0] & 1) | ((h[:, 1] & 1) << 1) | ((h[:, 2] & 1) << 2)


def patch(centre, rng, n=3):
    """n x n points 0.2 m apart in the plane z = centre z + 0.3, shuffled"""
    g = (np.arange(n) - (n - 1) / 2) * 0.2
    p = np.stack(np.meshgrid(g, g, [0.3], indexing="ij"), -1).reshape(-1, 3) + centre
    return p[rng.permutation(len(p))]


def f4(xyz, rng=None):
    a = np.zeros((len(xyz), 4), np.float32)
    a[:, :3] = xyz
    if rng is not None:
        a[:, 3] = rng.uniform(0, 50, len(xyz))
    return a


def centre_of(c):
    return (np.asarray(c, float) + 0.5) * 1.25


# ---- the cases: (map, queries, max_map_points, table slots, queries of slot 0)
def case_wrap():
    rng = np.random.default_rng(20261021)
    cap = 1024
    # cells of odd parity on every axis whose 2 x 2 x 2 block hashes to the table's last line: their home is slot cap - 1
    last = [c for c in ((2 * bx + 1, 2 * by + 1, 2 * bz + 1) for bx in range(4, 40) for by in range(-20, 20) for bz in range(0, 3)) if home_slot(np.array(c), cap) == cap - 1]
    assert len(last) >= 3, "the search box holds cells whose home is the last slot"
    cells = last[:3]
    # ... and cells around them, whatever their home
    for c in last[:3]:
        cells += [(c[0] + 1, c[1], c[2]), (c[0], c[1] - 1, c[2])]
    cells += [(bx, by, 0) for bx in range(6, 12) for by in range(-3, 4)]
    cells = list(dict.fromkeys(cells))[:56]                                    # 9 points each: at most 504 of the 512 the table is sized for
    mp = np.concatenate([patch(centre_of(c), rng) for c in cells])
    mp = mp[rng.permutation(len(mp))]
    # queries: 4 in the patch of every occupied cell (a little off the plane), 100 elsewhere
    qs = np.concatenate([centre_of(c) + np.c_[rng.uniform(-0.25, 0.25, (4, 2)), 0.3 + rng.uniform(-0.04, 0.04, (4, 1))] for c in cells] +
                        [rng.uniform([5, -5, 0], [20, 5, 2], (100, 3))])
    homes = [home_slot(np.array(c), cap) for c in cells]
    assert homes.count(cap - 1) >= 2, "two occupied cells share the last slot: one of them is stored behind the table's end"
    in_patches = np.isin(pack_key(cells_of(f4(qs))), pack_key(np.array(cells))).mean()
    assert in_patches > 0.5, in_patches
    return f4(mp, rng), f4(qs, rng), 512, cap, len(qs) // 2


def case_signs():
    rng = np.random.default_rng(20261022)
    cells = [(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)]
    for sx in (-1, 1):
        cells += [(sx * 80000 + dx, 2 + dy, dz) for dx in (-1, 0) for dy in (0, 1) for dz in (0, 1)]
    mp = np.concatenate([patch(centre_of(c), rng) for c in cells])
    mp = mp[rng.permutation(len(mp))]
    qs = np.concatenate([centre_of(c) + np.c_[rng.uniform(-0.3, 0.3, (6, 2)), 0.3 + rng.uniform(-0.05, 0.05, (6, 1))] for c in cells] +
                        [rng.uniform([-3, -3, -3], [3, 3, 3], (200, 3))])
    got = cells_of(f4(mp))
    assert set(map(tuple, got)) == set(cells) and abs(mp[:, 0]).max() > 9.9e4
    for a in range(3):
        assert {-1, 0} <= set(got[:, a]) and {0, 1} == set(got[:, a] & 1)
    return f4(mp, rng), f4(qs, rng), 1024, 2048, len(qs) // 2


def case_tiles():
    rng = np.random.default_rng(20261023)
    # tile 0: 512 distinct cells, eight around each of 64 shared corners (the points 0.2 m off the corner in x and y, 0.02 m in z: nearly planar)
    corners = np.array([(2 * i, 2 * j, 0) for i in range(8) for j in range(8)])                       # in cells: the corner of cells (c - 1 .. c)^3
    off = np.array([(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) * [0.2, 0.2, 0.02]
    t0 = (corners[:, None, :] * 1.25 + off[None, :, :]).reshape(-1, 3)
    t0 = t0[rng.permutation(len(t0))]
    # tile 1: 512 points of one cell, in a plane
    one = (20, 20, 1)
    t1 = centre_of(one) + np.c_[rng.uniform(-0.6, 0.6, (512, 2)), np.full(512, 0.1)]
    mp = np.concatenate([t0, t1])
    assert len(t0) == 512 and len(np.unique(pack_key(cells_of(f4(t0))))) == 512 and len(np.unique(pack_key(cells_of(f4(t1))))) == 1
    qs = np.concatenate([t0[rng.integers(0, 512, 1100)] + rng.normal(0, 0.03, (1100, 3)), centre_of(one) + np.c_[rng.uniform(-0.6, 0.6, (1700, 2)), 0.1 + rng.uniform(-0.05, 0.05, (1700, 1))]])
    qs = qs[rng.permutation(len(qs))]
    split = 2300
    assert split > 2 * 1024 and split % 1024 and len(qs) - split > 0, "slot 0 fills two tiles of the query grouping and part of a third"
    return f4(mp, rng), f4(qs, rng), 1024, 2048, split


CASES = {"wrap": case_wrap, "signs": case_signs, "tiles": case_tiles}
_made = {}


def made(name):
    """the case's inputs and the oracle's records of its queries split into two slots, computed once"""
    if name not in _made:
        from glio_amd import synth
        from oracle import pyoracle as po
        mp, qs, max_map, cap, split = CASES[name]()
        slots = [np.ascontiguousarray(qs[:split]), np.ascontiguousarray(qs[split:])]
        o = synth.default_opts(2, pts=max(len(s) for s in slots), map_pts=max_map)
        rng = np.random.default_rng(5)
        if name != "tiles":                                                # (wrap: the queries stay in the cells they were picked for; signs: a rotation would move the far blocks by metres)
            quats = np.tile([1.0, 0, 0, 0], (2, 1)); trans = np.zeros((2, 3))
        else:
            quats = np.array([np.r_[1.0, 0.5 * rng.normal(0, 0.004, 3)] for _ in range(2)]); quats /= np.linalg.norm(quats, axis=1, keepdims=True)
            trans = rng.normal(0, 0.02, (2, 3))
        want = [po.associate(o, mp, slots[s], quats[s], trans[s])[:3] for s in range(2)]
        assert sum(len(w[2]) for w in want) > 0, "the oracle keeps records"
        _made[name] = (mp, slots, o, cap, quats, trans, want)
    return _made[name]


def read_table(ctx, n):
    from glio_amd import capi
    import ctypes as C
    lib = capi.load()
    cap = C.c_int32()
    assert lib.glio_debug_read_map_table(ctx._h, C.byref(cap), None, None, None) == 0
    ent = np.zeros((cap.value, 4), np.int32); sub = np.zeros((cap.value, 4), np.uint32); srt = np.zeros((n, 4), np.float32)
    assert lib.glio_debug_read_map_table(ctx._h, None, ent.ctypes.data_as(C.c_void_p), sub.ctypes.data_as(C.c_void_p), srt.ctypes.data_as(C.c_void_p)) == 0
    return ent, sub, srt


def same(got, want):
    return all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))


@pytest.mark.parametrize("name", list(CASES))
def test_k1_table_against_the_restatement(name):
    from glio_amd import capi
    mp, slots, o, cap, quats, trans, want = made(name)
    ctx = capi.Context(o); ctx.set_map(mp)
    ent, sub, srt = read_table(ctx, len(mp))
    ctx.close()
    assert len(ent) == cap
    keys = pack_key(cells_of(mp))
    uniq, counts = np.unique(keys, return_counts=True)
    full = (ent[:, 0].astype(np.uint32).astype(np.uint64)) | (ent[:, 1].astype(np.uint32).astype(np.uint64) << np.uint64(32))
    occ = np.flatnonzero(full != np.uint64(M64))
    # the occupied slots hold exactly the map's cells with their counts; the empty ones (-1, -1, x, 0)
    order = np.argsort(full[occ])
    assert np.array_equal(full[occ][order], uniq) and np.array_equal(ent[occ][order][:, 3], counts)
    assert np.all(ent[full == np.uint64(M64), 3] == 0)
    # every key lies on its probe chain: from its home slot to its slot no slot is empty (the walk may pass the table's end)
    behind = []                                                             # the slots whose key was stored behind the table's end
    for s in occ:
        h = home_slot(unpack_key(full[s]), cap)
        steps = (int(s) - h) % cap
        chain = (h + np.arange(steps)) % cap
        assert np.all(full[chain] != np.uint64(M64)), (name, int(s), h)
        if h + steps >= cap:
            behind.append(int(s))
    if name == "wrap":
        assert behind, "an insertion stepped from slot cap - 1 to slot 0"
        assert np.isin(full[behind], pack_key(np.concatenate([cells_of(s) for s in slots]))).any(), "a query's look-up does the same"
    # the cells' runs partition the sorted map; a run holds its cell's points (w = original index), ordered by octant as the prefixes say
    starts = np.sort(ent[occ, 2])
    assert np.array_equal(starts, np.r_[0, np.cumsum(ent[occ][np.argsort(ent[occ, 2])][:, 3])[:-1]])
    orig = srt[:, 3].view(np.int32)
    assert np.array_equal(np.sort(orig), np.arange(len(mp))) and np.array_equal(srt[:, :3], mp[orig, :3])
    oc = octant_of(mp)
    for s in occ:
        first, cnt = int(ent[s, 2]), int(ent[s, 3])
        run = orig[first:first + cnt]
        assert np.all(keys[run] == full[s]), (name, int(s))
        assert np.all(np.diff(oc[run]) >= 0), (name, int(s))
        pre = np.r_[[(int(w) >> sh) & 0xffff for w in sub[s] for sh in (0, 16)]]
        assert np.array_equal(pre, np.r_[0, np.cumsum(np.bincount(oc[run], minlength=8))[:-1]]), (name, int(s))


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_records_in_every_search_mode(name, mode):
    from glio_amd import capi
    mp, slots, o, cap, quats, trans, want = made(name)
    lib = capi.load()
    lib.glio_debug_set_knn_mode(mode)
    try:
        ctx = capi.Context(o); ctx.set_map(mp)
        for s in range(2):                                                 # a lone scan
            n = ctx.associate(s, slots[s], quats[s], trans[s])
            assert n == len(want[s][2]), (name, mode, s, n, len(want[s][2]))
            assert same(ctx.get_correspondences(s), want[s]), (name, mode, s)
        for rep in range(2):                                               # the one-call window association; twice: the grouping tables are left clean
            cnt = ctx.associate_window(quats, trans)
            for s in range(2):
                assert cnt[s] == len(want[s][2]) and same(ctx.get_correspondences(s), want[s]), (name, mode, rep, s)
        ctx.close()
    finally:
        lib.glio_debug_set_knn_mode(0)


# ---- the batch path
PAIRS = (np.array([0, 1, 1, 2, 0, 2], np.int32), np.array([1, 0, 2, 1, 2, 0], np.int32))


def batch_frames():
    from glio_amd import synth
    win = synth.make_window(W=3, pts_per_scan=600, seed=synth.SEED_BASE + 7101, perturb=(0.03, 0.2, 0.0), scan_radius=9.0, map_density=1.0)
    tlb = np.array(win.opts.t_lb, np.float32)
    scans = []
    for s in range(3):
        sc = win.scans[s].copy(); sc[:, :3] -= tlb
        scans.append(np.ascontiguousarray(sc))
    return scans, np.c_[win.init.trans, win.init.quat]


def batch_records(local):
    from glio_amd import batch, capi
    scans, poses = batch_frames()
    lib = capi.load()
    lib.glio_debug_set_bassoc_local(local)
    try:
        ba = batch.BatchAssociation(3, 1024, 6 * 1024)
        for k in range(3):
            ba.set_frame(k, scans[k])
        out = []
        for rep in range(2):                                               # twice: the second run finds the local tables built
            counts, total = ba.run(poses, *PAIRS)
            out.append((counts.tolist(), [a.copy() for a in ba.read()]))
        ba.close()
    finally:
        lib.glio_debug_set_bassoc_local(1)
    assert out[0][0] == out[1][0] and same(out[0][1], out[1][1])
    return out[0]


def check_batch(got):
    from oracle import pyoracle as po
    scans, poses = batch_frames()
    counts, (cp, nc, sc) = got
    first = 0
    for p in range(len(PAIRS[0])):
        i, j = PAIRS[0][p], PAIRS[1][p]
        ocp, onc, osc, _ = po.associate_pair(scans[i], poses[i], scans[j], poses[j])
        n = counts[p]
        assert n == len(osc), (p, n, len(osc))
        assert same((cp[first:first + n], nc[first:first + n], sc[first:first + n]), (ocp, onc, osc)), p
        first += n
    assert first > 100, "the scene produces pair records"


@pytest.mark.parametrize("local", [1, 0])
def test_batch_pairs_in_both_table_modes(local):
    check_batch(batch_records(local))


def test_batch_pairs_without_shared_bins():
    """GLIO_BASSOC_SHARED_BINS is read once per process: a child, tables at the run's poses (the only mode that shares its bins)"""
    env = dict(os.environ, GLIO_BASSOC_SHARED_BINS="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "bassoc-child"], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("{")))
    assert got["shared_bins"] == 0
    counts, recs = batch_records(0)
    assert got["counts"] == counts and got["hex"] == [a.tobytes().hex() for a in recs]


if __name__ == "__main__" and sys.argv[1:] == ["bassoc-child"]:
    from glio_amd import capi
    counts, recs = batch_records(0)
    sw = {r["name"]: r["value"] for r in capi.switches()}
    print(json.dumps({"shared_bins": sw["GLIO_BASSOC_SHARED_BINS"], "counts": counts, "hex": [a.tobytes().hex() for a in recs]}))

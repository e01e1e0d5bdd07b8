"""Bits of the association (csrc/assoc_kernels.hip) and of the local map's voxel table, for A/B runs of two builds of the library (GLIO_HIP_LIB selects one;
a fresh process per build): one sha256 per case over the output arrays.  Two builds that compute the same print the same lines.
  K1            the table of the window's map: entries (key, count), octant prefixes and the sorted map, read through glio_debug_read_map_table.  Which of two
                colliding cells gets the earlier slot, where a cell's run starts and the order of the points inside an octant follow the order the atomics
                arrive in, so the hash is taken over a canonical form: the entries by key, every octant's points by original index
  lone scan     records and counts of a 6000-point scan under GLIO_KNN_MODE 0, 1, 2 and 3
  window        the one-call window association of 4 slots (mode 0: the merged grouping) and glio_select_correspondences_window on it
  batch         glio_bassoc_run of a pair list (5 keyframes, range 2, both directions) with the tables in the frames' own frames and at the run's poses
                (glio_debug_set_bassoc_local 1 / 0); the same with GLIO_BASSOC_SHARED_BINS=0 is another process (the switch is read once): its lines carry the value
  draws         glio_bassoc_run_append_async + glio_bassoc_select_tail_draws_async (the on-stream selection), 25 records per pair
  local map     glio_localmap push / build of 5 keyframes (the voxel key it shares with K1), then K1 from the map on the device and a window association on it
    GLIO_HIP_LIB=<library> [GLIO_BASSOC_SHARED_BINS=0] python scripts/assoc_bits_ab.py > bits.txt"""
import ctypes as C
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from glio_amd import batch, capi, synth


def sha(*parts):
    m = hashlib.sha256()
    for p in parts:
        m.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return m.hexdigest()[:16]


lib = capi.load()
bins = {r["name"]: r["value"] for r in capi.switches()}["GLIO_BASSOC_SHARED_BINS"]
win = synth.make_window(W=4, pts_per_scan=6000, seed=synth.SEED_BASE + 7201, scan_radius=20.0)
poses = [capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s]) for s in range(win.W)]
quats, trans = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])

# ---- K1
ctx = capi.Context(win.opts)
ctx.set_map(win.map_pts)
cap = C.c_int32()
assert lib.glio_debug_read_map_table(ctx._h, C.byref(cap), None, None, None) == 0
ent = np.zeros((cap.value, 4), np.int32); sub = np.zeros((cap.value, 4), np.uint32); srt = np.zeros((len(win.map_pts), 4), np.float32)
assert lib.glio_debug_read_map_table(ctx._h, None, ent.ctypes.data_as(C.c_void_p), sub.ctypes.data_as(C.c_void_p), srt.ctypes.data_as(C.c_void_p)) == 0
occ = np.flatnonzero((ent[:, 0] & ent[:, 1]) != -1)
key = ent[occ, 0].astype(np.uint32).astype(np.uint64) | (ent[occ, 1].astype(np.uint32).astype(np.uint64) << np.uint64(32))
order = occ[np.argsort(key)]
runs = []
for s in order:
    first, cnt = int(ent[s, 2]), int(ent[s, 3])
    pre = [(int(w) >> sh) & 0xffff for w in sub[s] for sh in (0, 16)] + [cnt]
    run = srt[first:first + cnt]
    runs += [run[pre[o]:pre[o + 1]][np.argsort(run[pre[o]:pre[o + 1], 3].view(np.int32), kind="stable")] for o in range(8)]
print("K1 map %d points table %d slots %d cells: ent %s sub %s sorted %s" % (len(win.map_pts), cap.value, len(occ), sha(np.sort(key), ent[order, 3]), sha(sub[order]), sha(*runs)))

# ---- a lone scan under every search mode
for mode in (0, 1, 2, 3):
    lib.glio_debug_set_knn_mode(mode)
    n = ctx.associate(0, win.scans[0], quats[0], trans[0])
    print("lone scan %d points GLIO_KNN_MODE %d kept %d: %s" % (len(win.scans[0]), mode, n, sha(*ctx.get_correspondences(0))))
lib.glio_debug_set_knn_mode(0)

# ---- the one-call window association, the window selection
for s in range(win.W):
    ctx.set_scan(s, win.scans[s])
cnt = ctx.associate_window(quats, trans)
print("window %d slots kept %s: %s" % (win.W, cnt.tolist(), sha(*[a for s in range(win.W) for a in ctx.get_correspondences(s)])))
rng = np.random.default_rng(7)
sel = [None if s == 1 else rng.permutation(int(cnt[s]))[:min(400, int(cnt[s]))] for s in range(win.W)]
ctx.select_correspondences_window(sel)
print("window selection %s: %s" % ([None if x is None else len(x) for x in sel], sha(*[a for s in range(win.W) for a in ctx.get_correspondences(s)])))
ctx.close()

# ---- the batch association
K = 5
bw = synth.make_window(W=K, pts_per_scan=4000, seed=synth.SEED_BASE + 7202, perturb=(0.03, 0.2, 0.0), scan_radius=14.0, map_density=1.0)
tlb = np.array(bw.opts.t_lb, np.float32)
clouds = []
for s in range(K):
    c = bw.scans[s].copy(); c[:, :3] -= tlb
    clouds.append(np.ascontiguousarray(c))
bposes = np.c_[bw.init.trans, bw.init.quat]
ci, cj = batch.pair_list(K, 2)
for local in (1, 0):
    lib.glio_debug_set_bassoc_local(local)
    ba = batch.BatchAssociation(K, 4096, 400000)
    for k in range(K):
        ba.set_frame(k, clouds[k])
    counts, total = ba.run(bposes, ci, cj)
    h1 = sha(counts, *ba.read())
    counts, total = ba.run(bposes, ci, cj)                      # (again: the local tables are built now)
    print("batch %d pairs local tables %d shared bins %d total %d: %s again %s" % (len(ci), local, bins, total, h1, sha(counts, *ba.read())))
    ba.close()
lib.glio_debug_set_bassoc_local(1)

# ---- the on-stream draw selection
ba = batch.BatchAssociation(K, 4096, 400000)
for k in range(K):
    ba.set_frame(k, clouds[k])
ba.reset()
pc = np.array([4, 4, 4, 4], np.int32); pj = np.array([0, 1, 2, 3], np.int32)
ba.run_append(bposes, pc, pj, wait=False)
ba.select_tail_draws(25, np.random.default_rng(9).integers(0, 1 << 62, 25 * len(pc), dtype=np.uint64))
counts, total = ba.finish()
print("draws %d pairs found %s held %d shared bins %d: %s" % (len(pc), counts.tolist(), total, bins, sha(*ba.read())))
ba.close()

# ---- the local map (its voxel key), K1 from the device, a window association on that map
W = 3
lw = synth.make_window(W=5, pts_per_scan=3000, seed=synth.SEED_BASE + 7203, scan_radius=25.0)
o = synth.default_opts(W, pts=4096, map_pts=1 << 15)
ctx = capi.Context(o)
ctx.localmap_config(4, 0.4, 4096)
hs, ns = [], []
ltlb = np.array(lw.opts.t_lb, np.float32)
for s in range(lw.W):
    c = lw.scans[s].copy(); c[:, :3] -= ltlb
    ctx.localmap_push(np.ascontiguousarray(c), lw.gt.quat[s], lw.gt.trans[s])
    ns.append(ctx.localmap_build()); hs.append(ctx.localmap_read())
lp = [capi.lidar_pose(lw.opts, lw.gt.quat[s], lw.gt.trans[s]) for s in range(W)]
for s in range(W):
    ctx.set_scan(s, lw.scans[s])
cnt = ctx.associate_window(np.array([p[0] for p in lp]), np.array([p[1] for p in lp]))
print("localmap width 4 voxels %s: %s  window on it kept %s: %s" % (ns, sha(*hs), cnt.tolist(), sha(*[a for s in range(W) for a in ctx.get_correspondences(s)])))
ctx.close()

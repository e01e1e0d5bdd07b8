"""Bits of the point-cloud stages, for A/B runs of two builds of the library (GLIO_HIP_LIB selects one; a fresh process per build): one sha256 per case
over everything the stage hands back.  Two builds that compute the same print the same lines.  The cases are the smallest shapes at which the routines of
csrc/cloud_device.h (transformCloud, the bounding box, the workgroup scan and rank, the radix pass) and the local map's table routines can still go wrong:
  local map     width 4 x 3000 points, 7 keyframes (pushes, builds, evictions past the ring) under both accumulations, by bitmap rank and by radix sort
                (GLIO_LM_SORT=1); builds of 1000 and of 1025 voxels (one partial tile, two tiles); the LARGE case of tests/localmap_cases.py (294 912 voxels:
                k_rs_scan beyond its register path, three digits); glio_localmap_push_scan with a LiDAR offset; glio_localmap_rebuild_from_frames on three
                frames of unequal sizes (the ring takes no empty frame from a rebuild, so the empty keyframe of the case is an empty PUSH into the ring of
                the push_scan case)
  global map    3 frames x 2500 points at 0.2 and 0.4 m; an append that opens voxels and adds to stored ones; a call that straddles zero on every axis; one call
                of 70 000 points (more than GM_SCAN_CHUNK x GM_SORT_TILE: every scan kernel over two chunks); an extent of four digits
  loop closure  glio_loop_build_submap (2 + 5 frames), glio_loop_align on them: the submaps, the transform, the correspondences, the fallback list
  features      a 16-line and a 32-line synthetic scan: every output cloud and the counts
    GLIO_HIP_LIB=<library> python scripts/cloud_bits_ab.py > bits.txt"""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import localmap_cases as lc
from glio_amd import batch, capi, features, loop, mapping, synth, synth_lidar
from glio_amd import ctypes_types as T


def sha(*parts):
    m = hashlib.sha256()
    for p in parts:
        m.update(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes())
    return m.hexdigest()[:16]


def lm_context(width, cap, max_map, mode, sort, scan_pts=None, W=1):
    o = synth.default_opts(W, pts=scan_pts or cap, map_pts=max_map)
    os.environ["GLIO_LM_SORT"] = "1" if sort else "0"          # (read when the ring is allocated)
    try:
        ctx = capi.Context(o)
        ctx.localmap_config(width, lc.LEAF, cap)
    finally:
        os.environ.pop("GLIO_LM_SORT", None)
    ctx.localmap_set_accumulation(mode)
    return ctx


def body_clouds(win):
    tlb = np.array(win.opts.t_lb, np.float32)
    out = []
    for s in range(win.W):
        c = win.scans[s].copy(); c[:, :3] -= tlb
        out.append(np.ascontiguousarray(c))
    return out


# ---- local map: pushes, builds, evictions
win = synth.make_window(W=7, pts_per_scan=3000, seed=synth.SEED_BASE + 4101, scan_radius=25.0)
clouds = body_clouds(win)
for mode in (0, 1):
    for sort in (0, 1):
        ctx = lm_context(4, 4096, 1 << 15, mode, sort)
        hs, ns = [], []
        for s in range(win.W):
            ctx.localmap_push(clouds[s], win.gt.quat[s], win.gt.trans[s])
            ns.append(ctx.localmap_build()); hs.append(ctx.localmap_read())
        path = int(ctx.localmap_stats()[3])
        ctx.close()
        print("localmap width 4 x 3000 accumulation %d sort %d path %d voxels %s: %s" % (mode, sort, path, ns, sha(*hs)))

# ---- one partial tile, two tiles
rng = np.random.default_rng(4102)
cells = np.stack(np.meshgrid(np.arange(-6, 7), np.arange(-6, 7), np.arange(-6, 7), indexing="ij"), -1).reshape(-1, 3)
cells = cells[rng.permutation(len(cells))]
for nv in (1000, 1025):
    pts = lc.lattice_points(np.repeat(cells[:nv], 2, axis=0)[rng.permutation(2 * nv)], rng)
    for mode in (0, 1):
        for sort in (0, 1):
            ctx = lm_context(2, 4096, 4096, mode, sort)
            ctx.localmap_push(pts, *lc.IDENT)
            n = ctx.localmap_build()
            assert n == nv, (n, nv)
            print("localmap %d voxels accumulation %d sort %d: %s" % (nv, mode, sort, sha(ctx.localmap_read())))
            ctx.close()

# ---- LARGE
frames = lc.large_map_case()
for mode in (0, 1):
    for sort in (0, 1):
        ctx = lm_context(lc.LARGE_WIDTH, lc.LARGE_CAP, lc.LARGE_MAX_MAP, mode, sort, scan_pts=1024)
        for f in frames:
            ctx.localmap_push(f, *lc.IDENT)
        n = ctx.localmap_build()
        st = ctx.localmap_stats()
        print("localmap LARGE accumulation %d sort %d path %d passes %d voxels %d: %s" % (mode, sort, st[3], st[4], n, sha(ctx.localmap_read())))
        ctx.close()
del frames

# ---- push_scan with a LiDAR offset (and an empty keyframe in the ring)
W = 3
tlb = np.array([0.05, -0.02, 0.1], np.float32)
for sort in (0, 1):
    ctx = lm_context(4, 4096, 1 << 15, 0, sort, W=W)
    hs = []
    for s in range(win.W):
        if s > 0:
            ctx.slide_window()
        if s == 3:
            ctx.localmap_push(np.zeros((0, 4), np.float32), win.gt.quat[s], win.gt.trans[s])
        else:
            ctx.set_scan(W - 1, win.scans[s])
            ctx.localmap_push_scan(W - 1, tlb, win.gt.quat[s], win.gt.trans[s])
        ctx.localmap_build(); hs.append(ctx.localmap_read())
    ctx.close()
    print("localmap push_scan offset %s sort %d: %s" % (tlb.tolist(), sort, sha(*hs)))

# ---- rebuild from frames of unequal sizes
sizes = (3000, 1, 1777)
ba = batch.BatchAssociation(3, 4096, 16)
for k, n in enumerate(sizes):
    ba.set_frame(k, clouds[k][:n])
poses = np.c_[win.gt.trans[:3], win.gt.quat[:3]]
for mode in (0, 1):
    for sort in (0, 1):
        ctx = lm_context(4, 4096, 1 << 15, mode, sort)
        n = ctx.localmap_rebuild_from_frames(ba, np.arange(3, dtype=np.int32), poses)
        h = [ctx.localmap_read()]
        ctx.localmap_push(clouds[3], win.gt.quat[3], win.gt.trans[3]); ctx.localmap_push(clouds[4], win.gt.quat[4], win.gt.trans[4])      # (evicts frame 0)
        n2 = ctx.localmap_build(); h.append(ctx.localmap_read())
        ctx.close()
        print("localmap rebuild_from_frames %s accumulation %d sort %d voxels %d then %d: %s" % (sizes, mode, sort, n, n2, sha(*h)))
ba.close()


# ---- global map
def gm_frames(n_frames, pts, seed, centre, radius=35.0, step=0.5):
    rng = np.random.default_rng(seed)
    scene = synth.make_scene()
    c0 = np.asarray(centre, float)
    scans = []
    for k in range(n_frames):
        p, _ = synth.sample_scene(scene, pts, rng, centre=c0, radius=radius)
        scans.append(np.ascontiguousarray(np.c_[p - c0, rng.uniform(0, 100, pts)], np.float32))
    poses = np.array([np.r_[c0 + k * np.array([step, 0.02 * step, 0.0]), synth.rotvec_q(np.array([0.0, 0.0, 0.002 * k]))] for k in range(n_frames)])
    return scans, poses


scans, poses = gm_frames(5, 2500, 4103, (40.0, 0.5, 1.8))
ba = batch.BatchAssociation(5, 4096, 16)
for k, s in enumerate(scans):
    ba.set_frame(k, s)
for leaf in (0.2, 0.4):
    gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=leaf, max_voxels=1 << 16, max_points_per_add=1 << 14))
    i1 = gm.add([0, 1, 2], poses[:3]); m1 = gm.read()
    i2 = gm.add([3, 4], poses[3:]); m2 = gm.read()              # the next frames overlap the first: new voxels and stored ones
    assert i2.n_voxels > i1.n_voxels and i2.n_voxels < i1.n_voxels + 5000
    gm.close()
    print("gmap 3 x 2500 leaf %.1f passes %d voxels %d: %s  append 2 x 2500 passes %d voxels %d: %s" % (leaf, i1.radix_passes, i1.n_voxels, sha(m1), i2.radix_passes, i2.n_voxels, sha(m2)))
# a call that straddles zero on every axis: the frames' own (sensor-centred) clouds at poses around the origin
zero_poses = poses.copy(); zero_poses[:, :3] = np.array([[0.3, -0.2, 0.1], [-0.4, 0.1, -0.3], [0.2, 0.3, -0.1], [0, 0, 0], [0, 0, 0]])
gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=0.2, max_voxels=1 << 16, max_points_per_add=1 << 14))
i = gm.add([0, 1, 2], zero_poses[:3]); m = gm.read()
assert np.all(m[:, :3].min(0) < 0) and np.all(m[:, :3].max(0) > 0)
gm.close()
print("gmap straddles zero passes %d voxels %d: %s" % (i.radix_passes, i.n_voxels, sha(m)))
# four digits: two frames 400 m apart on x and on y, 10 m on z (12 + 12 + 7 or 8 bits of extent at 0.2 m)
far = poses[:2].copy(); far[1, :3] += np.array([400.0, 400.0, 10.0])
gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=0.2, max_voxels=1 << 16, max_points_per_add=1 << 14))
i = gm.add([0, 1], far); m = gm.read()
assert i.radix_passes == 4, i.radix_passes
gm.close()
print("gmap wide extent passes %d voxels %d: %s" % (i.radix_passes, i.n_voxels, sha(m)))
ba.close()
# more than GM_SCAN_CHUNK x GM_SORT_TILE = 65 536 points in one call
scans, poses = gm_frames(2, 35000, 4104, (40.0, 0.5, 1.8))
ba = batch.BatchAssociation(2, 35000, 16)
for k, s in enumerate(scans):
    ba.set_frame(k, s)
gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=0.2, max_voxels=1 << 17, max_points_per_add=1 << 17))
i = gm.add([0, 1], poses); m = gm.read()
gm.close(); ba.close()
print("gmap one call of 70000 points passes %d voxels %d: %s" % (i.radix_passes, i.n_voxels, sha(m)))

# ---- loop closure
Q_BL = synth.rotvec_q(np.array([0.01, -0.02, 0.015]))
T_BL = np.array([0.05, -0.02, 0.1])
nf = 7
dscans = synth_lidar.drive(n_frames=nf, n_scans=16, n_az=900, step=(0.5, 0.02, 0.0), yaw_step=0.004)
dclouds = [np.ascontiguousarray(sc[np.isfinite(sc[:, :3]).all(axis=1)][::3], np.float32) for sc in dscans]
info = np.array([np.r_[np.array([40.0, 0.5, 1.8]) + k * np.array([0.5, 0.02, 0.0]), synth.rotvec_q(np.array([0.0, 0.0, 0.004 * k]))] for k in range(nf)])
ba = batch.BatchAssociation(nf, 8192, 16)
for k, c in enumerate(dclouds):
    ba.set_frame(k, c)
lp = loop.LoopClosure(ba, loop.default_opts(max_target_points=1 << 17, max_source_points=1 << 16))
src_f, tgt_f = [6, 5], [0, 1, 2, 3, 4]
ns = lp.build_submap(loop.SOURCE, src_f, loop.frame_poses(info[src_f], Q_BL, T_BL))
nt = lp.build_submap(loop.TARGET, tgt_f, loop.frame_poses(info[tgt_f], Q_BL, T_BL))
src, tgt = lp.read_submap(loop.SOURCE), lp.read_submap(loop.TARGET)
r = lp.align()
idx, d2 = lp.read_correspondences(ns)
fb = lp.fallbacks()
print("loop submaps %d + %d: %s  align iterations %d state %d: transform %s correspondences %s fallbacks %s: %s current %s" % (
    ns, nt, sha(src, tgt), r.iterations, r.state, sha(np.asarray(r.transform, np.float64)), sha(idx, d2), fb.tolist(), sha(fb), sha(lp.read_current())))
lp.close(); ba.close()

# ---- features
for lines in (16, 32):
    raw = synth_lidar.make_scan(lines, 300 if lines == 16 else 200, sweep_yaw=0.05, seed=5)
    ctx = capi.Context(synth.default_opts(1, pts=1 << 14, map_pts=1 << 14))
    ctx.features_config(features.default_opts(lines))
    c = ctx.features_extract(raw, np.array([np.cos(0.025), 0, 0, np.sin(0.025)]))
    outs = [ctx.features_read(w) for w in (T.FEAT_SURF, T.FEAT_EDGE_LESS_SHARP, T.FEAT_SHARP, T.FEAT_FLAT, T.FEAT_CUT_CLOUD)]
    ctx.close()
    print("features %d lines %d points counts %s: %s" % (lines, len(raw), c.as_dict(), sha(*outs)))

"""The global map restated in numpy, and the cases tests/test_hip_global_map.py (GPU) and tests/test_global_map_cpu.py (CPU) share.

restated_voxel_grid: pcl::VoxelGrid as include/glio_hip.h states it for glio_gmap_* -- a 63-bit ABSOLUTE key per point (21 biased bits per axis of
floorf(p * (1.0f / leaf)), iz highest), a STABLE sort by that key, per run the four channels summed sequentially in float32, divided by the float32 count.
No bounding box enters: PCL's linear index ix + iy dx + iz dx dy orders voxels by (iz, iy, ix) whatever the box is."""
import numpy as np

BIAS = 1 << 20


def voxel_keys(pts, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    c = np.floor(np.ascontiguousarray(pts, np.float32)[:, :3] * inv).astype(np.int64)
    assert (c >= -BIAS).all() and (c < BIAS).all()
    return ((c[:, 2] + BIAS) << 42) | ((c[:, 1] + BIAS) << 21) | (c[:, 0] + BIAS)


def restated_voxel_grid(pts, leaf):
    pts = np.ascontiguousarray(pts, np.float32)
    key = voxel_keys(pts, leaf)
    order = np.argsort(key, kind="stable")
    ks, ps = key[order], pts[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    start = np.flatnonzero(head)
    length = np.diff(np.r_[start, len(ks)])
    acc = np.zeros((len(start), 4), np.float32)
    for t in range(int(length.max())):                      # the t-th point of every run that has one: sequential float32 sums, run by run
        live = length > t
        acc[live] = acc[live] + ps[start[live] + t]
    return acc / length.astype(np.float32)[:, None], ks[start]


def box_cells(pts, leaf):
    """cells of the bounding box as PCL counts them (dx dy dz), as a Python int"""
    inv = np.float32(1.0) / np.float32(leaf)
    c = np.floor(np.ascontiguousarray(pts, np.float32)[:, :3] * inv).astype(np.int64)
    d = c.max(axis=0) - c.min(axis=0) + 1
    return int(d[0]) * int(d[1]) * int(d[2])


# ---- the cases
K, CAP = 8, 8192
CUT = {3: 1, 4: 1023, 5: 4097}            # ragged frames, as tests/test_hip_localmap_rebuild.py cuts them


def window_case():
    """8 keyframes of 5000 points (the fixture of tests/test_hip_localmap_rebuild.py), some cut short; body clouds = scan - t_lb; the poses the clouds arrived
    with and the corrected ones (moved by ~0.3 m / 2 degrees).  -> clouds, old [K][7], new [K][7] (t, q)"""
    from glio_amd import synth
    win = synth.make_window(W=K, pts_per_scan=5000, seed=synth.SEED_BASE + 81, scan_radius=25.0)
    tlb = np.array(win.opts.t_lb, np.float32)
    clouds = []
    for s in range(K):
        c = np.ascontiguousarray(win.scans[s][:CUT.get(s, len(win.scans[s]))]).copy()
        c[:, :3] -= tlb
        clouds.append(np.ascontiguousarray(c))
    rng = np.random.default_rng(11)
    old = np.zeros((K, 7)); new = np.zeros((K, 7))
    for s in range(K):
        old[s, :3], old[s, 3:] = win.gt.trans[s], win.gt.quat[s]
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        half = np.deg2rad(2.0) / 2
        q = synth.qmul(np.array([np.cos(half), *(np.sin(half) * ax)]), win.gt.quat[s])
        d = rng.normal(size=3); d *= 0.3 / np.linalg.norm(d)
        new[s, :3], new[s, 3:] = win.gt.trans[s] + d, q / np.linalg.norm(q)
    return clouds, old, new


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def pose_at(x, y, z, yaw=0.0):
    return np.array([x, y, z, np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])


def faces_cloud():
    """negative coordinates and points exactly on voxel faces: a lattice of multiples of 0.2 over [-3, 3) x [-2, 2) x [-1, 1) (every coordinate a face of the
    0.2 grid as far as float32 has it, every other one of the 0.4 grid), each lattice point twice more with a small offset either way; added at the identity pose,
    which transformCloud applies exactly"""
    g = np.stack(np.meshgrid(np.arange(-15, 15), np.arange(-10, 10), np.arange(-5, 5), indexing="ij"), -1).reshape(-1, 3)
    lat = (g.astype(np.float32) * np.float32(0.2)).astype(np.float32)
    rng = np.random.default_rng(3)
    eps = rng.uniform(1e-4, 0.05, lat.shape).astype(np.float32)
    xyz = np.vstack([lat, lat - eps, lat + eps]).astype(np.float32)
    return np.ascontiguousarray(np.c_[xyz, rng.uniform(0, 100, len(xyz)).astype(np.float32)].astype(np.float32))


def far_case():
    """two overlapping clouds of 2000 points near the origin and a third one 3 km away along x and y: at leaf 0.2 the bounding box holds ~1.1e10 cells, more
    than INT32_MAX (PCL 1.8.1 would pass the cloud through unfiltered) -> clouds [3], poses [3][7]"""
    rng = np.random.default_rng(5)
    clouds = [np.ascontiguousarray(np.c_[rng.uniform(-20, 20, (2000, 2)), rng.uniform(-2, 6, 2000), rng.uniform(0, 100, 2000)].astype(np.float32)) for _ in range(3)]
    poses = np.array([pose_at(0.0, 0.0, 0.0), pose_at(0.3, -0.2, 0.05, 0.02), pose_at(3000.0, 3000.0, 0.0, 0.5)])
    return clouds, poses


def one_voxel_case():
    """5000 points inside ONE 0.2 m voxel around (1000.3, -2000.5, 10.1) (voxel (5001, -10003, 50): its faces are 0.1 m away, the points within 0.08 m): a run
    longer than any tile of the sort -> cloud, pose"""
    rng = np.random.default_rng(9)
    c = np.c_[rng.uniform(-0.08, 0.08, (5000, 3)), rng.uniform(0, 100, 5000)].astype(np.float32)
    return np.ascontiguousarray(c), pose_at(1000.3, -2000.5, 10.1)


def ring_case(n_frames=80):
    """80 entries over the 8 keyframes of window_case (so every index repeats), each at a pose on a ring of 30 m radius -> frames [80], poses [80][7]"""
    frames = [(3 * i + i // 8) % K for i in range(n_frames)]
    poses = np.array([pose_at(30.0 * np.cos(2 * np.pi * i / n_frames), 30.0 * np.sin(2 * np.pi * i / n_frames), 0.1 * (i % 5), 2 * np.pi * i / n_frames + 1.0)
                      for i in range(n_frames)])
    return frames, poses


def sort_constants():
    """the #defines of glio_amd/csrc/globalmap_kernels.hip that bound what one wavefront / workgroup of the sort and of the run scan covers"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glio_amd", "csrc", "globalmap_kernels.hip")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (GM_[A-Z_]+) (\d+)\b", src)}

"""Inputs at which the device-resident local map (glio_amd/csrc/localmap_kernels.hip) changes its path, a float64 reference of its default
(fixed-point) centroids and the host's view of its voxel table.  The local-map tests push at most 7 keyframes into a table twenty times too
large, so none of these is reached there:

  drive_case()         40 keyframes through a table sized for 6000 voxels: the tombstone rebuild every few keyframes
  small_table_clouds() clouds of 40 .. 200 distinct voxels for a 128-slot table: both refusals of a build and what follows them
  box_cases()          bounding boxes of exactly 2^27 cells and of one slice more: the bitmap / radix switch
  large_map_case()     more than 262 144 voxels: the radix sort's scan beyond its register path
  dense_voxel_case()   one voxel holding thousands of points: the in-thread sort of the float accumulation

exact_centroids() restates pcl::VoxelGrid's voxel assignment with the oracle's float formulas and accumulates in float64;
simulate_table() applies the host's rule for the rebuild.  tests/test_localmap_cases_cpu.py proves with the oracle alone that every case takes
its branch; tests/test_hip_localmap_limits.py runs them on the device.

No GPU and no library in here: numpy and glio_amd.synth only (clouds are moved into the map frame by the caller, with the oracle)."""
import numpy as np

from glio_amd import synth

LEAF = 0.4
BM_MAX_BITS = 1 << 27            # cells of the occupancy bitmap (localmap_kernels.hip)
RS_TILE = 1024                   # voxels per tile of the radix sort
RS_SCAN_TILES = 256              # tiles the scan keeps in registers: more take its loop
IDENT = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3))


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def table_cap(max_map_points):
    return next_pow2(2 * max_map_points)


# ------------------------------------------------------------------------------------------------ references
def voxel_coords(points, leaf):
    """absolute voxel coordinates, floorf(p * inv_leaf) in float as the oracle and the device form them -> [n][3] int64"""
    inv = np.float32(1) / np.float32(leaf)
    return np.floor(np.asarray(points, np.float32)[:, :3] * inv).astype(np.int64)


def voxel_keys(points, leaf):
    """one integer per absolute voxel (what the device's table is keyed by)"""
    v = voxel_coords(points, leaf) + (1 << 20)
    assert v.min() >= 0 and v.max() < (1 << 21)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def grid_geometry(points, leaf):
    """pcl::VoxelGrid's min_b, div_b of a cloud (float min / max, floorf(x * inv))"""
    pts = np.asarray(points, np.float32)
    inv = np.float32(1) / np.float32(leaf)
    min_b = np.floor(pts[:, :3].min(0) * inv).astype(np.int64)
    div_b = np.floor(pts[:, :3].max(0) * inv).astype(np.int64) - min_b + 1
    return min_b, div_b


def exact_centroids(points, leaf):
    """pcl::VoxelGrid's voxel assignment (the oracle's float formulas: inv = 1.f / leaf, floorf(p * inv) - (float) min_b, linear index over the
    bounding box) with the centroids accumulated in float64 -> (centroids [nv][4] float64 by ascending linear index, the indices [nv] int64)"""
    pts = np.ascontiguousarray(points, np.float32)
    if len(pts) == 0:
        return np.zeros((0, 4)), np.zeros(0, np.int64)
    inv = np.float32(1) / np.float32(leaf)
    min_b, div_b = grid_geometry(pts, leaf)
    rel = (np.floor(pts[:, :3] * inv) - min_b.astype(np.float32)).astype(np.int64)
    lin = rel[:, 0] + rel[:, 1] * div_b[0] + rel[:, 2] * div_b[0] * div_b[1]
    idx, inverse, counts = np.unique(lin, return_inverse=True, return_counts=True)
    cen = np.stack([np.bincount(inverse, weights=pts[:, c].astype(np.float64), minlength=len(idx)) for c in range(4)], axis=1) / counts[:, None]
    return cen, idx


def simulate_table(voxel_sets, width, max_map_points):
    """The host's view of the voxel table over a drive: voxel_sets[b] = the set of voxel keys of keyframe b (in the map frame); every keyframe is
    pushed and then built.  The table claims a slot for every distinct key since its last clear; a build whose PREVIOUS build saw more than
    table_cap / 2 claimed keys clears the table and re-inserts the ring.  Returns a dict: rebuilds (the builds that rebuild, 0-based), peak
    (largest number of claimed keys, reached after a push and before its build), keys (claimed keys after every build), live (voxels per build),
    table_cap."""
    cap = table_cap(max_map_points)
    claimed, nkeys_seen = set(), 0
    rebuilds, keys, live = [], [], []
    peak = 0
    for b, vs in enumerate(voxel_sets):
        ring = set().union(*voxel_sets[max(0, b + 1 - width):b + 1])
        claimed |= set(vs)
        peak = max(peak, len(claimed))
        if nkeys_seen > cap // 2:
            claimed = set(ring)
            rebuilds.append(b)
        nkeys_seen = len(claimed)
        keys.append(nkeys_seen)
        live.append(len(ring))
    return dict(rebuilds=rebuilds, peak=peak, keys=keys, live=live, table_cap=cap)


def radix_passes(points, leaf):
    """8-bit passes the radix sort needs for the linear indices of this cloud's bounding box"""
    _, div_b = grid_geometry(points, leaf)
    span = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    bits = 1
    while bits < 63 and (1 << bits) < span:
        bits += 1
    return (bits + 7) // 8


# ------------------------------------------------------------------------------------------------ clouds on a voxel lattice
def lattice_points(voxels, rng, leaf=LEAF):
    """one point inside each listed voxel (absolute integer coordinates [n][3]), at (index + u) * leaf with u in [0.125, 0.875]: never near a face, so
    the float32 product p * inv_leaf falls into the intended voxel; intensity in [0, 100)"""
    voxels = np.asarray(voxels, np.int64)
    u = rng.uniform(0.125, 0.875, size=voxels.shape)
    out = np.empty((len(voxels), 4), np.float32)
    out[:, :3] = ((voxels + u) * leaf).astype(np.float32)
    out[:, 3] = rng.uniform(0.0, 100.0, len(voxels)).astype(np.float32)
    assert np.array_equal(voxel_coords(out, leaf), voxels)
    return out


# ------------------------------------------------------------------------------------------------ the drive
DRIVE_W, DRIVE_WIDTH, DRIVE_MAX_MAP, DRIVE_CAP = 40, 4, 6000, 2048


def drive_case():
    """(win, body-frame clouds, ground-truth poses (q, t)) of a 40-keyframe drive"""
    win = synth.make_window(W=DRIVE_W, pts_per_scan=1500, seed=synth.SEED_BASE + 81, scan_radius=25.0, kf_dt=0.1)
    tlb = np.array(win.opts.t_lb, np.float32)
    clouds = []
    for s in range(win.W):
        c = win.scans[s].copy(); c[:, :3] -= tlb
        clouds.append(np.ascontiguousarray(c))
    poses = [(win.gt.quat[s].copy(), win.gt.trans[s].copy()) for s in range(win.W)]
    return win, clouds, poses


# ------------------------------------------------------------------------------------------------ a 128-slot table
SMALL_MAX_MAP, SMALL_WIDTH, SMALL_CAP = 64, 2, 1024


def small_table_clouds():
    """Clouds over one list of 200 distinct voxels: big100 = voxels [0, 100) (more than max_map_points = 64, fits the 128-slot table), big200 = all of
    them (more than the table has slots), a = [0, 40), b = [20, 60), c = [30, 70): any two neighbours of a, b, c together hold 60 / 50 voxels.
    One to three points per voxel."""
    rng = np.random.default_rng(synth.SEED_BASE + 8101)
    cells = np.stack(np.meshgrid(np.arange(-4, 4), np.arange(-4, 4), np.arange(-4, 4), indexing="ij"), -1).reshape(-1, 3)
    vox = cells[rng.permutation(len(cells))[:200]]

    def cloud(lo, hi):
        reps = rng.integers(1, 4, hi - lo)
        pts = lattice_points(np.repeat(vox[lo:hi], reps, axis=0), rng)
        return np.ascontiguousarray(pts[rng.permutation(len(pts))])
    return dict(big100=cloud(0, 100), big200=cloud(0, 200), a=cloud(0, 40), b=cloud(20, 60), c=cloud(30, 70))


# ------------------------------------------------------------------------------------------------ the bitmap's limit
BOX_MAX_MAP, BOX_CAP = 4096, 4096
BOX_ORIGIN = -60                 # absolute voxel coordinate of the box's corner: the base cloud lies within 24 m of the origin


def box_cases():
    """(base cloud, [(name, cloud, expected path)]): a base cloud of about 2000 points in voxels [0, 120)^3 relative to a corner voxel it always
    contains, plus single-point voxels (relative coordinates) that stretch the bounding box:
      exact_corner   (511,511,511): 512^3 = 2^27 cells exactly, largest index 2^27 - 1             -> bitmap rank
      exact_faces    (511,0,0) (0,511,0) (0,0,511): 2^27 cells, every index well below            -> bitmap rank
      over_corner    (512,511,511): 513 x 512 x 512 cells, an index >= 2^27 (no bit for it)        -> radix sort
      over_span_only (512,0,0) (0,511,0) (0,0,511): 513 x 512 x 512 cells but every index < 2^27: only the span rule takes the bitmap away, and
                     every voxel has set a bit that the radix path's emit must clear               -> radix sort"""
    rng = np.random.default_rng(synth.SEED_BASE + 8102)
    rel = np.unique(rng.integers(0, 120, size=(1500, 3)), axis=0)
    rel = np.vstack([[[0, 0, 0]], rel[np.any(rel != 0, axis=1)]])
    rel = np.vstack([rel, rel[rng.integers(0, len(rel), 2000 - len(rel))]])           # some voxels hold several points
    base = lattice_points(rel[rng.permutation(len(rel))] + BOX_ORIGIN, rng)
    extra = dict(exact_corner=[(511, 511, 511)], exact_faces=[(511, 0, 0), (0, 511, 0), (0, 0, 511)],
                 over_corner=[(512, 511, 511)], over_span_only=[(512, 0, 0), (0, 511, 0), (0, 0, 511)])
    path = dict(exact_corner=1, exact_faces=1, over_corner=2, over_span_only=2)
    cases = []
    for name, vs in extra.items():
        far = lattice_points(np.array(vs, np.int64) + BOX_ORIGIN, rng)
        cl = np.vstack([base, far])
        cases.append((name, np.ascontiguousarray(cl[rng.permutation(len(cl))]), path[name]))
    return base, cases


# ------------------------------------------------------------------------------------------------ more than 256 tiles
LARGE_WIDTH, LARGE_CAP, LARGE_MAX_MAP = 6, 65536, 1 << 19
LARGE_DIMS = (72, 64, 64)        # 294 912 voxels > 262 144
LARGE_ORIGIN = (-36, -32, -32)   # a whole number of leaves: the lattice's voxels are the grid's


def large_map_case():
    """6 keyframes x 65 536 points (identity poses): one point in every voxel of a 72 x 64 x 64 lattice, the remaining 98 304 thrown at random into
    the same voxels; the points are dealt to the keyframes in random order"""
    rng = np.random.default_rng(synth.SEED_BASE + 8103)
    cells = np.stack(np.meshgrid(*[np.arange(d) for d in LARGE_DIMS], indexing="ij"), -1).reshape(-1, 3) + np.array(LARGE_ORIGIN)
    n = LARGE_WIDTH * LARGE_CAP
    vox = np.vstack([cells, cells[rng.integers(0, len(cells), n - len(cells))]])
    pts = lattice_points(vox[rng.permutation(n)], rng)
    return [np.ascontiguousarray(pts[k * LARGE_CAP:(k + 1) * LARGE_CAP]) for k in range(LARGE_WIDTH)]


# ------------------------------------------------------------------------------------------------ a voxel that holds thousands of points
DENSE_WIDTH, DENSE_CAP, DENSE_MAX_MAP, DENSE_POINTS = 4, 8192, 2048, 3000
DENSE_VOXEL = (3, -2, 1)


def dense_voxel_case():
    """(four keyframes, one cloud): voxel DENSE_VOXEL receives 3000 points, 750 from each of four keyframes, next to about 500 ordinary voxels (2000
    points); and the four keyframes as ONE cloud, to be pushed four times at the same pose (every voxel then holds four times its points: 12 000 in
    the dense one)"""
    rng = np.random.default_rng(synth.SEED_BASE + 8104)
    others = np.unique(rng.integers(-10, 10, size=(520, 3)), axis=0)
    others = others[np.any(others != np.array(DENSE_VOXEL), axis=1)]
    vox = np.vstack([np.tile(np.array(DENSE_VOXEL), (DENSE_POINTS, 1)), others[rng.integers(0, len(others), 2000)]])
    pts = lattice_points(vox[rng.permutation(len(vox))], rng)
    dense = np.all(voxel_coords(pts, LEAF) == np.array(DENSE_VOXEL), axis=1)
    di, oi = np.flatnonzero(dense), np.flatnonzero(~dense)
    frames = []
    for k in range(DENSE_WIDTH):
        sel = np.concatenate([di[k::DENSE_WIDTH], oi[k::DENSE_WIDTH]])
        frames.append(np.ascontiguousarray(pts[sel[rng.permutation(len(sel))]]))
    return frames, np.ascontiguousarray(pts)

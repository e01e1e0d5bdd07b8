"""GPU: the device-resident local map over a long drive and at the limits of its tables (cases of tests/localmap_cases.py; that every case takes
its branch is shown on the CPU by tests/test_localmap_cases_cpu.py, and glio_debug_localmap_stats says which branch the device took).

Every build is compared in BOTH accumulation modes:
  mode 1 (pcl::VoxelGrid's float sums in concatenation order): the map equals the oracle's voxel grid of the oracle-transformed concatenation bit
         for bit;
  mode 0 (the default, exact fixed point): the same count and every component within 2^-21 + spacing(float32(|c|)) of localmap_cases.exact_centroids
         (float64 sums).  The device rounds every point to the 2^-20 grid (<= 2^-21 each, the mean no worse), adds exact integers, divides once in
         double and rounds once to float: half an ulp, and half an ulp of margin for the cast.  A bound, not a measurement: every test prints the
         largest observed fraction of it.

Every test prints `[localmap-limits] <case> mode <m>: mode-0 max diff / gate = ..., stats = [...]` (pytest -s): the largest mode-0 difference as a
fraction of its gate and the vector of glio_debug_localmap_stats after the case's last build."""
import os

import numpy as np
import pytest

import localmap_cases as lc
from glio_amd import synth

pytestmark = pytest.mark.gpu

MODES = (0, 1)


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


class Ref:
    """both references of one concatenated map-frame cloud, computed once"""

    def __init__(self, po, cloud):
        self.oracle, _ = po.voxel_grid(cloud, lc.LEAF) if len(cloud) else (np.zeros((0, 4), np.float32), None)
        self.exact, _ = lc.exact_centroids(cloud, lc.LEAF)
        assert len(self.oracle) == len(self.exact)


class Worst:
    def __init__(self):
        self.ratio = 0.0


def _compare(n, got, ref, mode, worst, tag):
    assert n == len(ref.oracle) == len(got), f"{tag}: {n} voxels, read {len(got)}, oracle {len(ref.oracle)}"
    if n == 0:
        return
    if mode == 1:
        assert np.array_equal(got, ref.oracle), f"{tag}: float accumulation differs from the oracle, max {np.abs(got - ref.oracle).max()}"
    else:
        gate = 2.0 ** -21 + np.spacing(np.abs(ref.exact).astype(np.float32)).astype(np.float64)
        ratio = float((np.abs(got.astype(np.float64) - ref.exact) / gate).max())
        worst.ratio = max(worst.ratio, ratio)
        assert ratio <= 1.0, f"{tag}: fixed-point centroid off by {ratio:.3f} of its gate"


def _report(name, mode, worst, stats):
    print(f"[localmap-limits] {name} mode {mode}: mode-0 max diff / gate = {worst.ratio:.4f}, stats = {stats}")


def _context(width, cap, max_map, mode, force_sort=False, scan_pts=None):
    from glio_amd import capi
    o = synth.default_opts(1, pts=scan_pts or cap, map_pts=max_map)
    o.t_lb[:] = [0, 0, 0]
    os.environ["GLIO_LM_SORT"] = "1" if force_sort else "0"
    try:
        ctx = capi.Context(o)
        ctx.localmap_config(width, lc.LEAF, cap)
    finally:
        os.environ.pop("GLIO_LM_SORT", None)
    ctx.localmap_set_accumulation(mode)
    return ctx


def _push_build(ctx, cloud, pose=lc.IDENT):
    ctx.localmap_push(cloud, *pose)
    n = ctx.localmap_build()
    return n, ctx.localmap_read().copy()


# ------------------------------------------------------------------------------------------------ 1. the drive
@pytest.fixture(scope="module")
def drive(po):
    _, clouds, poses = lc.drive_case()
    glob = [po.transform_cloud(c, q, t) for c, (q, t) in zip(clouds, poses)]
    sim = lc.simulate_table([set(lc.voxel_keys(g, lc.LEAF).tolist()) for g in glob], lc.DRIVE_WIDTH, lc.DRIVE_MAX_MAP)
    refs = [Ref(po, np.vstack(glob[max(0, s + 1 - lc.DRIVE_WIDTH):s + 1])) for s in range(len(glob))]
    return clouds, poses, sim, refs


@pytest.mark.parametrize("mode", MODES)
def test_drive_through_a_table_that_fills_with_tombstones(drive, mode):
    """40 keyframes through a table of 16 384 slots that the drive fills with tombstones every four keyframes: every keyframe's map against the oracle,
    the rebuilds counted by the device where the host's rule puts them, and (mode 0) the final map byte for byte a fresh context's"""
    clouds, poses, sim, refs = drive
    assert len(sim["rebuilds"]) >= 3 and sim["peak"] < sim["table_cap"] and max(sim["live"]) <= lc.DRIVE_MAX_MAP
    ctx = _context(lc.DRIVE_WIDTH, lc.DRIVE_CAP, lc.DRIVE_MAX_MAP, mode)
    worst = Worst()
    for s in range(len(clouds)):
        n, got = _push_build(ctx, clouds[s], poses[s])
        _compare(n, got, refs[s], mode, worst, f"keyframe {s}")
        st = ctx.localmap_stats()
        assert st[1] == sim["keys"][s] and st[5] == sim["live"][s], f"keyframe {s}: {st}"
    st = ctx.localmap_stats()
    _report("drive", mode, worst, st)
    assert st[0] == sim["table_cap"] and st[2] == len(sim["rebuilds"]) >= 3 and st[1] == sim["keys"][-1]
    if mode == 0:
        fresh = _context(lc.DRIVE_WIDTH, lc.DRIVE_CAP, lc.DRIVE_MAX_MAP, mode)
        for s in range(len(clouds) - lc.DRIVE_WIDTH, len(clouds)):
            fresh.localmap_push(clouds[s], *poses[s])
        assert fresh.localmap_build() == n and np.array_equal(fresh.localmap_read(), got)
        assert fresh.localmap_stats()[2] == 0
        fresh.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. empty keyframes
@pytest.mark.parametrize("mode", MODES)
def test_empty_keyframes_and_an_empty_ring(po, drive, mode):
    clouds, poses = drive[0], drive[1]
    empty = np.zeros((0, 4), np.float32)
    seq = [0, None, 1, None, None, None, 2]                      # cloud, empty, cloud, empty, empty, empty, cloud
    width = 3
    ctx = _context(width, lc.DRIVE_CAP, lc.DRIVE_MAX_MAP, mode)
    glob = [None if k is None else po.transform_cloud(clouds[k], *poses[k]) for k in seq]
    worst = Worst()
    for s, k in enumerate(seq):
        n, got = _push_build(ctx, empty if k is None else clouds[k], lc.IDENT if k is None else poses[k])
        ring = [g for g in glob[max(0, s + 1 - width):s + 1] if g is not None]
        ref = Ref(po, np.vstack(ring) if ring else empty)
        _compare(n, got, ref, mode, worst, f"build {s}")
        st = ctx.localmap_stats()
        assert st[5] == len(ref.oracle) and (st[3] == 0) == (not ring), f"build {s}: {st}"
        if s == 5:                                               # three empty keyframes: an empty map, no error
            assert n == 0 and len(got) == 0 and st[3] == 0
            assert ctx.associate(0, clouds[3], *poses[3]) == 0   # nothing to associate against: 0 kept, no failure
            assert len(ctx.get_correspondences(0)[0]) == 0
        if s == 6:                                               # ... and the next push gives the oracle's map of that one cloud
            assert n == len(po.voxel_grid(glob[6], lc.LEAF)[0]) > 0
    _report("empty keyframes", mode, worst, ctx.localmap_stats())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. / 4. the two refusals
@pytest.fixture(scope="module")
def small(po):
    cl = lc.small_table_clouds()
    refs = {names: Ref(po, np.vstack([cl[n] for n in names])) for names in (("a", "b"), ("b", "c"))}
    return cl, refs


def _fresh_map(cl, names, mode):
    ctx = _context(lc.SMALL_WIDTH, lc.SMALL_CAP, lc.SMALL_MAX_MAP, mode)
    for nm in names:
        ctx.localmap_push(cl[nm], *lc.IDENT)
    n = ctx.localmap_build()
    got = ctx.localmap_read().copy()
    ctx.close()
    return n, got


@pytest.mark.parametrize("mode", MODES)
def test_too_many_voxels_is_refused_and_the_ring_stays_valid(small, mode):
    from glio_amd import capi
    cl, refs = small
    ctx = _context(lc.SMALL_WIDTH, lc.SMALL_CAP, lc.SMALL_MAX_MAP, mode)
    assert ctx.localmap_stats()[0] == 128
    worst = Worst()
    ctx.localmap_push(cl["big100"], *lc.IDENT)
    with pytest.raises(capi.GlioError) as e:
        ctx.localmap_build()
    assert "error -1" in str(e.value) and "100 voxels, max_map_points is 64" in str(e.value)
    ctx.localmap_push(cl["a"], *lc.IDENT)                        # the large cloud is still in the ring: refused again, for the same reason
    with pytest.raises(capi.GlioError) as e:
        ctx.localmap_build()
    assert "100 voxels, max_map_points is 64" in str(e.value)
    n, got = _push_build(ctx, cl["b"])                           # ... and evicted now
    _compare(n, got, refs[("a", "b")], mode, worst, "after the refusal")
    st = ctx.localmap_stats()
    _report("too many voxels", mode, worst, st)
    assert st[6] >= 1, "the refused builds left bits in the bitmap: the next build wipes it"
    assert st[1] == n == 60, "the table was reconstructed from the ring: no key of the evicted cloud is left"
    fn, fgot = _fresh_map(cl, ("a", "b"), mode)
    assert fn == n and np.array_equal(fgot, got)
    ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_table_overflow_is_refused_and_is_not_permanent(small, mode):
    from glio_amd import capi
    cl, refs = small
    ctx = _context(lc.SMALL_WIDTH, lc.SMALL_CAP, lc.SMALL_MAX_MAP, mode)
    worst = Worst()
    ctx.localmap_push(cl["big200"], *lc.IDENT)                   # 200 voxels into 128 slots
    with pytest.raises(capi.GlioError) as e:
        ctx.localmap_build()
    assert "error -1" in str(e.value) and "voxel table overflow" in str(e.value)
    ctx.localmap_push(cl["a"], *lc.IDENT)                        # still in the ring: the reconstructed table overflows again
    with pytest.raises(capi.GlioError) as e:
        ctx.localmap_build()
    assert "voxel table overflow" in str(e.value)
    n, got = _push_build(ctx, cl["b"])                           # evicts the offending keyframe (its removal meets keys that were never inserted)
    _compare(n, got, refs[("a", "b")], mode, worst, "after the overflow")
    st = ctx.localmap_stats()
    assert st[1] == n == 60 and st[6] >= 1, st
    fn, fgot = _fresh_map(cl, ("a", "b"), mode)
    assert fn == n and np.array_equal(fgot, got), "byte for byte what a context that never overflowed holds"
    n, got = _push_build(ctx, cl["c"])                           # nothing later is affected: plain insert / evict again
    _compare(n, got, refs[("b", "c")], mode, worst, "one keyframe later")
    fn, fgot = _fresh_map(cl, ("b", "c"), mode)
    assert fn == n == 50 and np.array_equal(fgot, got)
    _report("table overflow", mode, worst, ctx.localmap_stats())
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the bitmap's limit
@pytest.fixture(scope="module")
def boxes(po):
    base, cases = lc.box_cases()
    seq = [("base", base, 1)] + cases + [("base again", base, 1)]
    return seq, [Ref(po, cl) for _, cl, _ in seq]


@pytest.mark.parametrize("mode", MODES)
def test_bounding_boxes_of_exactly_2_27_cells_and_one_slice_more(boxes, mode):
    """base cloud, 2^27 cells with the last index occupied, 2^27 cells, one slice more with an index outside the bitmap, one slice more with every index
    inside it (bits set that only the radix path's emit can clear), base cloud: by the bitmap's rank where it applies, and all by the radix sort"""
    seq, refs = boxes
    results = []
    for force in (False, True):
        ctx = _context(1, lc.BOX_CAP, lc.BOX_MAX_MAP, mode, force_sort=force)
        worst = Worst()
        maps, paths = [], []
        for (name, cloud, path), ref in zip(seq, refs):
            n, got = _push_build(ctx, cloud)
            _compare(n, got, ref, mode, worst, f"{name} (sort forced: {force})")
            st = ctx.localmap_stats()
            paths.append(st[3])
            if st[3] == 2:
                assert st[4] == lc.radix_passes(cloud, lc.LEAF), f"{name}: {st}"
            maps.append(got)
        _report(f"bitmap limit (sort forced: {force})", mode, worst, ctx.localmap_stats())
        assert paths == ([2] * len(seq) if force else [p for _, _, p in seq]), paths
        assert np.array_equal(maps[0], maps[-1]), "no bit was left behind"
        assert ctx.localmap_stats()[6] == 0
        results.append(maps)
        ctx.close()
    for a, b in zip(*results):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. more than 256 tiles
@pytest.fixture(scope="module")
def large(po):
    frames = lc.large_map_case()
    cloud = np.vstack(frames)
    return frames, Ref(po, cloud), lc.radix_passes(cloud, lc.LEAF)


@pytest.mark.parametrize("mode", MODES)
def test_a_map_of_more_than_256_sort_tiles(large, mode):
    frames, ref, passes = large
    assert -(-len(ref.oracle) // lc.RS_TILE) > lc.RS_SCAN_TILES
    maps = []
    for force in (False, True):
        ctx = _context(lc.LARGE_WIDTH, lc.LARGE_CAP, lc.LARGE_MAX_MAP, mode, force_sort=force, scan_pts=1024)
        for f in frames:
            ctx.localmap_push(f, *lc.IDENT)
        n = ctx.localmap_build()
        got = ctx.localmap_read().copy()
        worst = Worst()
        _compare(n, got, ref, mode, worst, f"sort forced: {force}")
        st = ctx.localmap_stats()
        _report(f"more than 256 tiles (sort forced: {force})", mode, worst, st)
        assert st[3:6] == ([2, passes, n] if force else [1, 0, n]), st
        maps.append(got)
        ctx.close()
    assert np.array_equal(maps[0], maps[1])


# ------------------------------------------------------------------------------------------------ 7. a dense voxel
@pytest.fixture(scope="module")
def dense(po):
    frames, once = lc.dense_voxel_case()
    return frames, once, Ref(po, np.vstack(frames)), Ref(po, np.vstack([once] * lc.DENSE_WIDTH))


@pytest.mark.parametrize("mode", MODES)
def test_a_voxel_that_holds_thousands_of_points(dense, mode):
    """mode 1 is the point: the voxel's list of 3000 (12 000) entries, filled in atomic order by every keyframe of the ring, is sorted inside one thread"""
    frames, once, ref_frames, ref_once = dense
    worst = Worst()
    for name, pushes, ref in (("four keyframes", frames, ref_frames), ("one cloud four times", [once] * lc.DENSE_WIDTH, ref_once)):
        ctx = _context(lc.DENSE_WIDTH, lc.DENSE_CAP, lc.DENSE_MAX_MAP, mode)
        for f in pushes:
            ctx.localmap_push(f, *lc.IDENT)
        n = ctx.localmap_build()
        _compare(n, ctx.localmap_read().copy(), ref, mode, worst, name)
        _report(f"dense voxel ({name})", mode, worst, ctx.localmap_stats())
        ctx.close()

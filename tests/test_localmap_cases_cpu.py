"""The cases of tests/localmap_cases.py take the branches they are about, shown with the oracle alone (CPU only), and the float64 reference
agrees with the oracle's voxel grid.  The numbers asserted here are the conditions under which tests/test_hip_localmap_limits.py means
anything: at least 3 table rebuilds in the drive, exactly 2^27 cells, more than 256 sort tiles, ..."""
import numpy as np
import pytest

import localmap_cases as lc


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def _dims(po, cloud):
    """(cells of the bounding box, largest linear index, voxels) by the oracle; the geometry restated in numpy must agree"""
    ref, idx = po.voxel_grid(cloud, lc.LEAF)
    _, div_b = lc.grid_geometry(cloud, lc.LEAF)
    assert int(idx.max()) < int(np.prod(div_b))
    return tuple(int(d) for d in div_b), int(idx.max()), len(ref)


# ------------------------------------------------------------------------------------------------ the reference
def test_exact_centroids_is_the_oracles_voxel_grid_in_float64(po):
    """same voxels, same linear indices, same order; centroids within the float accumulation's error of the oracle's: n points summed in float lose at
    most (n - 1) ulp/2 of the largest partial sum, the division and the inputs' magnitude bound it by n * 2^-24 * max|p| per component"""
    base, cases = lc.box_cases()
    frames, once = lc.dense_voxel_case()
    for cloud in [base, once, np.vstack(frames)] + [c for _, c, _ in cases]:
        ref, idx = po.voxel_grid(cloud, lc.LEAF)
        cen, idx64 = lc.exact_centroids(cloud, lc.LEAF)
        assert np.array_equal(idx, idx64)
        _, counts = np.unique(lc.voxel_keys(cloud, lc.LEAF), return_counts=True)
        bound = (counts.max() + 1) * 2.0 ** -24 * np.abs(cloud).max()
        assert np.abs(cen - ref).max() <= bound
    # one point per voxel: the centroid IS the point
    one = lc.lattice_points(np.array([[0, 0, 0], [5, -3, 2], [-7, 1, 1]]), np.random.default_rng(1))
    cen, idx = lc.exact_centroids(one, lc.LEAF)
    ref, ridx = po.voxel_grid(one, lc.LEAF)
    assert np.array_equal(cen.astype(np.float32), ref) and np.array_equal(idx, ridx)
    assert lc.exact_centroids(np.zeros((0, 4), np.float32), lc.LEAF)[0].shape == (0, 4)


def test_simulate_table_on_a_hand_made_sequence():
    # max_map_points 4 -> 8 slots, rebuild when the previous build saw more than 4 keys; width 2
    sets = [{1, 2, 3}, {4, 5}, {6}, {7}, {8}]
    sim = lc.simulate_table(sets, 2, 4)
    assert sim["table_cap"] == 8
    assert sim["keys"] == [3, 5, 3, 4, 5]           # build 2: previous saw 5 > 4 -> only the ring {4,5,6} stays
    assert sim["rebuilds"] == [2] and sim["peak"] == 6 and sim["live"] == [3, 5, 3, 2, 2]


# ------------------------------------------------------------------------------------------------ each case takes its branch
def test_drive_case_rebuilds_the_table_again_and_again(po):
    _, clouds, poses = lc.drive_case()
    assert len(clouds) == lc.DRIVE_W and max(len(c) for c in clouds) <= lc.DRIVE_CAP
    glob = [po.transform_cloud(c, q, t) for c, (q, t) in zip(clouds, poses)]
    sets = [set(lc.voxel_keys(g, lc.LEAF).tolist()) for g in glob]
    sim = lc.simulate_table(sets, lc.DRIVE_WIDTH, lc.DRIVE_MAX_MAP)
    print("drive: rebuilds at", sim["rebuilds"], "peak", sim["peak"], "of", sim["table_cap"], "max live", max(sim["live"]))
    assert len(sim["rebuilds"]) >= 3
    assert sim["peak"] < sim["table_cap"], "the table never overflows"
    assert max(sim["live"]) <= lc.DRIVE_MAX_MAP
    # the live count is the oracle's voxel count of the ring
    for b in (0, 5, lc.DRIVE_W - 1):
        lo = max(0, b + 1 - lc.DRIVE_WIDTH)
        ref, _ = po.voxel_grid(np.vstack(glob[lo:b + 1]), lc.LEAF)
        assert len(ref) == sim["live"][b]


def test_small_table_clouds(po):
    cl = lc.small_table_clouds()
    cap = lc.table_cap(lc.SMALL_MAX_MAP)
    assert cap == 128

    def nvox(*names):
        return len(po.voxel_grid(np.vstack([cl[n] for n in names]), lc.LEAF)[0])
    assert nvox("big100") == 100 and lc.SMALL_MAX_MAP < 100 < cap                 # refused by the voxel count, the table holds it
    assert nvox("big200") == 200 > cap                                            # the table cannot hold it
    assert nvox("a") == nvox("b") == nvox("c") == 40
    assert nvox("big100", "a") == 100 and nvox("big200", "a") == 200              # still refused while the large cloud is in the ring
    assert nvox("a", "b") == 60 <= lc.SMALL_MAX_MAP and nvox("b", "c") == 50
    assert max(len(c) for c in cl.values()) <= lc.SMALL_CAP


def test_box_cases_sit_at_the_bitmap_limit(po):
    base, cases = lc.box_cases()
    assert 1900 <= len(base) <= 2100 and np.abs(base[:, :3]).max() <= 24.0
    assert max(_dims(po, base)[0]) <= 120
    got = {name: _dims(po, cloud) for name, cloud, _ in cases}
    path = {name: p for name, _, p in cases}
    assert [n for n, _, _ in cases] == ["exact_corner", "exact_faces", "over_corner", "over_span_only"]
    assert got["exact_corner"][0] == (512, 512, 512) and 512 ** 3 == lc.BM_MAX_BITS and got["exact_corner"][1] == lc.BM_MAX_BITS - 1
    assert got["exact_faces"][0] == (512, 512, 512) and got["exact_faces"][1] == 511 * 512 * 512
    assert got["over_corner"][0] == (513, 512, 512) and got["over_corner"][1] >= lc.BM_MAX_BITS
    assert got["over_span_only"][0] == (513, 512, 512) and got["over_span_only"][1] == 134217216 < lc.BM_MAX_BITS
    assert path == dict(exact_corner=1, exact_faces=1, over_corner=2, over_span_only=2)
    for name, cloud, _ in cases:
        assert got[name][2] <= lc.BOX_MAX_MAP and len(cloud) <= lc.BOX_CAP
        assert lc.radix_passes(cloud, lc.LEAF) == 4                               # 2^27 and 513 * 2^18 cells: 27 and 28 bits


def test_large_map_case_needs_more_than_256_tiles(po):
    frames = lc.large_map_case()
    assert len(frames) == lc.LARGE_WIDTH and all(len(f) == lc.LARGE_CAP for f in frames)
    cloud = np.vstack(frames)
    div, top, nv = _dims(po, cloud)
    assert div == lc.LARGE_DIMS and nv == int(np.prod(lc.LARGE_DIMS)) > 262144
    assert -(-nv // lc.RS_TILE) > lc.RS_SCAN_TILES
    assert nv <= lc.LARGE_MAX_MAP and int(np.prod(div)) <= lc.BM_MAX_BITS         # the bitmap takes it unless the sort is forced
    assert lc.radix_passes(cloud, lc.LEAF) == 3
    assert all(len(set(lc.voxel_keys(f, lc.LEAF).tolist())) > 50000 for f in frames)


def test_dense_voxel_case(po):
    frames, once = lc.dense_voxel_case()
    assert len(frames) == lc.DENSE_WIDTH and max(len(f) for f in frames) <= lc.DENSE_CAP and len(once) <= lc.DENSE_CAP
    key = lc.voxel_keys(lc.lattice_points(np.array([lc.DENSE_VOXEL]), np.random.default_rng(0)), lc.LEAF)[0]
    per_frame = [int((lc.voxel_keys(f, lc.LEAF) == key).sum()) for f in frames]
    assert per_frame == [750] * 4 and int((lc.voxel_keys(once, lc.LEAF) == key).sum()) == lc.DENSE_POINTS
    nv = len(po.voxel_grid(np.vstack(frames), lc.LEAF)[0])
    assert 450 <= nv <= 560 and nv <= lc.DENSE_MAX_MAP
    assert len(po.voxel_grid(np.vstack([once] * 4), lc.LEAF)[0]) == nv
    _, counts = np.unique(lc.voxel_keys(np.vstack(frames), lc.LEAF), return_counts=True)
    assert np.sort(counts)[-2] < 64, "every other voxel is an ordinary one"

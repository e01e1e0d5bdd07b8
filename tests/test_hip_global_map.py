"""GPU: glio_gmap_* -- the global map built on the device from the keyframe clouds a batch association holds (mapVisualizationThread's save_pcd part and
publishCompleteMap, reference GLIO/src/Estimator.cpp:5315-5350, :5275-5313): transformCloud at caller-supplied poses, the concatenation through one pcl::VoxelGrid.
The map must equal the oracle's restatement (transform_cloud + voxel_grid) bit for bit, appends must equal a rebuild bit for bit, and a refusal must leave the map
exactly as it was.  Every comparison of device output is np.array_equal.  The cases are tests/global_map_restated.py's; tests/test_global_map_cpu.py shows with the
oracle alone that they are what they claim to be."""
import re

import numpy as np
import pytest

import global_map_restated as gr
from glio_amd import batch, loop, mapping, capi

pytestmark = pytest.mark.gpu

K = gr.K
NEVER_SET, EMPTY = K, K + 1
F4, F4M = [2, 3, 4, 5], [5, 2, 4, 3]


@pytest.fixture(scope="module")
def rig():
    """the window case in a batch association of K + 2 frames (frame K is never set, frame K + 1 is set to an empty cloud)"""
    clouds, old, new = gr.window_case()
    ba = batch.BatchAssociation(K + 2, gr.CAP, 400000)
    for s in range(K):
        ba.set_frame(s, clouds[s])
    ba.set_frame(EMPTY, np.zeros((0, 4), np.float32))
    yield dict(clouds=clouds, old=old, new=new, ba=ba)
    ba.close()


@pytest.fixture(scope="module")
def oracle(rig):
    """every reference map the tests below compare against, computed once"""
    from oracle import pyoracle as po

    def vg(frames, poses, leaf):
        return po.voxel_grid(np.vstack([po.transform_cloud(rig["clouds"][f], p[3:], p[:3]) for f, p in zip(frames, poses)]), leaf)[0]
    out = {}
    for leaf in (0.2, 0.4):
        out["asc", leaf] = vg(F4, rig["new"][F4], leaf)
        out["mixed", leaf] = vg(F4M, rig["new"][F4M], leaf)
    out["stale"] = vg(F4, rig["old"][F4], 0.2)
    frames, poses = gr.ring_case()
    out["ring"] = vg(frames, poses, 0.2)
    return out


def _rc(exc):
    return int(re.search(r"error (-?\d+)", str(exc.value)).group(1))


def _same(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_map_equals_the_oracle_bit_for_bit(rig, oracle, leaf):
    gm = mapping.GlobalMap(rig["ba"], mapping.default_opts(leaf=leaf, max_voxels=1 << 16, max_points_per_add=1 << 15))
    for name, frames in (("asc", F4), ("mixed", F4M)):                   # (the frames overlap: the order changes the float sums)
        gm.clear()
        info = gm.add(frames, rig["new"][frames])
        got, want = gm.read(), oracle[name, leaf]
        print(name, leaf, info.as_dict(), len(want))
        assert info.n_voxels == gm.size() == len(want) and info.n_points_total == sum(len(rig["clouds"][f]) for f in frames)
        assert not info.pcl_index_overflow and 1 <= info.radix_passes <= 4
        assert _same(got, want), (name, leaf)
    assert not np.array_equal(oracle["asc", leaf], oracle["mixed", leaf])
    gm.close()


def test_a_map_at_the_old_poses_is_another_map(rig, oracle):
    gm = mapping.GlobalMap(rig["ba"], mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 15))
    gm.add(F4, rig["old"][F4])
    assert _same(gm.read(), oracle["stale"])
    gm.clear(); gm.add(F4, rig["new"][F4])
    got = gm.read()
    assert _same(got, oracle["asc", 0.2]) and not _same(got, oracle["stale"])          # (a map left at the old poses would not pass)
    gm.close()


def test_appends_equal_a_rebuild(rig, oracle):
    opts = mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 15)
    gm = mapping.GlobalMap(rig["ba"], opts)
    new = rig["new"]
    sizes = []
    for part in ([2, 3], [4], [5]):
        sizes.append(gm.add(part, new[part]).n_voxels)
    three = gm.read()
    assert sizes[0] < sizes[-1] and _same(three, oracle["asc", 0.2])
    assert _same(gm.read(100, 50), three[100:150])                      # (ranges)
    gm.clear()
    assert gm.size() == 0 and len(gm.read()) == 0
    gm.add(F4, new[F4])
    assert _same(gm.read(), three)                                      # cleared and rebuilt: the same bytes
    other = mapping.GlobalMap(rig["ba"], opts)
    other.add(F4, new[F4])
    assert _same(other.read(), three)                                   # two builds: identical bytes
    # the other order, split the other way
    gm.clear(); gm.add([5], new[[5]]); gm.add([2, 4], new[[2, 4]]); gm.add([3], new[[3]])
    assert _same(gm.read(), oracle["mixed", 0.2])
    other.close(); gm.close()


@pytest.mark.parametrize("leaf", [0.2, 0.4])
def test_map_equals_the_submap_route(rig, leaf):
    """glio_loop_build_submap on the same frames, poses and leaf: the only route to a map before glio_gmap"""
    lp = loop.LoopClosure(rig["ba"], loop.default_opts(leaf=leaf))
    gm = mapping.GlobalMap(rig["ba"], mapping.default_opts(leaf=leaf, max_voxels=1 << 16, max_points_per_add=1 << 15))
    for frames in (F4, F4M, [2]):
        n = lp.build_submap(loop.TARGET, frames, rig["new"][frames])
        gm.clear()
        info = gm.add(frames, rig["new"][frames])
        assert info.n_voxels == n and _same(gm.read(), lp.read_submap(loop.TARGET))
    gm.close(); lp.close()


def test_many_frames_past_every_constant_of_the_sort(rig, oracle):
    c = gr.sort_constants()
    frames, poses = gr.ring_case()
    n = sum(len(rig["clouds"][f]) for f in frames)
    limits = {"pairs of one wavefront of k_gm_hist / k_gm_scatter (GM_SORT_TILE)": c["GM_SORT_TILE"],
              "pairs of one workgroup of k_gm_scan_a / _c (GM_SCAN_CHUNK tiles)": c["GM_SCAN_CHUNK"] * c["GM_SORT_TILE"],
              "points of one workgroup of k_gm_runs (GM_RUN_BLOCK)": c["GM_RUN_BLOCK"],
              "points k_gm_runs_top covers with one block total per thread (GM_TOP_THREADS x GM_RUN_BLOCK)": c["GM_TOP_THREADS"] * c["GM_RUN_BLOCK"],
              "points of one workgroup of k_gm_transform (GM_TF_THREADS x GM_TF_PER)": c["GM_TF_THREADS"] * c["GM_TF_PER"]}
    for what, lim in limits.items():
        assert n >= 2 * lim and n % lim != 0, (what, lim, n)            # at least twice over, with a ragged tail
    assert len(frames) == 80 > loop.default_opts().max_frames_per_submap and len(set(frames)) < len(frames)
    gm = mapping.GlobalMap(rig["ba"], mapping.default_opts(max_voxels=1 << 19, max_points_per_add=1 << 19))
    info = gm.add(frames, poses)
    print(info.as_dict(), n, gm.last_device_ms(), gm.last_stage_ms())
    assert info.n_points_total == n and info.n_voxels == len(oracle["ring"])
    assert _same(gm.read(), oracle["ring"])
    # ... and the same 80 frames in five calls of 16: every call merges into a map that already holds most of its voxels
    gm.clear()
    for a in range(0, 80, 16):
        gm.add(frames[a:a + 16], poses[a:a + 16])
    assert _same(gm.read(), oracle["ring"])
    gm.close()


@pytest.fixture(scope="module")
def extents():
    """frame 0: the faces cloud; 1-3: the far case; 4: the one-voxel cloud"""
    from oracle import pyoracle as po
    faces = gr.faces_cloud()
    fc, fp = gr.far_case()
    one, one_pose = gr.one_voxel_case()
    clouds = [faces] + fc + [one]
    ba = batch.BatchAssociation(len(clouds), 18432, 16)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    want = {("faces", leaf): po.voxel_grid(po.transform_cloud(faces, gr.IDENTITY[3:], gr.IDENTITY[:3]), leaf)[0] for leaf in (0.2, 0.4)}
    want["far"] = po.voxel_grid(np.vstack([po.transform_cloud(c, p[3:], p[:3]) for c, p in zip(fc, fp)]), 0.2)[0]
    want["one"] = po.voxel_grid(po.transform_cloud(one, one_pose[3:], one_pose[:3]), 0.2)[0]
    yield dict(ba=ba, want=want, far_poses=fp, one_pose=one_pose)
    ba.close()


def test_extents(extents):
    ba, want = extents["ba"], extents["want"]
    passes_near = None
    for leaf in (0.2, 0.4):                                             # negative coordinates, points exactly on voxel faces
        gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=leaf, max_voxels=1 << 16, max_points_per_add=1 << 15))
        info = gm.add([0], gr.IDENTITY[None, :])
        assert not info.pcl_index_overflow and _same(gm.read(), want["faces", leaf])
        passes_near = info.radix_passes
        gm.close()
    gm = mapping.GlobalMap(ba, mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 15))
    info = gm.add([1, 2, 3], extents["far_poses"])                      # 3 km apart: PCL's int index would overflow, the 64-bit one does not
    print("far", info.as_dict(), len(want["far"]))
    assert info.pcl_index_overflow and info.radix_passes > passes_near and info.radix_passes > 4
    assert info.n_points_total == 6000 and _same(gm.read(), want["far"])
    gm.clear()
    near = gm.add([1, 2], extents["far_poses"][:2])
    assert not near.pcl_index_overflow
    far = gm.add([3], extents["far_poses"][2:])                         # the flag is about everything added since the clear
    assert far.pcl_index_overflow and _same(gm.read(), want["far"])
    gm.clear()
    info = gm.add([4], extents["one_pose"][None, :])                    # 5000 points, one voxel: a run longer than any tile, no digit varies
    assert len(want["one"]) == 1 and info.n_voxels == 1 and info.radix_passes == 0 and _same(gm.read(), want["one"])
    again = gm.add([4], extents["one_pose"][None, :])                   # ... and 5000 more continue its sum
    assert again.n_voxels == 1 and again.n_points_total == 10000
    gm.close()


def test_refusals_leave_the_map_as_it_was(rig):
    new = rig["new"]
    gm = mapping.GlobalMap(rig["ba"], mapping.default_opts(max_voxels=1 << 16, max_points_per_add=12000))
    gm.add([2, 4], new[[2, 4]])
    before, size, dev = gm.read(), gm.size(), gm.points_dev()
    bad_pose = {"nan": new[[2]].copy(), "inf": new[[2]].copy(), "far": new[[2]].copy()}
    bad_pose["nan"][0, 4] = np.nan; bad_pose["inf"][0, 0] = np.inf
    bad_pose["far"][0, 0] = 3e5                                         # 3e5 m / 0.2 m = 1.5e6 > 2^20: the key's range
    cases = [("no frames", [], np.zeros((0, 7))), ("index above", [K + 2], new[[2]]), ("index below", [-1], new[[2]]), ("never set", [NEVER_SET], new[[2]]),
             ("empty", [EMPTY], new[[2]]), ("valid then never set", [2, NEVER_SET], new[[2, 2]]), ("nan pose", [2], bad_pose["nan"]), ("inf pose", [2], bad_pose["inf"]),
             ("too many points", [2, 6, 7], new[[2, 6, 7]]), ("coordinate limit", [2], bad_pose["far"]), ("coordinate limit behind a good frame", [6, 2], np.vstack([new[[6]], bad_pose["far"]]))]
    for what, frames, poses in cases:
        with pytest.raises(capi.GlioError) as e:
            gm.add(frames, poses)
        assert _rc(e) == -1, what
        assert gm.size() == size and gm.points_dev() == dev and _same(gm.read(), before), what
    gm.close()
    # more voxels than max_voxels: the first add fits, the second does not
    small = mapping.GlobalMap(rig["ba"], mapping.default_opts(max_voxels=4000, max_points_per_add=1 << 15))
    n1 = small.add([5], new[[5]]).n_voxels
    assert 0 < n1 <= 4000
    before, dev = small.read(), small.points_dev()
    with pytest.raises(capi.GlioError) as e:
        small.add([2, 6], new[[2, 6]])
    assert _rc(e) == -1 and small.size() == n1 and small.points_dev() == dev and _same(small.read(), before)
    small.add([3], new[[3]])                                            # (and the object goes on)
    assert small.size() in (n1, n1 + 1)
    small.close()


def test_add_beside_an_association_in_flight(rig, oracle):
    """an add issued while a glio_bassoc_run_append_async is on the association's stream: the same bytes as alone, the association's records unchanged"""
    ba, new = rig["ba"], rig["new"]
    poses_all = np.zeros((K + 2, 7)); poses_all[:, 3] = 1.0
    poses_all[:K] = new
    ci, cj = batch.pair_list(3, 1)
    ba.reset()
    cnt0, tot0 = ba.run_append(poses_all, ci, cj)
    rec0 = [a.copy() for a in ba.read()]
    gm = mapping.GlobalMap(ba, mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 15))
    ba.reset()
    ba.run_append(poses_all, ci, cj, wait=False)
    gm.add(F4, new[F4])
    cnt1, tot1 = ba.finish()
    rec1 = ba.read()
    assert _same(gm.read(), oracle["asc", 0.2])
    assert tot0 == tot1 and tot0 > 0 and np.array_equal(cnt0, cnt1) and all(np.array_equal(a, b) for a, b in zip(rec0, rec1))
    ba.reset()
    gm.close()


def test_host_demo_map_equals_the_python_driver(rig, tmp_path):
    from glio_amd.host import window_io
    q_bl, t_bl = np.array([0.9998, 0.01, -0.012, 0.008]), np.array([0.05, -0.02, 0.1])
    q_bl = q_bl / np.linalg.norm(q_bl)
    info = np.c_[rig["new"][:, :3], rig["new"][:, 3:]]
    opts = mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 15)
    path = str(tmp_path / "map_case.bin")
    window_io.write_map_case(path, opts, gr.CAP, rig["clouds"], info, q_bl, t_bl, 3, 2)
    got = window_io.run_demo_map(path)
    frames = mapping.global_map_frames(K, 3)
    assert frames == [0, 3, 6] and got["n_frames"] == 3
    gm = mapping.GlobalMap(rig["ba"], opts)
    for a in range(0, len(frames), 2):
        last = gm.add(frames[a:a + 2], loop.frame_poses(info[frames[a:a + 2]], q_bl, t_bl))
    assert (got["n_voxels"], got["n_points_total"], got["radix_passes"], got["pcl_index_overflow"]) == (last.n_voxels, last.n_points_total, last.radix_passes, last.pcl_index_overflow)
    assert got["checksum"] == window_io.loop_checksum(gm.read())
    gm.close()

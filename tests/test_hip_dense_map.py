"""GPU: the dense store (glio_dense_*, include/glio_dense.h) and the global map over it (glio_gmap_create_on_dense).  A frame is
keyframe_cloud_restated.keyframe_cloud(pts, leaf, trans, quat) -- and what glio_set_scan_filtered + glio_get_scan give on a window context, which ties the
wavefront-per-long-list emit to the existing chain; the map is global_map_restated.restated_voxel_grid of the moved frames.  Every comparison is on bytes."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_map_restated as dr  # noqa: E402
import global_map_restated as gr  # noqa: E402
import keyframe_cloud_restated as kr  # noqa: E402

from glio_amd import batch, capi, features, mapping, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

pytestmark = pytest.mark.gpu

LEAF = dr.LEAF
TRANS = (0.6, -0.05, 0.02)
QUAT = (math.cos(0.015), 0.0, 0.0, math.sin(0.015))            # yaw 0.03 rad over the sweep
Q0 = np.array([1.0, 0.0, 0.0, 0.0])
MOTIONS = [(None, None), (TRANS, None), (TRANS, QUAT)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cloud(n, seed, span=6.0):
    """points on both sides of zero on every axis, ~ 15 per 0.4 m voxel at n = 4097 near the middle: lists of many lengths"""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, span / 3, (n, 3)).clip(-span, span)
    inten = rng.integers(0, 16, n) + rng.uniform(0.0, 0.11, n)
    return np.ascontiguousarray(np.concatenate([xyz, inten[:, None]], 1).astype(np.float32))


@pytest.fixture(scope="module")
def store():
    d = mapping.DenseClouds(6, 1 << 14, 20480)
    yield d
    d.close()


@pytest.fixture(scope="module")
def window():
    ctx = capi.Context(synth.default_opts(1, pts=1 << 13, map_pts=1 << 14))
    ctx.scan_filter_config(1 << 13)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_host_source(store, window, n):
    p = _cloud(n, 300 + n, span=1.5 if n <= 65 else 6.0)
    rec = capi.to_pcl_xyzi(p)
    for trans, quat in MOTIONS:
        want = kr.keyframe_cloud(p, LEAF, trans, quat)
        assert store.set_frame(1, p, LEAF, trans, quat) == len(want) == store.frame_count(1)
        got = store.read_frame(1)
        print(f"n {n} motion {trans is not None}/{quat is not None}: {len(got)} voxels, words that differ from the restatement "
              f"{int((_bits(got) != _bits(want)).sum()) if got.shape == want.shape else -1}")
        assert _same(got, want), (n, trans, quat)
        # the existing chain: the same cloud through the keyframe cloud stage of a window context
        assert window.set_scan_filtered(0, p, LEAF, trans, quat) == len(want)
        assert _same(got, window.get_scan(0)), (n, trans, quat)
        # 32-byte records: the same bytes
        assert store.set_frame(2, rec, LEAF, trans, quat, ioff=capi.PCL_XYZI_INTENSITY_OFFSET) == len(want)
        assert _same(store.read_frame(2), got)
    if n >= 1023:
        assert len(want) < n                                         # (it filtered)


def test_long_lists(store, window):
    """voxels whose lists hold 1 .. 4097 points and every threshold of the emit at -1, +0, +1, no list contiguous in the input"""
    pts, sizes, _ = dr.long_list_cloud()
    k = dr.wave_constants()
    assert max(sizes) > k["LM_WAVE_LIST_LDS"] and min(sizes) <= k["LM_WAVE_LIST_MIN"] and len(pts) <= store.max_in
    want = kr.keyframe_cloud(pts, LEAF)
    assert len(want) == len(sizes)
    assert store.set_frame(0, pts, LEAF) == len(want)
    got = store.read_frame(0)
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(axis=1)) if got.shape == want.shape else None
    print("long lists: voxels that differ", bad)
    assert _same(got, want)
    # and one list alone, on either side of every path
    for n in (k["LM_WAVE_LIST_MIN"], k["LM_WAVE_LIST_MIN"] + 1, 64, 65, k["LM_WAVE_LIST_LDS"], k["LM_WAVE_LIST_LDS"] + 1, 4097):
        one = dr.one_voxel_cloud(n)
        w1 = kr.keyframe_cloud(one, LEAF)
        assert len(w1) == 1 and store.set_frame(0, one, LEAF) == 1 and _same(store.read_frame(0), w1), n
    # the existing emit gives the same bytes for the mixed cloud (max_input_points of the window's stage: 8192 -> the first 8192 points)
    part = pts[:1 << 13]
    assert store.set_frame(0, part, LEAF) == window.set_scan_filtered(0, part, LEAF)
    assert _same(store.read_frame(0), window.get_scan(0))


def test_overflow_rule_and_copy(store):
    p = _cloud(100, 9, span=1.0)
    two = np.array([[-5000.0, -5000.0, -5000.0, 3.05], [5000.0, 5000.0, 5000.0, 7.02]], np.float32)
    for cloud in (two, np.vstack([p[:50], two[:1], p[50:], two[1:]])):
        for trans in (None, TRANS):
            want = kr.keyframe_cloud(cloud, LEAF, trans)
            assert _same(want, kr.keyframe_cloud(cloud, 0.0, trans))                  # (25 000^3 cells: the restatement passes the de-skewed cloud through)
            assert store.set_frame(3, cloud, LEAF, trans) == len(cloud) and _same(store.read_frame(3), want)
    # the next call filters again
    want = kr.keyframe_cloud(p, LEAF)
    assert store.set_frame(3, p, LEAF) == len(want) < 100 and _same(store.read_frame(3), want)
    # leaf <= 0: a copy (of the de-skewed cloud)
    for leaf in (0.0, -1.0):
        for trans in (None, TRANS):
            assert store.set_frame(3, p, leaf, trans) == 100 and _same(store.read_frame(3), kr.keyframe_cloud(p, 0.0, trans))


def test_refusals_leave_the_frame():
    d = mapping.DenseClouds(2, 1024, 4096)
    p = _cloud(300, 21)
    keep = kr.keyframe_cloud(p, LEAF)
    assert d.set_frame(0, p, LEAF) == len(keep)
    other = capi.Context(synth.default_opts(1, pts=1 << 10, map_pts=1 << 10))
    calls = [lambda: d.set_frame(-1, p, LEAF), lambda: d.set_frame(2, p, LEAF),                                   # k outside [0, K)
             lambda: d.set_frame(0, np.zeros((10, 3), np.float32), LEAF, ioff=8),                                   # 12-byte records
             lambda: d.set_frame(0, _cloud(4097, 22), LEAF),                                                        # n > max_input_points
             lambda: d.set_frame(0, p[:10], LEAF, (0.1, float("nan"), 0.0)),
             lambda: d.set_frame(0, p[:10], LEAF, TRANS, (1.0, 0.0, float("inf"), 0.0))]
    for i, call in enumerate(calls):
        with pytest.raises(capi.GlioError) as e:
            call()
        assert e.value.code == capi.E_ARG, i
        assert d.frame_count(0) == len(keep) and _same(d.read_frame(0), keep), i
    with pytest.raises(capi.GlioError) as e:
        d.set_frame_from_features(0, other, LEAF)                      # a front end without an extraction
    assert e.value.code == capi.E_STATE and _same(d.read_frame(0), keep)
    # more outputs than max_points_per_frame: one point per voxel, 1025 of them -- n_out tells the count
    g = np.array([[0.2 + 0.4 * (i % 33), 0.2 + 0.4 * (i // 33), 0.2, float(i % 16)] for i in range(1025)], np.float32)
    g = g[np.random.default_rng(6).permutation(1025)]
    for leaf in (LEAF, 0.0):
        with pytest.raises(capi.GlioError) as e:
            d.set_frame(0, g, leaf)
        assert e.value.code == capi.E_ARG and e.value.n_out == 1025
        assert d.frame_count(0) == len(keep) and _same(d.read_frame(0), keep)
    assert d.frame_count(1) == 0 and len(d.read_frame(1)) == 0         # the other frame was never touched
    assert d.set_frame(0, g[:1024], LEAF) == 1024 and _same(d.read_frame(0), kr.keyframe_cloud(g[:1024], LEAF))      # exactly full, and the stage still works
    other.close(); d.close()


def _frontend(n_scans=16):
    fe = capi.Context(synth.default_opts(1, pts=1 << 14, map_pts=1 << 14))
    fe.features_config(features.default_opts(n_scans, max_raw_points=1 << 15))
    return fe


@pytest.fixture(scope="module")
def drive():
    return sl.drive(n_frames=2, n_scans=16, n_az=900)


@pytest.mark.parametrize("trans", [None, TRANS])
def test_resident_source_equals_host_source(store, drive, trans):
    fe = _frontend()
    fe.features_extract(drive[0], Q0)
    cut = fe.features_read(T.FEAT_CUT_CLOUD)
    assert 5000 < len(cut) <= store.max_in
    want = kr.keyframe_cloud(cut, LEAF, trans)
    assert store.set_frame_from_features(4, fe, LEAF, trans) == len(want)
    assert store.set_frame(5, cut, LEAF, trans) == len(want)
    a, b = store.read_frame(4), store.read_frame(5)
    assert _same(a, b) and _same(a, want)
    assert _same(fe.features_read(T.FEAT_CUT_CLOUD), cut)              # the de-skew is out of place
    fe.close()


@pytest.mark.parametrize("leaf", [LEAF, 0.0])
def test_two_readers_are_ordered_before_the_next_extraction(store, drive, leaf):
    """the window reads the surf features on its upload stream, the store the cut cloud on its own, and the front end extracts the NEXT scan at once: both
    hold the FIRST scan's cloud (leaf 0: the store's call does not wait for the host at all)"""
    fe = _frontend()
    win = capi.Context(synth.default_opts(2, pts=1 << 13, map_pts=1 << 14))
    win.scan_filter_config(1 << 13)
    fe.features_extract(drive[0], Q0)
    surf0, cut0 = fe.features_read(T.FEAT_SURF), fe.features_read(T.FEAT_CUT_CLOUD)
    want_w, want_d = kr.keyframe_cloud(surf0, 0.9, TRANS), kr.keyframe_cloud(cut0, leaf, TRANS)
    nw = win.set_scan_from_features(fe, 0, 0.9, TRANS, ahead=True)
    nd = store.set_frame_from_features(4, fe, leaf, TRANS)
    fe.features_extract(drive[1], Q0)
    win.slide_window()
    assert nw == len(want_w) and nd == len(want_d)
    assert _same(win.get_scan(1), want_w)
    assert _same(store.read_frame(4), want_d)
    assert not _same(fe.features_read(T.FEAT_CUT_CLOUD), cut0) and not _same(fe.features_read(T.FEAT_SURF), surf0)
    # the other order of the two readers
    fe.features_extract(drive[0], Q0)
    nd = store.set_frame_from_features(5, fe, leaf, TRANS)
    nw = win.set_scan_from_features(fe, 0, 0.9, TRANS, ahead=True)
    fe.features_extract(drive[1], Q0)
    win.slide_window()
    assert _same(win.get_scan(1), want_w) and _same(store.read_frame(5), want_d)
    win.close(); fe.close()


def test_world_cloud():
    d = mapping.DenseClouds(1, 1024, 2048)
    pose = gr.pose_at(3.0, -2.0, 0.5, 0.3)
    with pytest.raises(capi.GlioError) as e:
        d.world_cloud(pose)
    assert f"error {capi.E_STATE}:" in str(e.value)
    tab = np.vstack([kr.intensity_table(), _cloud(700, 31)])
    for leaf in (LEAF, 0.0):
        for trans in (None, TRANS):
            d.set_frame(0, tab, leaf, trans)
            assert _same(d.world_cloud(pose), dr.world_cloud(tab, trans, None, pose)), (leaf, trans)
            assert _same(d.world_cloud(gr.IDENTITY), kr.keyframe_cloud(tab, 0.0, trans))
            assert _same(d.read_frame(0), kr.keyframe_cloud(tab, leaf, trans))          # (reading the world cloud changes nothing)
    d.set_frame(0, np.zeros((0, 4), np.float32), LEAF)
    assert len(d.world_cloud(pose)) == 0
    d.close()


# ---- the map over the store
POSES = np.array([gr.pose_at(0.0, 0.0, 0.0), gr.pose_at(0.7, -0.2, 0.05, 0.02), gr.pose_at(1.5, 0.4, 0.0, -0.05), gr.pose_at(2.1, 1.0, 0.1, 0.4),
                  gr.pose_at(-1.0, 2.0, -0.1, 1.0)])


@pytest.fixture(scope="module")
def map_rig():
    from oracle import pyoracle as po
    d = mapping.DenseClouds(7, 4096, 4096)
    frames = []
    for k in range(5):
        c = _cloud(2000 + 37 * k, 50 + k, span=8.0)
        d.set_frame(k, c, LEAF, TRANS)
        frames.append(kr.keyframe_cloud(c, LEAF, TRANS))
        assert _same(d.read_frame(k), frames[k])
    d.set_frame(6, np.zeros((0, 4), np.float32), LEAF)               # frame 5 is never set, frame 6 is empty
    moved = [po.transform_cloud(frames[k], POSES[k][3:], POSES[k][:3]) for k in range(5)]
    assert _same(moved[3], dr.move(frames[3], POSES[3]))              # (the oracle's transformCloud is the restatement's)
    want, _ = gr.restated_voxel_grid(np.vstack(moved), 0.2)
    yield dict(d=d, frames=frames, want=want)
    d.close()


def test_map_over_the_store(map_rig):
    d, want = map_rig["d"], map_rig["want"]
    opts = mapping.default_opts(leaf=0.2, max_voxels=1 << 15, max_points_per_add=1 << 15)
    gm = mapping.GlobalMap(d, opts)
    all5 = list(range(5))
    info = gm.add(all5, POSES)
    assert info.n_voxels == gm.size() == len(want) and info.n_points_total == sum(len(f) for f in map_rig["frames"])
    five = gm.read()
    assert _same(five, want)
    # 1 + 4 frames, and clear + 5
    gm.clear(); gm.add([0], POSES[:1]); gm.add(all5[1:], POSES[1:])
    assert _same(gm.read(), five)
    gm.clear()
    assert gm.size() == 0
    gm.add(all5, POSES)
    assert _same(gm.read(), five)
    # refused adds leave size, bytes and device pointer as they were
    ptr = gm.points_dev()
    small = mapping.GlobalMap(d, mapping.default_opts(leaf=0.2, max_voxels=len(want) - 1, max_points_per_add=1 << 15))
    small.add([0], POSES[:1])
    keep_small, ptr_small = small.read(), small.points_dev()
    for g, frames, poses in ((gm, [5], POSES[:1]), (gm, [6], POSES[:1]), (gm, [7], POSES[:1]),          # never set, empty, outside [0, K)
                             (small, all5[1:], POSES[1:])):                                              # max_voxels exceeded
        with pytest.raises(capi.GlioError) as e:
            g.add(frames, poses)
        assert f"error {capi.E_ARG}:" in str(e.value), frames
    assert gm.points_dev() == ptr and _same(gm.read(), five)
    assert small.points_dev() == ptr_small and _same(small.read(), keep_small)
    # the store's next write to a frame comes behind the map's read, and the map reads what the store holds then
    c = _cloud(1500, 77, span=8.0)
    d.set_frame(4, c, LEAF)
    gm.clear(); gm.add([4], POSES[4:5])
    from oracle import pyoracle as po
    w4, _ = gr.restated_voxel_grid(po.transform_cloud(kr.keyframe_cloud(c, LEAF), POSES[4][3:], POSES[4][:3]), 0.2)
    assert _same(gm.read(), w4)
    d.set_frame(4, _cloud(2000 + 37 * 4, 54, span=8.0), LEAF, TRANS)                 # (as the rig made it)
    assert _same(d.read_frame(4), map_rig["frames"][4])
    small.close(); gm.close()


def test_a_map_on_an_association_gives_what_it_gave():
    faces = gr.faces_cloud()
    ba = batch.BatchAssociation(2, len(faces), 1000)
    ba.set_frame(0, faces)
    gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=0.2, max_voxels=1 << 16, max_points_per_add=1 << 15))
    gm.add([0], gr.IDENTITY[None, :])
    want, _ = gr.restated_voxel_grid(faces, 0.2)
    assert _same(gm.read(), want)
    gm.close(); ba.close()

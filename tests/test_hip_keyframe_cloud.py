"""The keyframe cloud on the device (glio_scan_filter_config, glio_set_scan_filtered*, glio_set_scan_from_features*, glio_get_scan) against the CPU
restatement tests/keyframe_cloud_restated.py followed by preproc_restated.voxel_grid.  The slot is read back with glio_get_scan."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_cloud_restated as kr  # noqa: E402
import preproc_restated as pr  # noqa: E402

from glio_amd import capi, features, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

pytestmark = pytest.mark.gpu

TRANS = (0.6, -0.05, 0.02)
IDENT = (1.0, 0.0, 0.0, 0.0)
Q0, T0 = np.array(IDENT), np.zeros(3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def drive():
    """raw scans of a 4-frame drive and the restatement's surf features of each (a few thousand points)"""
    raws = sl.drive(n_frames=4, n_scans=16, n_az=900)
    return raws, [pr.extract(r, 16)["surf"] for r in raws]


def _ctx(W=1, pts=1 << 13, max_in=1 << 13, map_pts=1 << 14):
    ctx = capi.Context(synth.default_opts(W, pts=pts, map_pts=map_pts))
    if max_in:
        ctx.scan_filter_config(max_in)
    return ctx


def _corr_same(a, b, slot=0):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a.get_correspondences(slot), b.get_correspondences(slot)))


@pytest.mark.parametrize("leaf", [0.9, 0.4])
def test_filter_alone(drive, leaf):
    """deskew_trans = NULL: the slot is pcl::VoxelGrid of the cloud bit for bit (count, order, four fields), and the association that follows equals the
    association after glio_set_scan of the expected cloud byte for byte"""
    surf = drive[1][0]
    want = kr.keyframe_cloud(surf, leaf)
    assert 100 < len(want) < len(surf)
    map_pts = pr.voxel_grid(drive[1][1], 0.4)
    a, b = _ctx(), _ctx(max_in=0)
    assert a.set_scan_filtered(0, surf, leaf) == len(want)
    assert _same(a.get_scan(0), want)
    b.set_scan(0, want)
    assert _same(b.get_scan(0), want)
    for c in (a, b):
        c.set_map(map_pts)
    na, nb = a.associate_resident(0, Q0, T0), b.associate_resident(0, Q0, T0)
    assert na == nb > 50 and _corr_same(a, b)
    a.close(); b.close()


@pytest.mark.parametrize("leaf", [0.9, 0.0, -1.0])
def test_reference_deskew(drive, leaf):
    """the reference's only call: trans = rel_pose's translation, quat the identity -- given as NULL and explicitly: both bit for bit the expected cloud"""
    surf = drive[1][1]
    want = kr.keyframe_cloud(surf, leaf, TRANS)
    assert not _same(want, kr.keyframe_cloud(surf, leaf))          # (the motion matters)
    ctx = _ctx()
    for quat in (None, IDENT):
        assert ctx.set_scan_filtered(0, surf, leaf, TRANS, quat) == len(want)
        assert _same(ctx.get_scan(0), want), quat
        ctx.set_scan(0, surf[:7])                                  # (something else in between)
    ctx.close()


def test_general_quat(drive):
    """yaw 0.03 rad over the sweep, leaf <= 0 so that no point can change voxel: identical counts, order and intensities, positions within
    2e-6 * range + 1e-6 m of the restatement (slerp through acos / sin, device against glibc: the gate of tests/test_hip_features.py)"""
    surf = drive[1][2]
    quat = (math.cos(0.015), 0.0, 0.0, math.sin(0.015))
    want = kr.keyframe_cloud(surf, 0.0, TRANS, quat)
    ctx = _ctx()
    assert ctx.set_scan_filtered(0, surf, 0.0, TRANS, quat) == len(surf)
    got = ctx.get_scan(0)
    assert got.shape == want.shape and np.array_equal(_bits(got[:, 3]), _bits(want[:, 3]))
    rng = np.linalg.norm(want[:, :3].astype(np.float64), axis=1)
    err = np.linalg.norm(got[:, :3].astype(np.float64) - want[:, :3], axis=1)
    print(f"general quat: max err {err.max():.3e} m, worst err - gate {(err - (2e-6 * rng + 1e-6)).max():.3e}")
    assert (err <= 2e-6 * rng + 1e-6).all()
    assert np.abs(got[:, :3] - surf[:, :3]).max() > 0.1               # (it moved)
    ctx.close()


def test_intensity_table_through_32_byte_records():
    tab = kr.intensity_table()
    rec = capi.to_pcl_xyzi(tab)
    ctx = _ctx()
    for leaf in (0.0, 0.5):
        want = kr.keyframe_cloud(tab, leaf, TRANS)
        assert ctx.set_scan_filtered(0, rec, leaf, TRANS, None, ioff=capi.PCL_XYZI_INTENSITY_OFFSET) == len(want)
        assert _same(ctx.get_scan(0), want), leaf
    # zero motion: the input itself
    assert ctx.set_scan_filtered(0, rec, 0.0, (0.0, 0.0, 0.0), IDENT, ioff=capi.PCL_XYZI_INTENSITY_OFFSET) == len(tab)
    assert _same(ctx.get_scan(0), tab)
    ctx.close()


def _random_cloud(n, seed, span=20.0):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-span, span, (n, 3))
    inten = rng.integers(0, 16, n) + rng.uniform(0.0, 0.11, n)
    return np.concatenate([xyz, inten[:, None]], 1).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1025])
def test_tile_boundaries(n):
    """points on both sides of zero on every axis, sizes around the kernel's 256-thread and 1024-point tiles"""
    p = _random_cloud(n, 100 + n, span=2.0)
    ctx = _ctx(pts=2048, max_in=2048)
    ctx.set_scan(0, _random_cloud(5, 1))
    for trans in (None, TRANS):
        want = kr.keyframe_cloud(p, 0.5, trans)
        assert ctx.set_scan_filtered(0, p, 0.5, trans) == len(want)
        assert _same(ctx.get_scan(0), want)
    if n > 1:
        assert (p[:, :3].min(0) < 0).all() and (p[:, :3].max(0) > 0).all() and len(want) < n
    ctx.close()


def test_one_voxel_full_slot_and_one_too_many():
    ctx = _ctx(pts=1024, max_in=4096)
    rng = np.random.default_rng(5)
    one = np.concatenate([rng.uniform(10.01, 10.49, (1000, 3)), rng.uniform(0, 16, (1000, 1))], 1).astype(np.float32)
    want = kr.keyframe_cloud(one, 0.5)
    assert len(want) == 1 and ctx.set_scan_filtered(0, one, 0.5) == 1 and _same(ctx.get_scan(0), want)
    # one point per voxel: a 33 x 32 lattice at the voxel centres, 1025 of them
    g = np.array([[0.25 + 0.5 * (i % 33), 0.25 + 0.5 * (i // 33), 0.25, float(i % 16)] for i in range(1025)], np.float32)
    g = g[np.random.default_rng(6).permutation(1025)]
    full = g[:1024]
    want = kr.keyframe_cloud(full, 0.5)
    assert len(want) == 1024
    assert ctx.set_scan_filtered(0, full, 0.5) == 1024 and _same(ctx.get_scan(0), want)          # exactly full
    with pytest.raises(capi.GlioError) as e:
        ctx.set_scan_filtered(0, g, 0.5)
    assert e.value.code == capi.E_ARG and e.value.n_out == 1025
    assert _same(ctx.get_scan(0), want)                                                           # the slot still holds its previous scan and count
    with pytest.raises(capi.GlioError) as e:
        ctx.set_scan_filtered(0, g, 0.0)                                                          # (the same without a filter)
    assert e.value.code == capi.E_ARG and e.value.n_out == 1025 and _same(ctx.get_scan(0), want)
    # and the stage goes on working after a refusal
    assert ctx.set_scan_filtered(0, one, 0.5) == 1
    ctx.close()


def test_pcl_overflow_rule_passes_the_cloud_through():
    p = _random_cloud(100, 9, span=5.0)
    p[17, :3] = (-1500.0, -1500.0, -1500.0)
    p[63, :3] = (1500.0, 1500.0, 1500.0)
    want = kr.keyframe_cloud(p, 0.2)
    assert _same(want, p)                                              # (15001^3 cells: the restatement passes it through)
    ctx = _ctx()
    assert ctx.set_scan_filtered(0, p, 0.2) == 100 and _same(ctx.get_scan(0), p)
    # the next call filters again (the interrupted build's bitmap bits are wiped)
    q = _random_cloud(300, 10, span=4.0)
    want = kr.keyframe_cloud(q, 0.5)
    assert ctx.set_scan_filtered(0, q, 0.5) == len(want) and _same(ctx.get_scan(0), want)
    ctx.close()


def test_refusals():
    p = _random_cloud(65, 11)
    ctx = _ctx(max_in=0)
    ctx.set_scan(0, p[:9])
    with pytest.raises(capi.GlioError) as e:
        ctx.set_scan_filtered(0, p, 0.5)                               # before glio_scan_filter_config
    assert e.value.code == capi.E_STATE
    ctx.scan_filter_config(64)
    for call in (lambda: ctx.set_scan_filtered(0, p, 0.5),              # n > max_input_points
                 lambda: ctx.set_scan_filtered(1, p[:10], 0.5),         # bad slot
                 lambda: ctx.set_scan_filtered(0, p[:10], 0.5, (0.1, float("nan"), 0.0)),
                 lambda: ctx.set_scan_filtered(0, p[:10], 0.5, TRANS, (1.0, 0.0, float("inf"), 0.0)),
                 lambda: ctx.set_scan_filtered(0, np.zeros((10, 3), np.float32), 0.5, ioff=8),        # 12-byte records
                 lambda: ctx.set_scan_filtered(0, p[:10], 0.5, ahead=True)):                          # W = 1: no row to send ahead into
        with pytest.raises(capi.GlioError) as e:
            call()
        assert e.value.code == capi.E_ARG
    with pytest.raises(capi.GlioError) as e:
        ctx.set_scan_from_features(ctx, 0, 0.5)                        # no extraction yet
    assert e.value.code == capi.E_STATE
    assert _same(ctx.get_scan(0), p[:9])                               # every refusal left the slot as it was
    assert ctx.set_scan_filtered(0, p[:64], 0.5) == len(kr.keyframe_cloud(p[:64], 0.5))
    ctx.close()


def _frontend(n_scans=16):
    fe = capi.Context(synth.default_opts(1, pts=1 << 14, map_pts=1 << 14))
    fe.features_config(features.default_opts(n_scans, max_raw_points=1 << 15))
    return fe


@pytest.mark.parametrize("leaf,trans", [(0.9, None), (0.9, TRANS), (0.0, TRANS)])
def test_resident_source_equals_host_source(drive, leaf, trans):
    raw = drive[0][0]
    fe = _frontend()
    fe.features_extract(raw, Q0)
    surf = fe.features_read(T.FEAT_SURF)
    assert len(surf) > 1000
    want = kr.keyframe_cloud(surf, leaf, trans)
    a, b = _ctx(W=2), _ctx(W=2)
    assert a.set_scan_from_features(fe, 1, leaf, trans) == len(want)
    assert b.set_scan_filtered(1, surf, leaf, trans) == len(want)
    ga, gb = a.get_scan(1), b.get_scan(1)
    assert _same(ga, gb) and _same(ga, want)
    assert _same(fe.features_read(T.FEAT_SURF), surf)                  # the de-skew is out of place
    a.close(); b.close(); fe.close()


@pytest.mark.parametrize("own", [False, True])
def test_handover_is_ordered_before_the_next_extraction(drive, own):
    """scan 0 handed over, scan 1 extracted at once on the front end, then the slot read: scan 0's cloud (own: the front end is the window's context)"""
    raws = drive[0]
    fe = _frontend()
    ctx = fe if own else _ctx()
    if own:
        ctx.scan_filter_config(1 << 13)
    fe.features_extract(raws[0], Q0)
    surf0 = fe.features_read(T.FEAT_SURF)
    want = kr.keyframe_cloud(surf0, 0.9, TRANS)
    n = ctx.set_scan_from_features(fe, 0, 0.9, TRANS)
    fe.features_extract(raws[1], Q0)
    assert n == len(want) and _same(ctx.get_scan(0), want)
    assert not _same(fe.features_read(T.FEAT_SURF), surf0)
    if not own:
        ctx.close()
    fe.close()


@pytest.mark.parametrize("resident", [False, True])
def test_ahead_forms(drive, resident):
    """set_scan_filtered_ahead / set_scan_from_features_ahead after a window's association, then glio_slide_window: slot W - 1 equals what the slot form
    gives, and the next associate_window matches a context that used glio_set_scan for the same cloud, bit for bit"""
    W = 3
    raws, surfs = drive
    map_pts = pr.voxel_grid(np.concatenate(surfs[:2]), 0.4)
    fe = _frontend()
    fe.features_extract(raws[3], Q0)
    new = fe.features_read(T.FEAT_SURF)
    want = kr.keyframe_cloud(new, 0.9, TRANS)
    a, b, c = _ctx(W=W), _ctx(W=W, max_in=0), _ctx(W=W)
    scans = [pr.voxel_grid(s, 0.9) for s in surfs[:3]]
    quats = np.tile(Q0, (W, 1)); trans = np.zeros((W, 3))
    for x in (a, b):
        x.set_map(map_pts)
        for s in range(W):
            x.set_scan(s, scans[s])
        x.associate_window(quats, trans)
    if resident:
        n = a.set_scan_from_features(fe, 0, 0.9, TRANS, ahead=True)
    else:
        n = a.set_scan_filtered(0, new, 0.9, TRANS, ahead=True)
    assert n == len(want)
    a.slide_window()
    b.slide_window(); b.set_scan(W - 1, want)
    assert c.set_scan_filtered(W - 1, new, 0.9, TRANS) == n
    assert _same(a.get_scan(W - 1), want) and _same(c.get_scan(W - 1), want)
    assert _same(a.get_scan(0), scans[1]) and _same(a.get_scan(1), scans[2])
    ca, cb = a.associate_window(quats, trans), b.associate_window(quats, trans)
    assert np.array_equal(ca, cb) and ca[W - 1] > 50
    for s in range(W):
        assert _corr_same(a, b, s), s
    a.close(); b.close(); c.close(); fe.close()

"""glio_features_* (Preprocessing::cloudHandler on the device) against the CPU restatement tests/preproc_restated.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_restated as pr  # noqa: E402
from features_cases import _bits, _ctx, _intensity_close, _same, _yaw_q  # noqa: E402,F401

from glio_amd import capi, features, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

pytestmark = pytest.mark.gpu

OUTPUTS = [("sharp", T.FEAT_SHARP), ("less_sharp", T.FEAT_EDGE_LESS_SHARP), ("flat", T.FEAT_FLAT), ("surf", T.FEAT_SURF)]


@pytest.mark.parametrize("n_scans,yaw,stride", [(16, 0.0, 16), (16, 0.08, 32), (32, 0.0, 32), (32, 0.08, 16), (64, 0.0, 16), (64, 0.08, 32)])
def test_selection_stages_are_bit_exact_on_the_devices_cut_cloud(n_scans, yaw, stride):
    """Steps 4-6 (curvature, sectors, picks, less-flat, per-ring VoxelGrid) restated on the device's own /lidar_cloud_cutted: every output bit for bit"""
    raw = sl.make_scan(n_scans, 1800 if n_scans == 32 else 900, sweep_yaw=yaw, seed=20 + n_scans)
    rec = sl.to_records(raw, stride, 16 if stride == 32 else 12)
    ctx = _ctx(n_scans)
    cnt = ctx.features_extract(rec, _yaw_q(yaw), ioff=16 if stride == 32 else 12)
    cut = ctx.features_read(T.FEAT_CUT_CLOUD)
    assert cnt.in_ == len(raw) and cnt.cut == len(cut) > 0
    rs, size = pr.rings_of_cut(cut, n_scans)
    want = pr.select(cut, rs, size)
    for name, which in OUTPUTS:
        got = ctx.features_read(which)
        assert _same(got, want[name]), (name, got.shape, want[name].shape)
    assert (cnt.sharp, cnt.less_sharp, cnt.flat, cnt.surf) == tuple(len(want[k]) for k in ("sharp", "less_sharp", "flat", "surf"))
    ctx.close()


@pytest.mark.parametrize("n_scans", [16, 32, 64])
def test_end_to_end_from_the_raw_scan_identity_rotation(n_scans):
    """Bin-centred lasers, q_imu = identity (slerp's linear branch: no transcendental function in the de-skew): the survivors, their rings and order
    identical, every output's xyz bit-identical with the same counts, intensities within 2 float ulps (atan2f on the device vs glibc)"""
    raw = sl.make_scan(n_scans, 1800 if n_scans == 32 else 900, seed=40 + n_scans)
    want = pr.extract(raw, n_scans)
    ctx = _ctx(n_scans)
    cnt = ctx.features_extract(raw, np.array([1.0, 0, 0, 0]))
    assert cnt.kept == want["kept"] and cnt.cut == len(want["cut"])
    cut = ctx.features_read(T.FEAT_CUT_CLOUD)
    assert np.array_equal(pr.rings_of_cut(cut, n_scans)[1], want["ring_size"])
    assert _same(cut[:, :3], want["cut"][:, :3])
    assert _intensity_close(cut[:, 3], want["cut"][:, 3])
    for name, which in OUTPUTS:
        got = ctx.features_read(which)
        assert got.shape == want[name].shape and _same(got[:, :3], want[name][:, :3]), name
        assert _intensity_close(got[:, 3], want[name][:, 3]), name
    ctx.close()


@pytest.mark.parametrize("n_scans", [16, 32])
def test_end_to_end_with_a_sweep_rotation(n_scans):
    """q_imu != identity (slerp through acos / sin): the same counts and order, positions within 2e-6 * range + 1e-6 m"""
    yaw = 0.1
    raw = sl.make_scan(n_scans, 1800 if n_scans == 32 else 900, sweep_yaw=yaw, seed=60 + n_scans)
    want = pr.extract(raw, n_scans, q_imu=_yaw_q(yaw))
    ctx = _ctx(n_scans)
    cnt = ctx.features_extract(raw, _yaw_q(yaw))
    assert cnt.kept == want["kept"] and cnt.cut == len(want["cut"])
    for name, which in OUTPUTS + [("cut", T.FEAT_CUT_CLOUD)]:
        got = ctx.features_read(which)
        w = want[name]
        assert got.shape == w.shape, name
        rng = np.linalg.norm(w[:, :3].astype(np.float64), axis=1)
        err = np.linalg.norm(got[:, :3].astype(np.float64) - w[:, :3], axis=1)
        assert (err <= 2e-6 * rng + 1e-6).all(), (name, (err - 2e-6 * rng).max())
    ctx.close()


def test_knife_edge_hdl32_table():
    """Nominal HDL-32E elevations sit on the 32-line formula's bin edges: the device and the restatement agree on every point whose bin coordinate
    is more than 1e-4 from an integer (the count of closer points is reported)"""
    raw = sl.make_scan(32, 1800, table="hdl32", seed=81)
    ctx = _ctx(32)
    ctx.features_extract(raw, np.array([1.0, 0, 0, 0]))
    cut = ctx.features_read(T.FEAT_CUT_CLOUD)
    dev = {cut[i, :3].tobytes(): int(np.rint(cut[i, 3])) for i in range(len(cut))}     # identity rotation: xyz pass through unchanged
    keep = pr.survivors(raw[:, :3])
    p = raw[keep, :3]
    sid, angle = pr.scan_ids(p, 32)
    binc = (angle.astype(np.float64) + 92.0 / 3.0) * 3.0 / 4.0
    near = np.abs(binc - np.rint(binc)) <= 1e-4
    far_bad = 0
    for i in range(len(p)):
        if near[i]:
            continue
        d = dev.get(p[i].tobytes(), -1)
        far_bad += d != int(sid[i])
    print(f"knife edge: {int(near.sum())} of {len(p)} survivors within 1e-4 of a bin edge")
    assert far_bad == 0
    ctx.close()


def test_one_ring_of_60000_points_takes_the_global_sort_path():
    """60 000 points in ONE ring (z = 0): sectors of 10 000 points and a less-flat cloud far beyond the LDS sort"""
    rng = np.random.default_rng(5)
    n = 60000
    a = 0.4 - 2 * np.pi * np.arange(n) / n
    r = 12.0 / np.maximum(np.abs(np.cos(a)), np.abs(np.sin(a))) ** 0.7 + 0.01 * rng.standard_normal(n)      # a rounded square: corners and flats
    raw = np.zeros((n, 4), np.float32)
    raw[:, 0], raw[:, 1] = r * np.cos(a), r * np.sin(a)
    want = pr.extract(raw, 32)
    assert np.count_nonzero(want["ring_size"]) == 1
    ctx = _ctx(32)
    cnt = ctx.features_extract(raw, np.array([1.0, 0, 0, 0]))
    assert cnt.cut == n
    for name, which in OUTPUTS:
        got = ctx.features_read(which)
        assert got.shape == want[name].shape and _same(got[:, :3], want[name][:, :3]), name
    ctx.close()


def test_robustness_edges():
    lib = capi.load()
    ctx = capi.Context(synth.default_opts(1, pts=4096, map_pts=4096))
    q = np.array([1.0, 0, 0, 0])
    cnt = T.GlioFeatCounts()
    pts = np.ones((10, 4), np.float32)
    assert lib.glio_features_extract(ctx._h, T.fptr(pts), 10, T.dptr(q), C.byref(cnt)) == -3          # GLIO_E_STATE before config
    ctx.features_config(features.default_opts(32, max_raw_points=1000))
    big = np.full((1001, 4), 5.0, np.float32)
    assert lib.glio_features_extract(ctx._h, T.fptr(big), 1001, T.dptr(q), C.byref(cnt)) == -1       # GLIO_E_ARG above max_raw_points
    inside = np.random.default_rng(1).uniform(-1.5, 1.5, (900, 4)).astype(np.float32)                   # all within 3 m
    c = ctx.features_extract(inside, q)
    assert c.as_dict() == {"in": 900, "kept": 0, "cut": 0, "sharp": 0, "less_sharp": 0, "flat": 0, "surf": 0}
    assert len(ctx.features_read(T.FEAT_SURF)) == 0
    ctx.close()


def test_two_calls_give_the_same_bits():
    raw = sl.make_scan(32, 1800, sweep_yaw=0.05, seed=99)
    ctx = _ctx(32)
    outs = []
    for _ in range(2):
        ctx.features_extract(raw, _yaw_q(0.05))
        outs.append([ctx.features_read(w) for _, w in OUTPUTS + [("cut", T.FEAT_CUT_CLOUD)]])
    for a, b in zip(*outs):
        assert _same(a, b)
    ctx.close()


def test_features_leave_the_window_solve_untouched():
    """a context with features configured (and used) solves a small window exactly as one without"""
    win = synth.make_window(W=4, pts_per_scan=600, with_gnss=True, with_prior=True, seed=synth.SEED_BASE)
    res = []
    for with_feat in (False, True):
        ctx = capi.Context(win.opts)
        if with_feat:
            ctx.features_config(features.default_opts(16, max_raw_points=20000))
            ctx.features_extract(sl.make_scan(16, 600, seed=3), np.array([1.0, 0, 0, 0]))
        ctx.set_map(win.map_pts)
        for s in range(win.W):
            q2, t2 = capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s])
            ctx.associate(s, win.scans[s], q2, t2)
        ctx.load_window(win, None)
        sol, summ = ctx.solve(win.init)
        res.append((sol.trans.copy(), sol.quat.copy(), summ.iterations))
        ctx.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


def test_to_scan_matches_the_restated_front_end_filter():
    """glio_features_to_scan: the surf features voxel-filtered at 0.2 m on the device == VoxelGrid(0.2) of the device's surf cloud; leaf <= 0 copies"""
    raw = sl.make_scan(32, 1800, seed=7)
    ctx = _ctx(32)
    ctx.features_extract(raw, np.array([1.0, 0, 0, 0]))
    surf = ctx.features_read(T.FEAT_SURF)
    n = ctx.features_to_scan(0, 0.2)
    got = ctx.features_read(T.FEAT_LAST_SCAN)
    assert n == len(got) and _same(got, pr.voxel_grid(surf, 0.2))
    assert ctx.features_to_scan(0, 0.0) == len(surf) and _same(ctx.features_read(T.FEAT_LAST_SCAN), surf)
    ctx.close()

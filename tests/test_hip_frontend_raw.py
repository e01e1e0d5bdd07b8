"""The front end from raw scans: odometry.ScanToMapOdometry.run_raw (features on the device, the 0.2 m filter on the device, the previous scan pushed
from slot 0) against run() fed with the restatement's features, and the C++ runRaw against the Python run_raw."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preproc_restated as pr  # noqa: E402

from glio_amd import capi, features, odometry, synth_lidar as sl  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1.0, 0, 0, 0])


def _drive():
    return sl.drive(n_frames=8, n_scans=16, n_az=900)


def test_run_raw_equals_run_on_the_restated_features():
    """8-scan drive, bin-centred lasers, q_imu = identity: run_raw gives bit-identical poses, rounds, kept counts and map sizes to run() fed with the
    restatement's surf features filtered at 0.2 m (pcl float accumulation in the local map on both)"""
    scans = _drive()
    o = odometry.frontend_opts(1 << 14, 1 << 16)
    ctx_raw, ctx_ref = capi.Context(o), capi.Context(o)
    ctx_raw.features_config(features.default_opts(16, max_raw_points=1 << 15))
    od_raw, od_ref = odometry.ScanToMapOdometry(ctx_raw), odometry.ScanToMapOdometry(ctx_ref)
    for k, raw in enumerate(scans):
        if k == 1:
            ctx_raw.localmap_set_accumulation(1); ctx_ref.localmap_set_accumulation(1)
        p_raw, r_raw, cnt = od_raw.run_raw(raw, IDENTITY, max_points=o.max_points_per_scan)
        want = pr.extract(raw, 16)
        assert cnt.surf == len(want["surf"])
        ds = pr.voxel_grid(want["surf"], odometry.LOCAL_MAP_LEAF)
        p_ref, r_ref = od_ref.run(ds, max_points=o.max_points_per_scan)
        assert np.array_equal(p_raw, p_ref), (k, np.abs(p_raw - p_ref).max())
        assert len(r_raw) == len(r_ref)
        for (sa, ka), (sb, kb) in zip(r_raw, r_ref):
            assert ka == kb and sa.iterations == sb.iterations and sa.termination == sb.termination, k
        assert od_raw.map_points == od_ref.map_points
    assert np.linalg.norm(od_raw.rel_pose[4:]) > 0.3          # it moved (0.6 m per scan)
    ctx_raw.close(); ctx_ref.close()


def test_cpp_run_raw_equals_the_python_twin(tmp_path):
    from glio_amd.host import window_io
    scans = _drive()[:6]
    o = odometry.frontend_opts(1 << 14, 1 << 16)
    fo = features.default_opts(16, max_raw_points=1 << 15)
    recs = [sl.to_records(s, 32, 16) for s in scans]
    path = str(tmp_path / "raw.bin")
    window_io.write_frontend_raw_stream(path, o, fo, recs, [IDENTITY] * len(recs), scan_match_cnt=2, ioff=16)
    poses, rows, info = window_io.run_demo_frontend_raw(path)
    ctx = capi.Context(o)
    ctx.features_config(fo)
    od = odometry.ScanToMapOdometry(ctx, scan_match_cnt=2)
    for k, rec in enumerate(recs):
        p, rounds, cnt = od.run_raw(rec, IDENTITY, stride=32, ioff=16, max_points=o.max_points_per_scan)
        assert np.array_equal(p, poses[k]), (k, np.abs(p - poses[k]).max())
        assert rows[k]["rounds"] == len(rounds) and rows[k]["surf"] == cnt.surf
        assert rows[k]["kept"] == sum(kk for _, kk in rounds)
        if k >= 1:
            assert rows[k]["map_points"] == od.map_points
    assert info["scans"] == len(recs)
    ctx.close()

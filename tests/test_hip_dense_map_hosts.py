"""The dense map in the hosts: the C++ demo (runRaw -> glio::KeyframeGate -> glio::DenseClouds::setFrameFromFeatures -> glio::GlobalMap on the store) against the
Python twin on the same drive: keyframe decisions, frame counts, frame bytes, map bytes -- and the restatements of both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_map_restated as gr  # noqa: E402
import keyframe_cloud_restated as kr  # noqa: E402

from glio_amd import capi, features, loop, mapping, odometry, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1.0, 0, 0, 0])


def _fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_demo_equals_the_python_twin(tmp_path):
    from glio_amd.host import window_io
    from oracle import pyoracle as po
    leaf, map_leaf = 0.4, 0.2
    scans = sl.drive(n_frames=8, n_scans=16, n_az=600)
    o = odometry.frontend_opts(1 << 14, 1 << 16)
    fo = features.default_opts(16, max_raw_points=1 << 14)
    recs = [sl.to_records(s, 32, 16) for s in scans]
    path = str(tmp_path / "raw.bin")
    window_io.write_frontend_raw_stream(path, o, fo, recs, [IDENTITY] * len(recs), scan_match_cnt=2, ioff=16)
    rows, kfs, gmap, info = window_io.run_demo_dense_map(path, leaf=leaf, map_leaf=map_leaf, chunk=2)
    fe = capi.Context(o)
    fe.features_config(fo)
    od = odometry.ScanToMapOdometry(fe, scan_match_cnt=2)
    dense = mapping.DenseClouds(len(recs), 1 << 14, 1 << 14)
    gate = odometry.KeyframeGate()
    mine, pose_info, moved = [], [], []
    for k, rec in enumerate(recs):
        _, _, cnt = od.run_raw(rec, IDENTITY, stride=32, ioff=16, max_points=o.max_points_per_scan)
        kf = gate.update_from(od)
        assert rows[k] == {"kf": int(kf), "cut": cnt.cut}, k
        if not kf:
            continue
        f = len(mine)
        trans = od.rel_pose[4:].copy()
        n = dense.set_frame_from_features(f, fe, leaf, trans)
        got = dense.read_frame(f)
        want = kr.keyframe_cloud(fe.features_read(T.FEAT_CUT_CLOUD), leaf, trans)
        assert n == len(want) and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        mine.append({"scan": k, "frame": f, "n": n, "hash": _fnv1a(got)})
        pose_info.append(np.r_[od.abs_pose[4:], od.abs_pose[:4]])
    assert kfs == mine and len(mine) >= 3 and info["keyframes"] == len(mine)
    poses = loop.frame_poses(np.array(pose_info), (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    gm = mapping.GlobalMap(dense, mapping.default_opts(leaf=map_leaf))
    for a in range(0, len(mine), 2):
        part = list(range(a, min(a + 2, len(mine))))
        minfo = gm.add(part, poses[part])
    got = gm.read()
    assert gmap == {"n_voxels": len(got), "hash": _fnv1a(got), "n_points": minfo.n_points_total, "frames": len(mine)}
    moved = [po.transform_cloud(dense.read_frame(f), poses[f][3:], poses[f][:3]) for f in range(len(mine))]
    want, _ = gr.restated_voxel_grid(np.vstack(moved), map_leaf)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    gm.close(); dense.close(); fe.close()

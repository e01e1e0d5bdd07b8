"""The keyframe cloud in the hosts: the C++ demo (runRaw -> glio::KeyframeGate -> setScanFromFrontEnd / setScanFiltered) against the Python twin, and the
sliding-window drivers with filter=LEAF, fed unfiltered clouds, against the default drivers fed the restatement's filtered clouds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_cloud_restated as kr  # noqa: E402
import preproc_restated as pr  # noqa: E402

from glio_amd import capi, features, odometry, sliding, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = np.array([1.0, 0, 0, 0])


def _fnv1a(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("deskew", [True, False])
def test_cpp_demo_equals_the_python_twin(tmp_path, deskew):
    """a 6-scan drive: the same keyframe decisions, the same counts and the same bytes per keyframe, resident route and host route, in both hosts --
    and the restatement's cloud"""
    from glio_amd.host import window_io
    W, leaf = 3, 0.9
    scans = sl.drive(n_frames=6, n_scans=16, n_az=900)
    o = odometry.frontend_opts(1 << 14, 1 << 16)
    fo = features.default_opts(16, max_raw_points=1 << 15)
    recs = [sl.to_records(s, 32, 16) for s in scans]
    path = str(tmp_path / "raw.bin")
    window_io.write_frontend_raw_stream(path, o, fo, recs, [IDENTITY] * len(recs), scan_match_cnt=2, ioff=16)
    rows, kfs, info = window_io.run_demo_keyframe_cloud(path, leaf=leaf, deskew=deskew, window=W)
    fe = capi.Context(o)
    fe.features_config(fo)
    od = odometry.ScanToMapOdometry(fe, scan_match_cnt=2)
    win = capi.Context(synth.default_opts(W, pts=o.max_points_per_scan, map_pts=64))
    win.scan_filter_config(o.max_points_per_scan)
    gate = odometry.KeyframeGate()
    mine = []
    for k, rec in enumerate(recs):
        _, _, cnt = od.run_raw(rec, IDENTITY, stride=32, ioff=16, max_points=o.max_points_per_scan)
        kf = gate.update_from(od)
        assert rows[k] == {"kf": int(kf), "surf": cnt.surf}, k
        if not kf:
            continue
        slot = len(mine) % W
        trans = od.rel_pose[4:].copy() if deskew else None
        n = win.set_scan_from_features(fe, slot, leaf, trans)
        got = win.get_scan(slot)
        want = kr.keyframe_cloud(fe.features_read(T.FEAT_SURF), leaf, trans)
        assert n == len(want) and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), k
        mine.append({"scan": k, "slot": slot, "n_resident": n, "hash_resident": _fnv1a(got), "n_host": n, "hash_host": _fnv1a(got)})
    assert kfs == mine
    assert [r["kf"] for r in rows] == [0, 1, 0, 0, 1, 0]          # the initialisation scan, the first judged scan, then every third while it moves
    assert info["keyframes"] == len(mine) == 2 and info["deskew"] == int(deskew)
    win.close(); fe.close()


@pytest.mark.parametrize("resident", [False, True])
def test_drivers_with_the_filter_equal_the_default_drivers_on_filtered_clouds(resident):
    """3 keyframes at W = 3: identical solve summaries, counts and poses"""
    W, L, leaf = 3, 5, 0.9
    long = synth.make_window(W=L, pts_per_scan=3000, seed=synth.SEED_BASE + 43)
    filtered = [pr.voxel_grid(s, leaf) for s in long.scans]
    assert all(100 < len(f) < len(s) for f, s in zip(filtered, long.scans))
    opts = synth.default_opts(W, pts=4096, map_pts=max(len(long.map_pts), 64))
    first = T.WindowState(W)
    first.trans[:], first.quat[:], first.speed_bias[:] = long.init.trans[:W], long.init.quat[:W], long.init.speed_bias[:W]
    ca, cb = capi.Context(opts), capi.Context(opts)
    cls = sliding.ResidentSlidingWindow if resident else sliding.SlidingWindowDriver
    da, db = cls(ca, opts, filter=leaf, filter_max_points=4096), cls(cb, opts)
    da.start(first); db.start(first)
    for k in range(L - W + 1):
        sa, ma, na = da.step(long.map_pts, long.scans[k:k + W], long.preints[k:k + W - 1])
        sb, mb, nb = db.step(long.map_pts, filtered[k:k + W], long.preints[k:k + W - 1])
        assert na == nb and sum(na) > 100, k
        assert ma.as_dict() == mb.as_dict(), k
        assert np.array_equal(sa.trans, sb.trans) and np.array_equal(sa.quat, sb.quat) and np.array_equal(sa.speed_bias, sb.speed_bias), k
        if k + W < L:
            for d in (da, db):
                d.slide(long.init.trans[k + W], long.init.quat[k + W], long.init.speed_bias[k + W])
    ca.close(); cb.close()

"""GPU: the pose graph's two hosts and the hand-over of its poses.  host_demo_pose_graph (C++: glio::GlobalGraph / glio::PoseGraph, glio_posegraph_backend.hpp)
and the Python driver (posegraph.GlobalGraph) run the same drive -- frames, a keyframe every few frames, some GPS fixes, one loop back to the start -- and must
agree; the corrected keyframe poses are then taken, unchanged, by glio_gmap_add_frames and glio_localmap_rebuild_from_frames."""
import json
import os

import numpy as np
import pytest

import pose_graph_restated as Wt
from glio_amd import batch, capi, mapping, posegraph, synth
from glio_amd import ctypes_types as T
from glio_amd.host import window_io

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_spread.json")))
W = 3
F, STEP = 61, 4


@pytest.fixture(scope="module")
def drive():
    truth = Wt.circle_truth(F, radius=25.0, turn=0.97, z_amp=0.3)
    frames = Wt.noisy_odometry(truth, np.random.default_rng(21), 2e-3, 5e-3)
    kf = list(range(0, F, STEP))                          # 16 keyframes; the last W - 1 are still in the window
    latest, closest = len(kf) - W, 0                      # the keyframe that just left the window closes the loop with the first
    rel = Wt.between(truth[kf[latest]], truth[kf[closest]])
    var = np.full(6, 0.04)
    rng = np.random.default_rng(22)
    gps = [(f, truth[f, :3] + rng.normal(0, 0.5, 3), np.array([0.5, 2.0, 4.0])) for f in (8, 24, 40)]
    return dict(frames=frames, kf=kf, latest=latest, closest=closest, rel=rel, var=var, gps=gps)


def python_driver(d):
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=F, max_loops=4, max_unary=len(d["gps"])))
    gg = posegraph.GlobalGraph(pg, W)
    calls = []
    for n in range(1, len(d["kf"]) + 1):
        ids = gg.keyframe_call(d["frames"][:d["kf"][n - 1] + 1], d["kf"], n)
        if ids:
            calls.append((n, ids[0], ids[-1]))
    for g in d["gps"]:
        pg.add_gps(*g)
    before = pg.error()
    info = gg.loop_closed(d["kf"], d["latest"], d["closest"], (d["rel"], d["var"]))
    return pg, gg, info, before, calls


def test_cpp_host_and_python_driver_agree(drive, tmp_path):
    path = str(tmp_path / "case.bin")
    window_io.write_pose_graph_case(path, drive["frames"], drive["kf"], W, drive["latest"], drive["closest"], drive["rel"], drive["var"], drive["gps"])
    cpp = window_io.run_demo_pose_graph(path)              # exits 0, or this raises
    pg, gg, info, before, calls = python_driver(drive)
    want = pg.read_poses()
    assert cpp["calls"] == calls and calls[0] == (W, 0, 0) and calls[-1][2] == drive["kf"][drive["latest"]]
    assert len(cpp["poses"]) == pg.size() == drive["kf"][drive["latest"]] + 1
    assert (cpp["iterations"], cpp["termination"]) == (info.iterations, info.termination) and info.termination == T.PGRAPH_CONVERGED
    assert cpp["n_keyframe_poses"] == len(drive["kf"]) - W + 1
    rel = Wt.spread(cpp["poses"], want, True)
    print("C++ against Python, relative to node 0:", rel, "errors", before, info.initial_error, info.final_error)
    assert rel[0] <= 100 * GOLD["S_rel_m"] and rel[1] <= 100 * GOLD["S_rel_rad"], rel
    assert cpp["final_error"] == info.final_error and cpp["error_before"] == before
    assert info.final_error < info.initial_error and info.initial_error > before       # the loop edge arrived after `before` was taken
    pg.close()


def test_corrected_poses_are_taken_by_the_global_map_and_the_local_map(drive):
    pg, gg, info, _, _ = python_driver(drive)
    poses = gg.keyframe_poses(drive["kf"], 4)             # the corrected poses of the first four keyframes, as read
    assert poses.shape == (4, 7) and np.array_equal(poses, pg.read_poses()[[0, 4, 8, 12]])
    win = synth.make_window(W=4, pts_per_scan=1500, seed=synth.SEED_BASE + 5, scan_radius=20.0)
    ba = batch.BatchAssociation(4, 2048, 16)
    for s in range(4):
        ba.set_frame(s, np.ascontiguousarray(win.scans[s]))
    gm = mapping.GlobalMap(ba, mapping.default_opts(max_voxels=1 << 14, max_points_per_add=1 << 13))
    mi = gm.add([0, 1, 2, 3], poses)
    assert mi.n_points_total == sum(len(win.scans[s]) for s in range(4)) and 0 < mi.n_voxels == gm.size()
    ctx = capi.Context(synth.default_opts(1, pts=2048, map_pts=1 << 15))
    ctx.localmap_config(4, 0.4, 2048)
    n = ctx.localmap_rebuild_from_frames(ba, [0, 1, 2, 3], poses)
    assert n > 0 and len(ctx.localmap_read()) == n
    ctx.close(); gm.close(); ba.close(); pg.close()

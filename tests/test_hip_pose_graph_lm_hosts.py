"""GPU: the damped solve through the pose graph's two hosts.  host_demo_pose_graph ... damped=1 (C++: glio::GlobalGraph::loopClosed(..., true),
glio_posegraph_backend.hpp) and the Python twin (posegraph.GlobalGraph.loop_closed(..., damped=True)) run a drive that revisits its start with the drift under
which Gauss-Newton's first step raises the error.  Both call the same library with the same bytes: they agree bit for bit.  Without damped=1 the demo prints
what it always printed."""
import numpy as np
import pytest

import pose_graph_restated as Wt
from glio_amd import posegraph
from glio_amd import ctypes_types as T
from glio_amd.host import window_io

pytestmark = pytest.mark.gpu

W = 3
F, STEP = 157, 4


@pytest.fixture(scope="module")
def drive():
    truth = Wt.circle_truth(F)
    frames = Wt.noisy_odometry(truth, np.random.default_rng(1), 5e-2, 3e-2)
    kf = list(range(0, F, STEP))                          # 40 keyframes; the last W - 1 are still in the window
    latest, closest = len(kf) - W, 0                      # the keyframe that just left the window closes the loop with the first
    return dict(frames=frames, kf=kf, latest=latest, closest=closest, rel=Wt.between(truth[kf[latest]], truth[kf[closest]]), var=np.full(6, 0.09))


def python_driver(d, damped):
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=F, max_loops=4, max_unary=1))
    gg = posegraph.GlobalGraph(pg, W)
    for n in range(1, len(d["kf"]) + 1):
        gg.keyframe_call(d["frames"][:d["kf"][n - 1] + 1], d["kf"], n)
    before = pg.error()
    info = gg.loop_closed(d["kf"], d["latest"], d["closest"], (d["rel"], d["var"]), damped=damped)
    poses = pg.read_poses()
    pg.close()
    return info, before, poses


def test_cpp_host_and_python_twin_agree_bit_for_bit(drive, tmp_path):
    path = str(tmp_path / "case.bin")
    window_io.write_pose_graph_case(path, drive["frames"], drive["kf"], W, drive["latest"], drive["closest"], drive["rel"], drive["var"], [])
    plain = window_io.run_demo_pose_graph(path, keep_stdout=True)
    cpp = window_io.run_demo_pose_graph(path, damped=True)
    gi, gbefore, gposes = python_driver(drive, False)
    info, before, poses = python_driver(drive, True)
    print("undamped", gi.as_dict())
    print("damped", info.as_dict())
    # the drive is one of those the damped solve exists for
    assert gi.final_error > gi.initial_error and gi.termination == T.PGRAPH_CONVERGED and gi.iterations == 1
    assert info.final_error < 0.7 * info.initial_error and info.initial_error == gi.initial_error and info.termination == T.PGRAPH_CONVERGED
    # C++ against Python, damped: the same library, the same bytes
    assert np.array_equal(cpp["poses"].view(np.uint64), poses.view(np.uint64))
    assert np.array_equal(cpp["history"].view(np.uint64), info.history.view(np.uint64))
    assert (cpp["iterations"], cpp["termination"], cpp["error_before"], cpp["initial_error"], cpp["final_error"], cpp["separators"], cpp["segments"]) == \
        (info.iterations, info.termination, before, info.initial_error, info.final_error, info.separators, info.segments)
    assert (cpp["accepted"], cpp["rejected"], cpp["invalid"], cpp["trials"], cpp["final_radius"]) == (info.accepted, info.rejected, info.invalid, info.trials, info.final_radius)
    # without damped=1: the undamped solve, and no line the demo did not print before
    assert np.array_equal(plain["poses"].view(np.uint64), gposes.view(np.uint64))
    assert (plain["iterations"], plain["termination"], plain["final_error"]) == (gi.iterations, gi.termination, gi.final_error)
    assert {ln.split()[0] for ln in plain["stdout"].splitlines() if ln.strip()} == {"call", "solve", "pose", "keyframes"}
    assert "accepted" not in plain and "history" not in plain

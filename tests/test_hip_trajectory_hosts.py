"""The two hosts of the every-frame trajectory on the same synthetic drive: host_demo_trajectory (glio::Trajectory, glio_trajectory_backend.hpp) against
glio_amd/trajectory.py bit for bit -- pose_each_frame, the rows after resolve_all, the per-gap summaries -- and the global graph either route feeds
(GlobalGraph.keyframe_call accepts the array and ends with the same nodes)."""
import numpy as np
import pytest

from glio_amd import posegraph, trajectory
from glio_amd.host import window_io

pytestmark = pytest.mark.gpu


def test_cpp_and_python_hosts_agree_bit_for_bit(tmp_path):
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    d = trajectory.make_drive(n_keyframes=12, W=4, seed=5)
    path = str(tmp_path / "drive.bin")
    window_io.write_trajectory_case(path, d["imu"], d["frame_stamps"], d["keyframe_id_in_frame"], d["imu_idx_in_kf"], d["W"], d["keyframe_poses"], d["start_states"],
                                    d["corrected"])
    cpp = window_io.run_demo_trajectory(path)
    F = len(d["frame_stamps"])
    store = trajectory.TrajectoryStore(max_gaps=12)
    graph = posegraph.PoseGraph(posegraph.default_opts(max_nodes=F, max_loops=1, max_unary=1))
    traj, calls = trajectory.run_drive(d, store, graph)
    rows = traj.poses()
    nodes = graph.read_poses()
    kf = d["keyframe_id_in_frame"]
    n_gaps = len(kf) - d["W"]
    assert rows.shape == (kf[n_gaps] + 1, 7) and len(calls) == n_gaps
    assert any(c[2] > 0 for c in calls) and any(c[2] == 0 for c in calls) or len(set(c[2] for c in calls)) > 1, calls          # gaps of different sizes
    assert cpp["calls"] == calls, (cpp["calls"], calls)
    assert cpp["frames"].tobytes() == rows.tobytes()
    assert len(nodes) == len(rows) and cpp["nodes"].tobytes() == nodes.tobytes()
    assert [g[1:] for g in cpp["graph"]][-1][1] == len(rows) - 1
    # keyframe rows are the table's, in-between rows are solved ones: finite, unit-ish quaternions, near the straight line between their keyframes
    for k in range(n_gaps + 1):
        assert np.array_equal(rows[kf[k]], d["keyframe_poses"][k])
    assert np.all(np.isfinite(rows)) and np.abs(np.linalg.norm(rows[:, 3:7], axis=1) - 1).max() < 1e-3
    summ = traj.resolve_all(d["corrected"])
    again = traj.poses()
    assert cpp["resolves"] == [(s["termination"], s["iterations"]) for s in summ]
    assert cpp["resolved"].tobytes() == again.tobytes()
    for k in range(n_gaps + 1):
        assert np.array_equal(again[kf[k]], d["corrected"][k])
    assert not np.array_equal(again, rows)
    print("calls (n, gap, frames, termination, iterations):", calls)
    print("resolves:", cpp["resolves"])
    store.close(); graph.close()

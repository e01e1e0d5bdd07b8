"""GPU: the two hosts of place recognition -- glio::PlaceRecognition with its helpers (host/glio_place_backend.hpp, through host_demo_place) and
glio_amd.place -- agree bit for bit on one case: tilted keyframes levelled with leveling_quaternion, every place against the earlier ones, the appearance
rule and the initial guess."""
import math

import numpy as np
import pytest

import place_scenes as S

pytestmark = pytest.mark.gpu


def tilted(cloud, yaw, pitch, roll):
    """the cloud as a sensor with attitude R = Rz Ry Rx sees it (p_sensor = R^T p_level), and the attitude's quaternion"""
    from glio_amd import synth
    Rm = synth.euler_R(yaw, pitch, roll)
    out = cloud.copy()
    out[:, :3] = (cloud[:, :3].astype(np.float64) @ Rm).astype(np.float32)
    return out, synth.R2q(Rm)


def test_the_cpp_host_and_the_python_host_agree_bit_for_bit(tmp_path):
    from glio_amd import batch, capi, place
    from glio_amd.host import window_io
    g = S.kept()
    seeds = g["seeds"][:3]
    params = [S.parameters(s) for s in seeds]
    level_clouds = [S.place_scan(p) for p in params] + [S.revisit_scan(params[1])]
    att_euler = [(0.4, 0.03, -0.02), (-2.0, -0.05, 0.04), (1.1, 0.0, 0.06), (2.6, 0.04, 0.03)]
    clouds, att = zip(*[tilted(c, *e) for c, e in zip(level_clouds, att_euler)])
    K, cap, top_k, gap = len(clouds), max(len(c) for c in clouds), 3, 30.0
    times = [0.0, 50.0, 100.0, 1000.0]
    pose_closest = np.r_[params[1]["origin"], att[1]]
    opts = capi.place_opts(max_places=K, max_radius=g["max_radius"], lidar_height=g["lidar_height"])
    path = str(tmp_path / "place_case.bin")
    window_io.write_place_case(path, opts, cap, top_k, gap, clouds, times, att, pose_closest)
    cpp = window_io.run_demo_place(path)

    ba = batch.BatchAssociation(K, cap, 16)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    pr = place.PlaceRecognition(ba, opts)
    level = np.array([place.leveling_quaternion(q) for q in att])
    pr.add_frames(range(K), range(K), times, level)
    assert cpp["level"] == level.tobytes()
    for k in range(K):
        h, m, _, _ = pr.read_descriptor(k)
        assert cpp["heights%d" % k] == h.tobytes() and cpp["mask%d" % k] == m and m != 0
    many, nf = pr.query_many(0, K, gap, True, top_k)
    # (the demo's rows beyond n_found are zero, like query_many's)
    assert cpp["n_found"] == nf.tobytes() and cpp["many"] == many.tobytes() and list(nf) == [0, 1, 2, 3]
    one = pr.query(K - 1, gap, top_k)
    assert cpp["query"] == one.tobytes() and int(one[0]["place"]) == 1
    closest, yaw, dist = place.detect_candidate_by_appearance(pr, K - 1, gap, times[-1], -1.0)
    assert cpp["candidate"] == closest == 1 and cpp["candidate_yaw_distance"] == np.array([yaw, dist]).tobytes()
    guess = np.r_[place.initial_guess(pose_closest, yaw), place.initial_guess(pose_closest, yaw, q_query=att[K - 1])]
    assert cpp["guess"] == guess.tobytes()
    # the levelling took the tilt out: the heading found is the revisit's heading against the place's, to a sector
    want = (params[1]["yaw"] + att_euler[3][0] - att_euler[1][0]) % (2 * math.pi)
    assert S.angle_diff(yaw, want) < math.radians(9.0) and dist < g["distance_threshold"]
    pr.close(); ba.close()

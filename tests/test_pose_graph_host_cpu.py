"""CPU: the host's share of the pose graphs (glio_amd/posegraph.py: which frames enter the global graph at a keyframe call, Estimator.cpp:4589-4611; the loop
edge between frame ids, :5251-5252; every gate of addGNSSFactor, :1915-1997) on hand-made cases, and its C++ twin (glio_amd/host/glio_posegraph_backend.hpp,
through the host-only host_posegraph_mirror_test.cpp) answer for answer, the numbers bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from glio_amd import posegraph

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glio_amd", "host")
W = 5
FAR = (100.0, 0.0, 0.0)                  # a keyframe position more than 5 m from last_GNSS_add_pos = 0
OPEN = np.diag([0, 0, 0, 4.0, 4.0, 0])   # poseCovariance that opens the covariance gate


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pg_mirror") / "host_posegraph_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", os.path.join(HOST, "host_posegraph_mirror_test.cpp"), "-I" + os.path.join(HOST, "..", "..", "include"), "-o", exe])

    def run(lines):
        return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def hx(v):
    return float(v).hex()


# ------------------------------------------------------------------------------------------------------------------------------------ the global graph
KF = [0, 3, 6, 10, 11, 15, 22, 23, 30]           # keyframe_id_in_frame: keyframes every few frames, unevenly


def test_per_frame_insertion_indices(mirror):
    """Estimator.cpp:4589-4611: nothing before the window is full, frame 0 when it is, then the frames after the previous departed keyframe up to the one leaving now"""
    want = {1: [], 4: [], 5: [0], 6: [1, 2, 3], 7: [4, 5, 6], 8: [7, 8, 9, 10], 9: [11]}
    lines, got = [], {}
    for n, ids in want.items():
        got[n] = posegraph.global_graph_frames(KF, n, W)
        assert got[n] == ids, n
        lines.append(f"frames {n} {W} {len(KF)} " + " ".join(map(str, KF)))
    out = mirror(lines)
    for ln, n in zip(out, want):
        assert [int(x) for x in ln.split()[1:]] == want[n], (n, ln)
    # consecutive calls tile the frames without a gap or an overlap
    seen = [i for n in range(1, 10) for i in posegraph.global_graph_frames(KF, n, W)]
    assert seen == list(range(KF[9 - W] + 1))


def test_loop_edge_joins_frame_ids(mirror):
    assert posegraph.loop_edge_frames(KF, 8, 1) == (30, 3)
    assert mirror([f"edge 8 1 {len(KF)} " + " ".join(map(str, KF))]) == ["edge 30 3"]


def test_global_graph_feeds_a_graph_in_order():
    class Fake:
        def __init__(self):
            self.n, self.log = 0, []

        def size(self):
            return self.n

        def set_prior(self, p):
            self.log.append(("prior", tuple(p)))

        def append(self, poses, prev_pose=None):
            self.log.append(("append", self.n, len(poses), None if prev_pose is None else tuple(prev_pose)))
            self.n += len(poses)

    P = np.arange(31 * 7, dtype=float).reshape(31, 7)
    fake = Fake()
    gg = posegraph.GlobalGraph(fake, W)
    for n in range(1, 10):
        gg.keyframe_call(P[:KF[n - 1] + 1], KF, n)
    assert fake.log[0] == ("prior", tuple(P[0])) and fake.log[1] == ("append", 0, 1, None)
    assert fake.log[2:] == [("append", 1, 3, tuple(P[0])), ("append", 4, 3, tuple(P[3])), ("append", 7, 4, tuple(P[6])), ("append", 11, 1, tuple(P[10]))]


# ------------------------------------------------------------------------------------------------------------------------------------ addGNSSFactor's gates
def both(mirror, script):
    """script: ("gate", timeshift, gnss thr, pose thr) | ("push", stamp, xyz, cov) | ("select", n, W, xyz, time, pose_cov 6x6).  Runs it through the Python gate
    and the C++ one; returns the Python answers after checking that the C++ answers are the same, numbers bit for bit."""
    gate, lines, answers = posegraph.GnssGate(), [], []
    for s in script:
        if s[0] == "gate":
            gate = posegraph.GnssGate(*s[1:])
            lines.append("gate " + " ".join(hx(v) for v in s[1:]))
        elif s[0] == "push":
            gate.push(s[1], s[2], s[3])
            lines.append("push " + " ".join(hx(v) for v in (s[1], *s[2], *s[3])))
        else:
            _, n, w, xyz, t, pc = s
            answers.append((gate.select(n, w, xyz, t, pc), len(gate.queue)))
            pc = np.asarray(pc)
            lines.append(f"select {n} {w} " + " ".join(hx(v) for v in (*xyz, t, pc[3, 3], pc[4, 4])))
    out = mirror(lines)
    assert len(out) == len(answers)
    for ln, (a, queued) in zip(out, answers):
        w = ln.split()
        if a is None:
            assert w == ["none", str(queued)], (ln, a)
        else:
            assert w[0] == "gps" and int(w[1]) == a[0] and int(w[8]) == queued, (ln, a)
            assert [float.fromhex(x) for x in w[2:5]] == a[1] and [float.fromhex(x) for x in w[5:8]] == a[2], (ln, a)
    return [a for a, _ in answers]


FIX = ("push", 10.0, (50.123456789, 7.0, 1.0), (0.25, 3.0, 400.0))


def test_gate_passes_a_fix_and_applies_the_floor(mirror):
    (a,) = both(mirror, [FIX, ("select", 7, W, FAR, 10.1, OPEN)])
    f32 = lambda v: float(np.float32(v))
    assert a == (2, [f32(50.123456789), 7.0, 1.0], [1.0, 3.0, 400.0])        # node n - W; float positions; max(noise, 1) per axis (noise_z is not gated)


def test_gate_window_not_past_the_sliding_window(mirror):
    assert both(mirror, [FIX, ("select", 5, W, FAR, 10.0, OPEN), ("select", 4, W, FAR, 10.0, OPEN)]) == [None, None]


def test_gate_empty_queue(mirror):
    assert both(mirror, [("select", 7, W, FAR, 10.0, OPEN)]) == [None]


def test_gate_spacing_to_the_last_added_position(mirror):
    """:1932 and :1992: 5 m from where the last factor was added (initially the origin), measured in double"""
    near, edge = (3.0, 3.9, 0.0), (3.0, 4.0, 0.0)          # 4.92 m and exactly 5 m from the origin
    second = ("push", 20.0, (70.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    third = ("push", 30.0, (90.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    a = both(mirror, [FIX, ("select", 7, W, near, 10.0, OPEN), ("select", 7, W, edge, 10.0, OPEN),
                      second, ("select", 8, W, (3.0, 8.9, 0.0), 20.0, OPEN),            # 4.9 m from the last added position
                      third, ("select", 9, W, (3.0, 9.0, 0.0), 30.0, OPEN)])            # 5 m: second is dropped as too old on the way, third is taken
    assert a[0] is None and a[1] is not None and a[2] is None and a[3] is not None and a[3][1][0] == 90.0


def test_gate_covariance_threshold(mirror):
    """:1938: closed only when BOTH (3,3) and (4,4) are below the threshold"""
    low, x_only, y_only = np.diag([9, 9, 9, 0.5, 0.99, 9.0]), np.diag([0, 0, 0, 1.0, 0.2, 0]), np.diag([0, 0, 0, 0.2, 1.0, 0])
    assert both(mirror, [FIX, ("select", 7, W, FAR, 10.0, low)]) == [None]
    assert both(mirror, [FIX, ("select", 7, W, FAR, 10.0, x_only)])[0] is not None
    assert both(mirror, [FIX, ("select", 7, W, FAR, 10.0, y_only)])[0] is not None
    assert both(mirror, [("gate", 0.0, 200.0, 0.1), FIX, ("select", 7, W, FAR, 10.0, low)])[0] is not None


def test_gate_time_window_and_timeshift(mirror):
    """:1946-1957: fixes older than t - 0.2 are dropped, one newer than t + 0.2 stops the search and stays queued; t = keyframe time + timeshift"""
    fix = lambda t, x=50.0: ("push", t, (x, 0.0, 0.0), (1.0, 1.0, 1.0))
    a = both(mirror, [fix(9.0), fix(9.79), fix(10.21), ("select", 7, W, FAR, 10.0, OPEN)])
    assert a == [None]
    gate = posegraph.GnssGate()
    for t in (9.0, 9.79, 10.21):
        gate.push(t, (50.0, 0, 0), (1, 1, 1))
    assert gate.select(7, W, FAR, 10.0, OPEN) is None and [q[0] for q in gate.queue] == [10.21]
    a = both(mirror, [fix(9.81), ("select", 7, W, FAR, 10.0, OPEN)])
    assert a[0] is not None
    a = both(mirror, [("gate", 0.5, 200.0, 1.0), fix(10.0), ("select", 7, W, FAR, 10.0, OPEN), fix(10.6, 80.0), ("select", 7, W, FAR, 10.0, OPEN)])
    assert a[0] is None and a[1] is not None and a[1][1][0] == 80.0


def test_gate_noisy_fix_is_skipped_and_the_next_one_taken(mirror):
    """:1967: noise_x or noise_y above gnssCovThreshold skips the fix (noise_z does not); the loop goes on inside the window"""
    a = both(mirror, [("push", 10.0, (50.0, 0, 0), (201.0, 1.0, 1.0)), ("push", 10.05, (51.0, 0, 0), (1.0, 200.5, 1.0)),
                      ("push", 10.1, (52.0, 0, 0), (200.0, 200.0, 9999.0)), ("select", 7, W, FAR, 10.0, OPEN)])
    assert a[0] == (2, [52.0, 0.0, 0.0], [200.0, 200.0, 9999.0])


def test_gate_spacing_to_the_last_gps_point(mirror):
    """:1980: a fix closer than 5 m (float arithmetic) to the last GPS point that passed this test is skipped; the point is remembered even across calls"""
    a = both(mirror, [("push", 10.0, (3.0, 3.9, 0.0), (1, 1, 1)), ("push", 10.1, (3.0, 4.0, 0.0), (1, 1, 1)), ("select", 7, W, FAR, 10.0, OPEN),
                      ("push", 20.0, (3.0, 8.9, 0.0), (1, 1, 1)), ("push", 20.1, (3.0, 9.0, 0.0), (1, 1, 1)), ("select", 8, W, (200.0, 0, 0), 20.0, OPEN)])
    assert a[0][1] == [3.0, 4.0, 0.0] and a[1][1] == [3.0, 9.0, 0.0]


def test_distances_bit_for_bit(mirror):
    rng = np.random.default_rng(2)
    lines, want = [], []
    for _ in range(40):
        a, b = rng.normal(0, 30, 3), rng.normal(0, 30, 3)
        lines.append("dist32 " + " ".join(hx(np.float32(v)) for v in (*a, *b))); want.append(posegraph.point_distance_f32(a, b))
        lines.append("dist64 " + " ".join(hx(v) for v in (*a, *b))); want.append(posegraph.point_distance_f64(a, b))
    got = [float.fromhex(ln.split()[1]) for ln in mirror(lines)]
    assert got == want

"""The host's share of the local map's schedule and of correctPoses: sliding.local_map_plan (buildLocalMapWithLandMark's bookkeeping, Estimator.cpp:3545-3610,
with quirk Q17: after a loop closure the deque refills with local_map_width - 1 clouds and every later call rebuilds) and loop.correct_window_poses (the
sliding window's share of correctPoses, :4664-4686, :4702-4773) on hand cases, and their C++ twins (glio::localMapPlan in glio_backend.hpp,
glio::correctWindowPoses in glio_loop_backend.hpp, through the host-only host_map_schedule_mirror_test.cpp) bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

from glio_amd import loop, sliding, synth
from glio_amd.sliding import MAP_NOTHING, MAP_PUSH, MAP_REBUILD


def test_local_map_plan_warm_up():
    # one keyframe: the map is that keyframe, at its current pose
    assert sliding.local_map_plan(0, 1, 50, -1) == (MAP_REBUILD, [0], 1, -1)
    # until local_map_width keyframes exist EVERY call rebuilds the whole map (the deque stays below the width), latest_frame_idx untouched
    assert sliding.local_map_plan(48, 49, 50, -1) == (MAP_REBUILD, list(range(49)), 49, -1)
    # the call that finds exactly local_map_width keyframes takes all of them ...
    assert sliding.local_map_plan(49, 50, 50, -1) == (MAP_REBUILD, list(range(50)), 50, -1)
    # ... and the next one pushes: the oldest leaves, the newest enters, latest_frame_idx is set
    assert sliding.local_map_plan(50, 51, 50, -1) == (MAP_PUSH, [50], 50, 50)
    assert sliding.local_map_plan(50, 51, 50, 50) == (MAP_NOTHING, [], 50, 50)            # no new keyframe since
    assert sliding.local_map_plan(50, 52, 50, 50) == (MAP_PUSH, [51], 50, 51)
    assert sliding.local_map_plan(0, 0, 50, -1) == (MAP_NOTHING, [], 0, -1)               # no keyframe yet (:3531)
    # a full deque whose latest_frame_idx was never set (the rebuild branch does not set it) pushes the newest keyframe even when it is in the deque already
    assert sliding.local_map_plan(50, 50, 50, -1) == (MAP_PUSH, [49], 50, 49)


def test_local_map_plan_after_a_loop_closure_rebuilds_for_good():
    # correctPoses cleared the deque at 60 keyframes: the guard `i <= size - local_map_width` stops the loop at i = 10 -> frames 11..59, 49 of them
    action, frames, recent, latest = sliding.local_map_plan(0, 60, 50, 59)
    assert action == MAP_REBUILD and frames == list(range(11, 60)) and len(frames) == 49 and recent == 49 and latest == 59
    # 49 < 50: the next keyframe call rebuilds again (12..60), and so on for good
    action, frames, recent, latest = sliding.local_map_plan(recent, 61, 50, latest)
    assert action == MAP_REBUILD and frames == list(range(12, 61)) and recent == 49 and latest == 59
    for n in range(62, 70):
        action, frames, recent, latest = sliding.local_map_plan(recent, n, 50, latest)
        assert action == MAP_REBUILD and frames == list(range(n - 49, n))
    # cleared with exactly local_map_width keyframes: all of them, then pushes
    assert sliding.local_map_plan(0, 50, 50, 49) == (MAP_REBUILD, list(range(50)), 50, 49)
    assert sliding.local_map_plan(0, 51, 50, 50)[1] == list(range(2, 51))
    # small widths: width 4 with 6 keyframes takes 3 (= width - 1)
    assert sliding.local_map_plan(0, 6, 4, 5) == (MAP_REBUILD, [3, 4, 5], 3, 5)
    assert sliding.local_map_plan(0, 4, 4, 3) == (MAP_REBUILD, [0, 1, 2, 3], 4, 3)
    # width 1 with more than one keyframe: the guard leaves NOTHING (recent stays 0, the map would be empty), as the reference's loop does
    assert sliding.local_map_plan(0, 3, 1, 2) == (MAP_REBUILD, [], 0, 2)


def _random_abs_poses(rng, N):
    a = np.zeros((N, 7))
    for i in range(N):
        a[i, :4] = synth.rotvec_q(rng.uniform(-1, 1, 3))          # (unit to rounding: Eigen's q * v, which chains the window back on, assumes a unit quaternion)
        a[i, 4:] = rng.uniform(-40, 40, 3)
    return a


def _relative(a, i):
    """pose i^-1 * pose i + 1 of abs_poses rows (q, t) as (R, t), with numpy"""
    Ri, Rj = synth.q2R(a[i, :4] / np.linalg.norm(a[i, :4])), synth.q2R(a[i + 1, :4] / np.linalg.norm(a[i + 1, :4]))
    return Ri.T @ Rj, Ri.T @ (a[i + 1, 4:] - a[i, 4:])


def test_correct_window_poses_identity_and_rigid_shift():
    rng = np.random.default_rng(3)
    N, W = 9, 4
    a = _random_abs_poses(rng, N)
    # identity correction: the keyframes up to the window's oldest keep their poses -> everything is preserved
    out, Rs, Ps = loop.correct_window_poses(a, a[1:N - W + 1], W)
    assert np.abs(out - a).max() < 1e-12
    for i in range(1, N):
        assert np.abs(Rs[i].reshape(3, 3) - synth.q2R(a[i, :4])).max() < 1e-8 and np.array_equal(Ps[i], out[i, 4:])
    assert not Rs[0].any() and not Ps[0].any()
    # a rigid shift of everything up to the anchor (the window's oldest keyframe, row N - W): the window follows rigidly, relative poses preserved
    qs, ts = synth.rotvec_q(np.array([0.1, -0.2, 0.7])), np.array([3.0, -2.0, 0.5])
    Rsft = synth.q2R(qs)
    c = a[1:N - W + 1].copy()
    for k in range(len(c)):
        c[k, :4] = synth.qmul(qs, c[k, :4]); c[k, 4:] = Rsft @ c[k, 4:] + ts
    out, Rs, Ps = loop.correct_window_poses(a, c, W)
    assert np.array_equal(out[0], a[0]) and np.array_equal(out[1:N - W + 1], c)
    for i in range(N - W, N - 1):
        R0, t0 = _relative(a, i)
        R1, t1 = _relative(out, i)
        assert np.abs(R0 - R1).max() < 1e-12 and np.abs(t0 - t1).max() < 1e-12
    for i in range(N - W + 1, N):
        assert np.abs(out[i, 4:] - (Rsft @ a[i, 4:] + ts)).max() < 1e-12
        assert np.abs(synth.q2R(out[i, :4]) - Rsft @ synth.q2R(a[i, :4])).max() < 1e-9
    with pytest.raises(ValueError):
        loop.correct_window_poses(a, c[:-1], W)


def test_correct_window_poses_by_hand_90_degree_yaw():
    # three rows, window of 2: row 1 (keyframe 0, the window's oldest) at the origin looking along x, row 2 one metre ahead of it with a 90 degree yaw of its own
    h = math.sqrt(0.5)
    a = np.array([[1, 0, 0, 0, 0, 0, 0],
                  [1, 0, 0, 0, 0, 0, 0],
                  [h, 0, 0, h, 1, 0, 0]], float)
    # the pose graph turns keyframe 0 by 90 degrees about z and moves it to (10, 20, 0)
    c = np.array([[h, 0, 0, h, 10, 20, 0]], float)
    out, Rs, Ps = loop.correct_window_poses(a, c, 2)
    assert np.array_equal(out[1], c[0])
    # "one metre ahead" now points along y; the two yaws add up to 180 degrees: q = (h, 0, 0, h)^2 = (0, 0, 0, 1)
    assert np.abs(out[2, 4:] - [10, 21, 0]).max() < 1e-15
    assert np.abs(out[2, :4] - [0, 0, 0, 1]).max() < 1e-15
    assert np.abs(Rs[2].reshape(3, 3) - np.diag([-1.0, -1.0, 1.0])).max() < 1e-15 and np.array_equal(Ps[2], out[2, 4:])
    assert np.abs(Rs[1].reshape(3, 3) - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], float)).max() < 1e-15


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(loop.__file__)), "host")
    exe = str(tmp_path_factory.mktemp("map_schedule_mirror") / "host_map_schedule_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", os.path.join(here, "host_map_schedule_mirror_test.cpp"), "-I" + os.path.join(here, "..", "..", "include"), "-o", exe])

    def run(lines):
        return subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def test_cpp_twins_agree_bit_for_bit(mirror):
    # the plan over a sweep of every state a stream can reach, small widths and the released one
    cases = [(r, n, w, lat) for w in (1, 2, 4, 50) for n in list(range(0, 9)) + [49, 50, 51, 60, 61] for r in sorted({0, 1, w - 1, w}) for lat in (-1, n - 2, n - 1)]
    out = mirror(["plan %d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    for c, ln in zip(cases, out):
        w = [int(x) for x in ln.split()[1:]]
        action, frames, recent, latest = sliding.local_map_plan(*c)
        assert w[:4] == [action, recent, latest, len(frames)] and w[4:] == frames, c
    # a whole stream with a loop closure, state carried along: both sides walk through the same plans
    recent, latest, lines, want = 0, -1, [], []
    for n in range(1, 14):
        lines.append("plan %d %d 4 %d" % (recent, n, latest))
        action, frames, recent, latest = sliding.local_map_plan(recent, n, 4, latest)
        want.append([action, recent, latest, len(frames)] + frames)
        if n == 9:
            recent = 0                                         # correctPoses
    assert [[int(x) for x in ln.split()[1:]] for ln in mirror(lines)] == want
    assert [w[0] for w in want] == [MAP_REBUILD] * 4 + [MAP_PUSH] * 5 + [MAP_REBUILD] * 4 and want[-1][4:] == [10, 11, 12]
    # correctPoses' window share
    rng = np.random.default_rng(5)
    for N, W in ((9, 4), (6, 1), (7, 7), (12, 5), (3, 2)):
        a = _random_abs_poses(rng, N)
        c = _random_abs_poses(rng, N - W)
        out = mirror(["correct %d %d " % (N, W) + " ".join(repr(float(x)) for x in np.r_[a.ravel(), c.ravel()])])
        assert out[0] == "ok 1"
        got = np.array([[float.fromhex(x) for x in ln.split()[1:]] for ln in out[1:]])
        want_a, want_R, want_P = loop.correct_window_poses(a, c, W)
        assert np.array_equal(got[:, :7], want_a) and np.array_equal(got[:, 7:16], want_R) and np.array_equal(got[:, 16:], want_P), (N, W)
    assert mirror(["correct 5 6 " + " ".join(["0.0"] * 35)])[0] == "ok 0"

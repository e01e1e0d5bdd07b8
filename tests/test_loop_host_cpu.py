"""The host's share of the loop thread (glio_amd/loop.py: detect_candidate, submap_frames, frame_poses, loop_constraint; Estimator.cpp:5113-5175,
:5210-5247) on hand cases, and its C++ twin (glio_amd/host/glio_loop_backend.hpp, through the host-only host_loop_mirror_test.cpp) bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

from glio_amd import loop, synth
from glio_amd import ctypes_types as T


def _result(transform=None, converged=True, fitness=0.01):
    s = T.GlioLoopResult()
    s.converged, s.fitness, s.state, s.iterations = int(converged), fitness, T.LOOP_TRANSFORM, 5
    for k, v in enumerate(np.asarray(np.eye(4) if transform is None else transform, np.float32).ravel()):
        s.transform[k] = float(v)
    return loop.LoopResult(s)


def test_detect_candidate():
    pos = np.array([[0, 0, 0], [3, 0, 0], [1, 0, 0], [0, 1, 0], [10, 0, 0], [0.5, 0, 0]], np.float32)
    times = np.array([0.0, 5.0, 50.0, 60.0, 0.0, 99.0])
    sel = np.zeros(3, np.float32)
    # within 7 m: 0, 5, 2, 3 (tie at d2 = 1: index 2 before 3), 1; the first older than 30 s counted from t = 100: keyframe 0 (the nearest)
    assert loop.detect_candidate(pos, times, sel, 100.0, 0.0, 7.0, 30.0) == 0
    # keyframe 0 too recent: 5 (99 s) is recent too, then the tie 2 / 3 -> the lower index
    times2 = times.copy(); times2[0] = 95.0
    assert loop.detect_candidate(pos, times2, sel, 100.0, 0.0, 7.0, 30.0) == 2
    times2[2] = 95.0
    assert loop.detect_candidate(pos, times2, sel, 100.0, 0.0, 7.0, 30.0) == 3
    # the radius is strict, squared, in double: keyframe 1 at exactly 3 m is outside a 3 m radius
    only = np.array([100.0, 0.0, 100.0, 100.0, 0.0, 100.0])
    assert loop.detect_candidate(pos, only, sel, 100.0, 0.0, 3.0, 30.0) == -1
    assert loop.detect_candidate(pos, only, sel, 100.0, 0.0, 3.0001, 30.0) == 1
    # nobody old enough
    assert loop.detect_candidate(pos, np.full(6, 90.0), sel, 100.0, 0.0, 7.0, 30.0) == -1
    # the 0.2 s gate on the last closed loop (:5127): strict
    assert loop.detect_candidate(pos, times, sel, 100.0, 99.9, 7.0, 30.0) == -1
    assert loop.detect_candidate(pos, times, sel, 100.0, 100.1, 7.0, 30.0) == -1
    assert loop.detect_candidate(pos, times, sel, 100.0, 99.75, 7.0, 30.0) == 0
    # no keyframe at all
    assert loop.detect_candidate(np.zeros((0, 3), np.float32), np.zeros(0), sel, 1.0, 0.0, 7.0, 30.0) == -1


def test_submap_frames():
    latest, src, tgt = loop.submap_frames(100, 5, 40, 25)
    assert latest == 95 and src == [95, 94, 93, 92, 91, 90] and tgt == list(range(15, 66)) and len(tgt) == 51
    # latest - j < 0: the young map
    latest, src, tgt = loop.submap_frames(8, 5, 1, 25)
    assert latest == 3 and src == [3, 2, 1, 0] and tgt == [0, 1, 2, 3]
    # closest + j > latest and closest + j < 0 are skipped
    latest, src, tgt = loop.submap_frames(60, 5, 50, 25)
    assert latest == 55 and tgt == list(range(25, 56))
    latest, src, tgt = loop.submap_frames(60, 5, 3, 25)
    assert tgt == list(range(0, 29))
    latest, src, tgt = loop.submap_frames(4, 5, 0, 25)
    assert latest == -1 and src == [] and tgt == []


def test_frame_poses():
    q_po, t_po = synth.rotvec_q(np.array([0.1, -0.2, 0.7])), np.array([3.0, -2.0, 1.0])
    q_bl, t_bl = synth.rotvec_q(np.array([0.02, 0.01, -0.03])), np.array([0.1, 0.2, 0.3])
    out = loop.frame_poses([np.r_[t_po, q_po]], q_bl, t_bl)
    assert out.shape == (1, 7)
    assert np.allclose(out[0, 3:], synth.qmul(q_po, q_bl), atol=1e-15)
    assert np.allclose(out[0, :3], synth.q2R(q_po) @ t_bl + t_po, atol=1e-14)
    ident = loop.frame_poses([np.r_[t_po, q_po]], [1, 0, 0, 0], [0, 0, 0])
    assert np.array_equal(ident[0], np.r_[t_po, q_po])


def test_eigen_R2q_is_eigens_rule():
    for v in ([0.1, -0.2, 0.3], [3.0, 0.1, 0.0], [0.0, 3.1, 0.2], [0.1, 0.0, -3.0], [0, 0, 0]):
        q = synth.rotvec_q(np.array(v, float))
        R = synth.q2R(q)
        e = np.array(loop.eigen_R2q(R))
        assert abs(np.linalg.norm(e) - 1.0) < 1e-12
        assert np.allclose(synth.q2R(e), R, atol=1e-12)
        s = synth.R2q(R)                       # the in-tree restatement: the same rule, then w >= 0 and a normalisation
        assert np.allclose(s, e if e[0] >= 0 else -e, atol=1e-12)


def test_loop_constraint():
    pl = np.r_[1.0, 2.0, 0.5, synth.rotvec_q(np.array([0.0, 0.1, 0.4]))]
    pc = np.r_[1.5, 1.0, 0.4, synth.rotvec_q(np.array([0.05, 0.0, -0.2]))]
    # an identity ICP result gives between(pose_latest, pose_closest)
    rel, var = loop.loop_constraint(_result(), pl, pc, 0.3)
    Rl, Rc = synth.q2R(pl[3:]), synth.q2R(pc[3:])
    assert np.allclose(rel[:3], Rl.T @ (pc[:3] - pl[:3]), atol=1e-14)
    assert np.allclose(synth.q2R(rel[3:]), Rl.T @ Rc, atol=1e-14)
    assert np.array_equal(var, np.full(6, 0.01))
    # the gate (:5210): not converged, or fitness above lc_icp_thres
    assert loop.loop_constraint(_result(converged=False), pl, pc, 0.3) is None
    assert loop.loop_constraint(_result(fitness=0.31), pl, pc, 0.3) is None
    assert loop.loop_constraint(_result(fitness=0.3), pl, pc, 0.3) is not None
    # a correction: poseFrom = T_icp * pose_latest
    M = np.eye(4); M[:3, :3] = synth.euler_R(0.02, -0.01, 0.005); M[:3, 3] = [0.3, -0.1, 0.05]
    rel, _ = loop.loop_constraint(_result(M), pl, pc, 0.3)
    M32 = M.astype(np.float32).astype(np.float64)
    Rf, tf = M32[:3, :3] @ Rl, M32[:3, :3] @ pl[:3] + M32[:3, 3]
    assert np.allclose(rel[:3], Rf.T @ (pc[:3] - tf), atol=1e-6)
    assert np.allclose(synth.q2R(rel[3:]), Rf.T @ Rc, atol=1e-6)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    here = os.path.join(os.path.dirname(os.path.abspath(loop.__file__)), "host")
    exe = str(tmp_path_factory.mktemp("loop_mirror") / "host_loop_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", os.path.join(here, "host_loop_mirror_test.cpp"), "-I" + os.path.join(here, "..", "..", "include"), "-o", exe])

    def run(cmd, *numbers):
        text = cmd + " " + " ".join(repr(float(x)) for x in numbers) + "\n"
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def test_cpp_header_agrees_bit_for_bit(mirror):
    rng = np.random.default_rng(7)
    # detect: random keyframes around the query, exact ties included
    for trial in range(6):
        n = 40
        pos = rng.uniform(-9, 9, (n, 3)).astype(np.float32)
        pos[5] = pos[11]; pos[20, :] = [1, 2, 2]; pos[21, :] = [2, 1, 2]; pos[22, :] = [2, 2, 1]
        times = rng.uniform(0, 100, n)
        sel = np.zeros(3, np.float32) if trial % 2 else rng.uniform(-1, 1, 3).astype(np.float32)
        t_new, t_last = 100.0, (99.9 if trial == 4 else 10.0)
        want = loop.detect_candidate(pos, times, sel, t_new, t_last, 7.0, 30.0 + 10 * trial)
        out = mirror("detect", n, 7.0, 30.0 + 10 * trial, t_new, t_last, *sel, *np.c_[pos.astype(np.float64), times].ravel())
        assert int(out[0].split()[1]) == want
    # frames
    for args in ((100, 5, 40, 25), (8, 5, 1, 25), (60, 5, 50, 25), (60, 5, 3, 25), (4, 5, 0, 25)):
        out = mirror("frames", *args)
        latest, src, tgt = loop.submap_frames(*args)
        assert int(out[0].split()[1]) == latest and [int(x) for x in out[1].split()[1:]] == src and [int(x) for x in out[2].split()[1:]] == tgt
    # poses
    info = np.array([np.r_[rng.uniform(-50, 50, 3), synth.rotvec_q(rng.uniform(-1, 1, 3))] for _ in range(9)])
    q_bl, t_bl = synth.rotvec_q(np.array([0.02, 0.01, -0.03])), np.array([0.1, 0.2, 0.3])
    out = mirror("poses", len(info), *q_bl, *t_bl, *info.ravel())
    got = np.array([[float.fromhex(x) for x in ln.split()[1:]] for ln in out])
    assert np.array_equal(got, loop.frame_poses(info, q_bl, t_bl))
    # constraint: a rotation with positive trace, one with negative trace (the other branch of Eigen's rule), the gate
    for v, conv, fit in (([0.02, -0.01, 0.03], 1, 0.01), ([3.0, 0.2, -0.1], 1, 0.2), ([0.1, 3.0, 0.3], 1, 0.05), ([0.2, -0.1, 3.1], 1, 0.05), ([0.02, 0, 0], 0, 0.01), ([0.02, 0, 0], 1, 0.4)):
        M = np.eye(4); M[:3, :3] = synth.q2R(synth.rotvec_q(np.array(v, float))); M[:3, 3] = rng.uniform(-1, 1, 3)
        M32 = M.astype(np.float32)
        pl, pc = info[0], info[1]
        want = loop.loop_constraint(_result(M32, bool(conv), fit), pl, pc, 0.3)
        out = mirror("constraint", conv, fit, 0.3, *M32.astype(np.float64).ravel(), *pl, *pc)
        if want is None:
            assert out[0] == "ok 0"
        else:
            assert out[0] == "ok 1"
            assert np.array_equal(np.array([float.fromhex(x) for x in out[1].split()[1:]]), want[0])
            assert np.array_equal(np.array([float.fromhex(x) for x in out[2].split()[1:]]), want[1])
            assert math.isclose(np.linalg.norm(want[0][3:]), 1.0, abs_tol=1e-12)

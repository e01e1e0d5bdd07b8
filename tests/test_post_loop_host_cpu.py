"""The arm / install / disarm sequence of the speed-bias priors in both hosts, call for call and bit for bit: glio::SlidingWindowBackend over a recording
stand-in for the C-ABI (glio_amd/host/host_post_loop_mirror_test.cpp, host-only) against sliding.SlidingWindowDriver / sliding.ResidentSlidingWindow over
a recording backend.  Both stand-ins "solve" by the same exact steps (speed/bias += 1/8, translation += 1/4), so the logs show which values were installed.
The C++ program also runs once under -fsanitize=address,undefined (it sizes the marginalization's buffers from glio_marginalize_size)."""
import os
import subprocess

import numpy as np
import pytest

from glio_amd import ctypes_types as T
from glio_amd import sliding
from glio_amd import synth

HOST = os.path.join(os.path.dirname(os.path.abspath(sliding.__file__)), "host")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall"] + flags + [os.path.join(HOST, "host_post_loop_mirror_test.cpp"), "-I" + os.path.join(HOST, "..", "..", "include"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("post_loop_mirror")
    exes = {"plain": _build(tmp, "mirror", []), "sanitized": _build(tmp, "mirror_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])}

    def run(W, commands, which="plain"):
        r = subprocess.run([exes[which], str(W)], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-800:]
        return r.stdout.splitlines()
    return run


def parse(lines):
    """log lines -> (name, ints / floats): hex floats compare as the doubles they are"""
    out = []
    for ln in lines:
        w = ln.split()
        out.append((w[0],) + tuple(float.fromhex(x) if "x" in x else int(x) for x in w[1:]))
    return out


class Recorder:
    """the methods of capi.Context the drivers call; the ones under test are logged"""

    def __init__(self, W):
        self.W, self.log, self.sbp = W, [], 0

    def _quiet(self, *a, **k):
        return None

    set_map = set_correspondences = set_imu = set_prior = set_gnss = set_scan = slide_window = _quiet

    def set_speed_bias_priors(self, targets):
        t = np.zeros((0, 9)) if targets is None else np.asarray(targets, float).reshape(-1, 9)
        self.log.append(("set_speed_bias_priors", len(t)) + tuple(t.ravel().tolist()))
        self.sbp = len(t)

    def solve(self, state):
        self.log.append(("solve",))
        s = state.copy()
        s.speed_bias += 0.125; s.trans += 0.25
        return s, None

    def _size(self):
        ne = max(self.sbp - 2, 0)
        return 6 * (self.W - 1) + 9 + 9 * ne, 2 * (self.W - 1) + 1 + ne

    def marginalize(self, state):
        n, nb = self._size()
        self.log.append(("marginalize_size", n, nb)); self.log.append(("marginalize", float(state.speed_bias[0, 0])))
        return dict(n=n, blk_slot=np.zeros(nb, np.int32))

    def marginalize_keep(self, state):
        self.log.append(("marginalize_keep", float(state.speed_bias[0, 0])))
        self.sbp = 0


def start_state(W):
    st = T.WindowState(W)
    st.speed_bias[:] = (0.5 * np.arange(9 * W) - 3.0).reshape(W, 9)
    return st


def drive(driver, be, steps, closing, prior_line):
    """`steps` keyframe calls without sliding (the C++ program does not slide either); the loop closes before the calls listed in `closing`"""
    log = []
    opts = synth.default_opts(W=be.W)
    d = driver(be, opts)
    d.start(start_state(be.W))
    empty = np.zeros((0, 4), np.float32)
    for k in range(steps):
        if k in closing:
            d.arm_speed_bias_priors()
            log.append(("armed", 1))
        before = int(d.speed_bias_priors_armed)
        n0 = len(be.log)
        d.step(empty, [empty] * be.W, [])
        new = be.log[n0:]
        i = new.index(("solve",))
        log += new[:i + 1] + [("armed", before)] + new[i + 1:]
        if prior_line:
            log.append(("prior",) + be._size_after)
        log.append(("armed", int(d.speed_bias_priors_armed)))
    return log


@pytest.mark.parametrize("W", [2, 3, 5])
def test_driver_with_readback_equals_cpp(mirror, W):
    class Rec(Recorder):
        def marginalize(self, state):
            self._size_after = self._size()
            return super().marginalize(state)
    be = Rec(W)
    want = drive(sliding.SlidingWindowDriver, be, 4, {1, 3}, True)
    cmds = []
    for k in range(4):
        cmds += (["arm"] if k in (1, 3) else []) + ["solve", "marginalize"]
    for which in ("plain", "sanitized"):
        assert parse(mirror(W, cmds, which)) == want


@pytest.mark.parametrize("W", [2, 4])
def test_resident_driver_equals_cpp(mirror, W):
    be = Recorder(W)
    want = drive(sliding.ResidentSlidingWindow, be, 3, {1}, False)
    cmds = ["solve", "keep", "arm", "solve", "keep", "solve", "keep"]
    assert parse(mirror(W, cmds)) == want
    # the two-halves form disarms like the one-call form
    got = parse(mirror(W, ["arm", "solve", "keep_async", "finish"], "sanitized"))
    assert got[-4:] == [("marginalize_keep_async", got[-4][1]), ("armed", 0), ("marginalize_keep_finish",), ("armed", 0)]
    assert got[1][0] == "set_speed_bias_priors" and got[1][1] == W - 1


def test_the_sequence_is_the_references(mirror):
    """armed: the factors are installed from the speed/bias as they stand BEFORE the solve, on slots 0 .. W-2; the marginalization sees the solved state, the
    context is cleared after a read-back marginalization, and the next window installs nothing"""
    W = 4
    log = parse(mirror(W, ["arm", "solve", "marginalize", "solve", "marginalize"]))
    names = [l[0] for l in log if l[0] != "armed"]
    assert names == ["set_speed_bias_priors", "solve", "marginalize_size", "marginalize", "set_speed_bias_priors", "prior", "solve", "marginalize_size", "marginalize", "prior"]
    inst = next(l for l in log if l[0] == "set_speed_bias_priors")
    assert inst[1] == W - 1 and inst[2:] == tuple((0.5 * np.arange(9 * (W - 1)) - 3.0).tolist())
    assert [l for l in log if l[0] == "marginalize"][0][1] == -3.0 + 0.125
    assert [l for l in log if l[0] == "set_speed_bias_priors"][1][1] == 0
    assert [l[1:] for l in log if l[0] == "prior"] == [(36, 8), (27, 7)]

"""CPU checks of the keyframe cloud's boundary: the new symbols are exported with the argument types include/glio_hip.h documents (and the ctypes
prototypes say the same), and the keyframe rule (LidarOdometry.cpp:566-578) is the same in C++ (glio::KeyframeGate, a stand-alone program), in Python
(odometry.KeyframeGate), in the tests' own restatement and in a hand-made 12-frame sequence."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keyframe_cloud_restated as kr  # noqa: E402

from glio_amd import ctypes_types as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glio_scan_filter_config", "glio_set_scan_filtered_strided", "glio_set_scan_filtered", "glio_set_scan_filtered_ahead_strided",
         "glio_set_scan_filtered_ahead", "glio_set_scan_from_features", "glio_set_scan_from_features_ahead", "glio_get_scan"]


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "glio_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/glio_hip.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        ptr = "*" in a or "[" in a
        if "glio_ctx" in a or ("void" in a and ptr):
            out.append(C.c_void_p)
        elif "double" in a:
            assert ptr
            out.append(T.c_double_p)
        elif "float" in a:
            out.append(T.c_float_p if ptr else C.c_float)
        else:
            assert re.match(r"(const )?int\b", a), a
            out.append(T.c_int_p if ptr else C.c_int)
    return out


def test_symbols_exist_with_the_documented_argument_types():
    from glio_amd import build, capi
    build.build()
    lib = capi.load()
    for n in NAMES + ["glio_scan_filter_last_device_ms"]:
        assert hasattr(lib, n), n
        assert T.KEYFRAME_CLOUD_PROTOTYPES[n] == _header_args(n), n
        assert getattr(lib, n).argtypes == T.KEYFRAME_CLOUD_PROTOTYPES[n] and getattr(lib, n).restype is C.c_int
    # the documented shapes, spelled out once
    assert T.KEYFRAME_CLOUD_PROTOTYPES["glio_set_scan_filtered_strided"] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, T.c_double_p,
                                                                              T.c_double_p, T.c_int_p]
    assert T.KEYFRAME_CLOUD_PROTOTYPES["glio_set_scan_from_features"] == [C.c_void_p, C.c_int, C.c_void_p, C.c_float, T.c_double_p, T.c_double_p, T.c_int_p]
    assert T.KEYFRAME_CLOUD_PROTOTYPES["glio_get_scan"] == [C.c_void_p, C.c_int, T.c_float_p, C.c_int, T.c_int_p]
    # the Python surface
    for m in ("scan_filter_config", "set_scan_filtered", "set_scan_from_features", "get_scan"):
        assert callable(getattr(capi.Context, m)), m
    # null contexts are refused, not dereferenced -- and without a device nothing else can be asked
    n = C.c_int(-7)
    assert lib.glio_scan_filter_config(None, 10) == capi.E_ARG
    assert lib.glio_set_scan_filtered(None, 0, None, 0, 0.9, None, None, C.byref(n)) == capi.E_ARG
    assert lib.glio_set_scan_from_features(None, 0, None, 0.9, None, None, C.byref(n)) == capi.E_ARG
    assert lib.glio_get_scan(None, 0, None, 0, C.byref(n)) == capi.E_ARG


def _yaw(a, scale=1.0):
    return (scale * math.cos(a / 2), 0.0, 0.0, scale * math.sin(a / 2))


ID = (1.0, 0.0, 0.0, 0.0)
Y = _yaw(0.15)
# (size, q, t, expected): size = the scans saved before the one judged
HAND_MADE = [
    (1, ID, (0.0, 0.0, 0.0), True),                 # the first frame: size <= 1
    (2, ID, (0.5, 0.0, 0.0), False),                # moved, but too soon (size - kf_num = 0)
    (3, ID, (1.0, 0.0, 0.0), False),                # moved, still too soon (1)
    (4, ID, (1.5, 0.0, 0.0), True),                 # moved and two frames on: dis > 0.2
    (5, ID, (1.5, 0.0, 0.0), False),
    (6, ID, (1.5, 0.1, 0.0), False),                # 0.1 m: not moved
    (7, Y, (1.5, 0.0, 0.0), True),                  # turned by 0.15 rad and two frames on: ang > 0.1
    (8, Y, (1.5, 0.0, 0.0), False),
    (9, Y, (1.5, 0.0, 0.0), False),
    (10, _yaw(0.15, 1.0 + 1e-9), (1.5, 0.0, 0.0), False),   # the third frame, unmoved; (q_last^-1 q).w = 1 + 1e-9: acos is NaN, NaN > 0.1 is false
    (11, Y, (1.5, 0.0, 0.0), True),                 # unmoved, but size - kf_num > 2
    (12, ID, (9.0, 0.0, 0.0), False),               # moved and turned at once after a keyframe: too soon
]


def _python_gate(frames):
    from glio_amd import odometry
    g = odometry.KeyframeGate()
    out = []
    for size, q, t, *_ in frames:
        kf = g.update(q, t, size)
        out.append((int(kf), g.kf_num))
    return out


@pytest.fixture(scope="module")
def gate_exe(tmp_path_factory):
    here = os.path.join(ROOT, "glio_amd", "host")
    exe = str(tmp_path_factory.mktemp("kfgate") / "host_keyframe_gate_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", os.path.join(here, "host_keyframe_gate_test.cpp"), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    return exe


def _cpp_gate(exe, frames):
    text = "".join(f"{size} " + " ".join(float(v).hex() for v in (*q, *t)) + "\n" for size, q, t, *_ in frames)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(frames))]


def test_keyframe_gate_hand_made_sequence(gate_exe):
    assert len(HAND_MADE) == 12
    want = [int(f[3]) for f in HAND_MADE]
    py, cpp = _python_gate(HAND_MADE), _cpp_gate(gate_exe, HAND_MADE)
    assert [k for k, _ in py] == want
    assert cpp == py
    assert [n for _, n in py] == [2, 2, 2, 5, 5, 5, 8, 8, 8, 8, 12, 12]
    assert [int(k) for k in kr.gate_sequence([(f[1], f[2]) for f in HAND_MADE])] == want
    # the NaN arm is what keeps frame 10 out: with the angle clamped into acos' domain nothing changes here (unmoved), but a NaN that compared TRUE would
    # have made it a keyframe -- size - kf_num is 2 there
    assert HAND_MADE[9][0] - py[8][1] == 2


def test_keyframe_gate_cpp_equals_python_on_a_random_walk(gate_exe):
    rng = np.random.default_rng(3)
    frames, t, yaw = [], np.zeros(3), 0.0
    for size in range(1, 201):
        t = t + rng.choice([0.0, 0.05, 0.15, 0.3]) * rng.standard_normal(3)
        yaw += rng.choice([0.0, 0.02, 0.08])
        frames.append((size, _yaw(yaw), tuple(t)))
    py, cpp = _python_gate(frames), _cpp_gate(gate_exe, frames)
    assert cpp == py
    assert [bool(k) for k, _ in py] == kr.gate_sequence([(f[1], f[2]) for f in frames])
    assert 40 < sum(k for k, _ in py) < 120

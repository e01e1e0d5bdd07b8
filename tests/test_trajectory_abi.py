"""CPU: the trajectory's share of the boundary (include/glio_traj.h): its entry points declared and exported, its struct layouts against the ctypes mirror,
its defaults, and what must NOT have moved."""
import ctypes as C
import os
import re

import pytest

from glio_amd import trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_traj_opts_default", "glio_traj_struct_sizes", "glio_traj_create", "glio_traj_destroy", "glio_traj_push_gap", "glio_traj_resolve", "glio_traj_read",
                "glio_traj_last_device_ms"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_traj_[a-z_0-9]+)\s*\(", stripped("glio_traj.h")))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_sizes_and_fields(lib):
    out = (C.c_int32 * 2)()
    assert lib.glio_traj_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(trajectory.GlioTrajOpts), C.sizeof(trajectory.GlioTrajSummary)] == [16, 40]
    fields = lambda name: re.findall(r"\b(\w+)\s*;", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), stripped("glio_traj.h"), re.S).group(1))
    assert fields("glio_traj_opts") == [f[0] for f in trajectory.GlioTrajOpts._fields_]
    assert fields("glio_traj_summary") == [f[0] for f in trajectory.GlioTrajSummary._fields_]


def test_defaults_and_codes(lib):
    o = trajectory.default_opts()
    assert (o.max_gaps, o.max_frames_per_gap, o.max_samples_per_gap, o.max_iterations) == (4096, 32, 4096, 15)
    assert trajectory.default_opts(max_gaps=7).max_gaps == 7
    hdr = stripped("glio_traj.h")
    assert re.search(r"#define GLIO_TRAJ_MAX_FRAMES 32\b", hdr) and trajectory.MAX_FRAMES == 32
    m = re.search(r"enum \{ GLIO_TRAJ_NO_CONVERGENCE = 0, GLIO_TRAJ_FUNCTION_TOLERANCE = 1, GLIO_TRAJ_PARAMETER_TOLERANCE = 2, GLIO_TRAJ_GRADIENT_TOLERANCE = 3,\s*"
                  r"GLIO_TRAJ_MIN_RADIUS = 4, GLIO_TRAJ_FAILURE = 5, GLIO_TRAJ_NOT_SOLVED = 6", hdr)
    assert m and len(trajectory.TERMINATION_NAMES) == 7
    import np_ceres
    assert (np_ceres.NO_CONVERGENCE, np_ceres.FUNCTION_TOL, np_ceres.PARAMETER_TOL, np_ceres.GRADIENT_TOL, np_ceres.MIN_RADIUS, np_ceres.FAILURE) == (0, 1, 2, 3, 4, 5)


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    hip = stripped("glio_hip.h")
    assert "glio_traj" not in hip and "glio_traj" not in stripped("glio_types.h")


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "trajectory_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "oracle" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "trajectory_restated" not in open(os.path.join(dirpath, f)).read(), f

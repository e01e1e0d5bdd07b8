"""CPU: the damped solve's share of the boundary (include/glio_pgraph_lm.h, included by include/glio_hip.h): its entry points declared and exported, its struct
layouts against the ctypes mirror, its defaults against Ceres 1.14's published ones -- and what must NOT have moved: glio_abi_version, glio_pgraph_struct_sizes,
the four earlier termination codes."""
import ctypes as C
import os
import re

import pytest

from glio_amd import ctypes_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_pgraph_lm_opts_default", "glio_pgraph_lm_struct_sizes", "glio_pgraph_solve_damped", "glio_pgraph_lm_history"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_pgraph_[a-z_0-9]+)\s*\(", stripped("glio_pgraph_lm.h")))
    assert declared == set(ENTRY_POINTS)
    assert re.search(r'#include\s+"glio_pgraph_lm.h"', stripped("glio_hip.h"))
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_sizes(lib):
    out = (C.c_int32 * 2)()
    assert lib.glio_pgraph_lm_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioPgraphLmOpts), C.sizeof(T.GlioPgraphLmInfo)] == [56, 24]
    fields = lambda name: re.findall(r"\b(\w+)\s*(?:,|;)", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), stripped("glio_types.h"), re.S).group(1))
    assert fields("glio_pgraph_lm_opts") == [f[0] for f in T.GlioPgraphLmOpts._fields_]
    assert fields("glio_pgraph_lm_info") == [f[0] for f in T.GlioPgraphLmInfo._fields_]


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    out = (C.c_int32 * 2)()
    assert lib.glio_pgraph_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioPgraphOpts), C.sizeof(T.GlioPgraphInfo)]
    assert (T.PGRAPH_NOT_RUN, T.PGRAPH_CONVERGED, T.PGRAPH_ITERATION_LIMIT, T.PGRAPH_NONPOSITIVE_PIVOT, T.PGRAPH_MIN_RADIUS) == (0, 1, 2, 3, 4)
    assert T.PGRAPH_LM_TERMINATION_NAMES == T.PGRAPH_TERMINATION_NAMES + ("MIN_RADIUS",)
    hdr = stripped("glio_types.h")
    assert re.search(r"GLIO_PGRAPH_NONPOSITIVE_PIVOT = 3 \}", hdr) and re.search(r"GLIO_PGRAPH_MIN_RADIUS = 4\b", hdr)


def test_defaults_are_the_published_ones(lib):
    from glio_amd import posegraph
    o = posegraph.default_lm_opts()
    assert (o.initial_radius, o.max_radius, o.min_radius, o.min_relative_decrease, o.min_diagonal, o.max_diagonal, o.max_trials) == (1e4, 1e16, 1e-32, 1e-3, 1e-6, 1e32, 0)
    assert posegraph.default_lm_opts(max_trials=7, initial_radius=1.0).max_trials == 7


def test_the_restatement_and_the_product_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "pose_graph_lm_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "oracle" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "pose_graph_lm_restated" not in open(os.path.join(dirpath, f)).read(), f

"""CPU: the pose graph's share of the drop-in boundary (glio_pgraph_*, include/glio_hip.h): struct layouts, the defaults against the reference's statements,
every entry point exported, and the restatement the GPU tests compare against kept apart from the product in both directions."""
import ctypes as C
import math
import os
import re

import pytest

from glio_amd import ctypes_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_pgraph_opts_default", "glio_pgraph_struct_sizes", "glio_pgraph_create", "glio_pgraph_destroy", "glio_pgraph_clear", "glio_pgraph_set_prior",
                "glio_pgraph_append", "glio_pgraph_add_between", "glio_pgraph_add_gps", "glio_pgraph_solve", "glio_pgraph_size", "glio_pgraph_read_poses",
                "glio_pgraph_marginal_covariance", "glio_pgraph_error", "glio_pgraph_poses_dev"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def test_entry_points_resolve_and_are_declared(lib):
    hdr = open(os.path.join(ROOT, "include", "glio_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(glio_pgraph_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_sizes(lib):
    out = (C.c_int32 * 2)()
    assert lib.glio_pgraph_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioPgraphOpts), C.sizeof(T.GlioPgraphInfo)]


def test_defaults_are_the_reference_statements(lib):
    from glio_amd import posegraph
    o = posegraph.default_opts()
    assert list(o.prior_var) == [1e-2, 1e-2, math.pi * math.pi, 1e8, 1e8, 1e8]          # Estimator.cpp:864 (vector6p; :487-488 declare the two noise models)
    assert list(o.odom_var) == [1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4]                      # Estimator.cpp:865
    assert o.gps_var_floor == 1.0                                                        # max(noise, 1.0f), Estimator.cpp:1986
    assert (o.max_iterations, o.relative_error_tol, o.absolute_error_tol) == (100, 1e-5, 1e-5)      # gtsam::GaussNewtonParams (unpinned)
    assert o.segment_nodes == 0 and o.max_nodes >= 65536 and o.max_loops >= 32 and o.max_unary >= 100
    assert (posegraph.GNSS_SPACING, posegraph.GNSS_TIME_WINDOW, posegraph.GNSS_COV_THRESHOLD, posegraph.POSE_COV_THRESHOLD) == (5.0, 0.2, 200.0, 1.0)
    assert T.PGRAPH_TERMINATION_NAMES == ("NOT_RUN", "CONVERGED", "ITERATION_LIMIT", "NONPOSITIVE_PIVOT")


def test_no_device_is_an_error_not_a_fallback(lib):
    if lib.glio_device_count() >= 1:
        pytest.skip("HIP device present")
    from glio_amd import capi, posegraph
    with pytest.raises(capi.GlioError, match="no HIP device"):
        posegraph.PoseGraph()


def test_the_restatement_and_the_product_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "pose_graph_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "oracle" not in src.replace("oracle's", "")
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "pose_graph_restated" not in open(os.path.join(dirpath, f)).read(), f

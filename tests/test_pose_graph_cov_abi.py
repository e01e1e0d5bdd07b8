"""CPU: the boundary of the pose graph's all-node covariance (include/glio_pgraph_cov.h): its entry points declared and exported, glio_pgraph_cov_info against
the ctypes mirror, the prototypes the Python wrapper calls through -- and what must NOT have moved: glio_abi_version and the earlier pose-graph structs."""
import ctypes as C
import os
import re

import pytest

from glio_amd import ctypes_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_pgraph_cov_struct_sizes", "glio_pgraph_covariance_all", "glio_pgraph_covariance_all_dev", "glio_pgraph_covariance_all_last_device_ms",
                "glio_pgraph_covariance_all_last_stage_ms"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_pgraph_[a-z_0-9]+)\s*\(", stripped("glio_pgraph_cov.h")))
    assert declared == set(ENTRY_POINTS) == set(T.PGRAPH_COV_PROTOTYPES)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes == T.PGRAPH_COV_PROTOTYPES[n] and getattr(lib, n).restype is C.c_int
    # a header of its own: the pinned ones neither declare nor include it
    for pinned in ("glio_hip.h", "glio_types.h", "glio_pgraph_lm.h"):
        assert "covariance_all" not in stripped(pinned) and "glio_pgraph_cov" not in stripped(pinned), pinned


def test_struct_size_and_fields(lib):
    out = (C.c_int32 * 1)()
    assert lib.glio_pgraph_cov_struct_sizes(out, 1) == 1
    assert list(out) == [C.sizeof(T.GlioPgraphCovInfo)] == [40]
    body = re.search(r"typedef struct glio_pgraph_cov_info \{(.*?)\} glio_pgraph_cov_info;", stripped("glio_pgraph_cov.h"), re.S).group(1)
    assert re.findall(r"\b(\w+)\s*(?:,|;)", body) == [f[0] for f in T.GlioPgraphCovInfo._fields_]
    assert (T.GlioPgraphCovInfo.bad_node.offset, T.GlioPgraphCovInfo.min_pivot.offset, T.GlioPgraphCovInfo.max_pivot.offset) == (16, 24, 32)


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    out = (C.c_int32 * 2)()
    assert lib.glio_pgraph_struct_sizes(out, 2) == 2 and list(out) == [C.sizeof(T.GlioPgraphOpts), C.sizeof(T.GlioPgraphInfo)]
    assert lib.glio_pgraph_lm_struct_sizes(out, 2) == 2 and list(out) == [C.sizeof(T.GlioPgraphLmOpts), C.sizeof(T.GlioPgraphLmInfo)] == [56, 24]


def test_the_wrappers_exist():
    from glio_amd import posegraph
    assert callable(posegraph.PoseGraph.marginal_covariances) and callable(posegraph.PoseGraph.marginal_covariances_dev)
    hpp = open(os.path.join(ROOT, "glio_amd", "host", "glio_posegraph_backend.hpp")).read()
    assert "marginalCovariances" in hpp and "glio_pgraph_covariance_all(" in hpp

"""CPU: the covariance's share of the boundary (include/glio_cov.h): its entry points declared and exported, its struct layout against the ctypes mirror, what the
header must say, and what must NOT have moved."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_cov_struct_sizes", "glio_covariance_columns", "glio_covariance_slots", "glio_covariance_last_device_ms", "glio_debug_covariance_of"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_(?:cov|covariance|debug_covariance)_[a-z_0-9]+)\s*\(", stripped("glio_cov.h")))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_sizes_and_fields(lib):
    from glio_amd import capi
    out = (C.c_int32 * 1)()
    assert lib.glio_cov_struct_sizes(out, 1) == 1
    assert list(out) == [C.sizeof(capi.GlioCovInfo)] == [32]
    body = re.search(r"typedef struct glio_cov_info \{(.*?)\} glio_cov_info;", stripped("glio_cov.h"), re.S).group(1)
    fields = [f for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for f in re.split(r"\s*,\s*", decl.strip())]
    assert fields == [f[0] for f in capi.GlioCovInfo._fields_]
    assert lib.glio_cov_struct_sizes(None, 0) == 1


def test_the_header_states_the_contract():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "glio_cov.h")).read().replace("\n * ", " "))
    for phrase in ("15 s + 3", "15 W + e", "QuaternionParameterization", "on the LEFT", "HALF a rotation vector", "H_kk == 0", "+INFINITY", "n_free_asked",
                   "GLIO_E_NUMERIC", "no regularisation", "listed twice", "symmetric to the bit", "ONE host wait"):
        assert phrase in text, phrase


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    assert "glio_cov" not in stripped("glio_hip.h") and "glio_cov" not in stripped("glio_types.h")


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "covariance_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "oracle" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "covariance_restated" not in open(os.path.join(dirpath, f)).read(), f

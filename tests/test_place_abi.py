"""CPU: place recognition's share of the boundary (include/glio_place.h): its entry points declared, exported and mirrored, its struct layouts and defaults
against the ctypes mirrors, what the header must say, and what must NOT have moved."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_place_opts_default", "glio_place_struct_sizes", "glio_place_tables", "glio_place_create", "glio_place_create_on_dense", "glio_place_destroy",
                "glio_place_add_frames", "glio_place_read_descriptor", "glio_place_set_descriptor", "glio_place_clear", "glio_place_query", "glio_place_query_many",
                "glio_place_last_device_ms"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), stripped("glio_place.h"), re.S).group(1)
    return [(name, ctype) for ctype, name in re.findall(r"\b(int32_t|float)\s+(\w+);", body)]


def mirror_fields(cls):
    return [(name, {C.c_int32: "int32_t", C.c_float: "float"}[t]) for name, t in cls._fields_]


def test_entry_points_are_declared_exported_and_mirrored(lib):
    from glio_amd import ctypes_types as T
    declared = set(re.findall(r"\b(glio_place_[a-z_0-9]+)\s*\(", stripped("glio_place.h")))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None, n
    assert set(T.PLACE_PROTOTYPES) | {"glio_place_opts_default", "glio_place_destroy"} == set(ENTRY_POINTS)
    # the mirrors take as many arguments as the header's declarations
    text = re.sub(r"\s+", " ", stripped("glio_place.h"))
    for n in ENTRY_POINTS:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(getattr(lib, n).argtypes) == len(args.split(",")), n


def test_struct_layouts_and_constants(lib):
    from glio_amd import ctypes_types as T
    out = (C.c_int32 * 2)()
    assert lib.glio_place_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioPlaceOpts), C.sizeof(T.GlioPlaceMatch)] == [16, 16]
    assert header_fields("glio_place_opts") == mirror_fields(T.GlioPlaceOpts)
    assert header_fields("glio_place_match") == mirror_fields(T.GlioPlaceMatch)
    text = stripped("glio_place.h")
    for name, value in (("GLIO_PLACE_RINGS", T.PLACE_RINGS), ("GLIO_PLACE_SECTORS", T.PLACE_SECTORS), ("GLIO_PLACE_TOP_K_MAX", T.PLACE_TOP_K_MAX)):
        assert re.search(r"#define %s (\d+)" % name, text).group(1) == str(value)
    assert (T.PLACE_RINGS, T.PLACE_SECTORS) == (20, 60)
    from glio_amd import place
    assert place.MATCH_DTYPE.itemsize == C.sizeof(T.GlioPlaceMatch) and [n for n, _ in T.GlioPlaceMatch._fields_] == list(place.MATCH_DTYPE.names)


def test_defaults(lib):
    from glio_amd import capi
    o = capi.place_opts()
    assert (o.max_places, o.top_k_max, o.max_radius, o.lidar_height) == (4096, 8, 80.0, 2.0)
    o = capi.place_opts(max_places=7, top_k_max=3)
    assert (o.max_places, o.top_k_max, o.max_radius) == (7, 3, 80.0)


def test_null_handles_are_refused(lib):
    from glio_amd import capi
    h, o = C.c_void_p(), capi.place_opts()
    assert lib.glio_place_create(None, C.byref(o), C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_place_create_on_dense(None, C.byref(o), C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_place_clear(None) == capi.E_ARG
    assert lib.glio_place_add_frames(None, 1, None, None, None, None) == capi.E_ARG
    n, m = C.c_int32(0), (__import__("glio_amd.ctypes_types", fromlist=["x"]).GlioPlaceMatch * 1)()
    assert lib.glio_place_query(None, 0, 0.0, 1, m, C.byref(n)) == capi.E_ARG
    assert lib.glio_place_query_many(None, 0, 1, 0.0, 0, 1, m, C.byref(n)) == capi.E_ARG
    lib.glio_place_destroy(None)


def test_the_header_states_the_contract():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "glio_place.h")).read().replace("\n * ", " "))
    for phrase in ("UNPINNED", "bit for bit", "no atan2f and no sqrtf", "0 < r2 < rb2[20]", "#{k in 1..19 : rb2[k] <= r2}", "(d.x y') - (d.y x') >= 0", "exactly +0",
                   "No atomic takes part in any sum", "ONE host function, glio_place_tables", "fp64 sum of squares over ascending ring", "cnt(s) = 0 gives exactly 1",
                   "LOWEST shift on a tie", "p_candidate = Rz(yaw) p_query", "depend on the two descriptors only", "Estimator.cpp:5119", "ONE host wait per query call",
                   "leave the store exactly as it was", "NOT BUILT", "ring-key prefilter"):
        assert phrase in text, phrase


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    assert "glio_place" not in stripped("glio_hip.h") and "glio_place" not in stripped("glio_types.h") and "glio_place" not in stripped("glio_dense.h")
    from glio_amd import build
    assert "place_kernels.hip" in build.SOURCES and any(h.endswith("glio_place.h") for h in build.HEADERS)
    assert os.path.exists(os.path.join(ROOT, "glio_amd", "csrc", "place_kernels.hip"))
    # no new environment switch
    src = open(os.path.join(ROOT, "glio_amd", "csrc", "place_kernels.hip")).read()
    assert "getenv" not in src and "glio_switch" not in src


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "place_restated.py")).read()
    assert "ctypes" not in src and "oracle" not in src and "glio_amd" not in src and "capi" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "place_restated" not in open(os.path.join(dirpath, f)).read(), f

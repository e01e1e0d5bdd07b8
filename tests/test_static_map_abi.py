"""CPU: the static map's share of the boundary (include/glio_static.h): its entry points declared, exported and mirrored, its struct layouts and defaults
against the ctypes mirrors, what the header must say, and what must NOT have moved."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_static_opts_default", "glio_static_struct_sizes", "glio_static_tables", "glio_static_relative_pose", "glio_static_create",
                "glio_static_create_on_dense", "glio_static_destroy", "glio_static_classify", "glio_static_read_frame", "glio_static_frame_count",
                "glio_static_read_votes", "glio_static_read_image", "glio_static_last_device_ms"]
CTYPES = {C.c_int32: "int32_t", C.c_float: "float", C.c_int64: "int64_t"}


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), stripped("glio_static.h"), re.S).group(1)
    return [(name, ctype) for ctype, name in re.findall(r"\b(int32_t|int64_t|float)\s+(\w+);", body)]


def test_entry_points_are_declared_exported_and_mirrored(lib):
    from glio_amd import ctypes_types as T
    text = re.sub(r"\s+", " ", stripped("glio_static.h"))
    declared = set(re.findall(r"\b(glio_static_[a-z_0-9]+)\s*\(", text))
    assert declared == set(ENTRY_POINTS)
    assert "glio_gmap_create_on_static" in text and hasattr(lib, "glio_gmap_create_on_static")
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert getattr(lib, n).argtypes is not None, n
        args = re.search(r"\b%s\s*\(([^)]*)\)" % n, text).group(1)
        assert len(getattr(lib, n).argtypes) == len(args.split(",")), n
    assert set(T.STATIC_PROTOTYPES) | {"glio_static_opts_default", "glio_static_destroy"} == set(ENTRY_POINTS) | {"glio_gmap_create_on_static"}


def test_struct_layouts_and_constants(lib):
    from glio_amd import ctypes_types as T
    out = (C.c_int32 * 2)()
    assert lib.glio_static_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioStaticOpts), C.sizeof(T.GlioStaticInfo)] == [48, 32]
    assert header_fields("glio_static_opts") == [(n, CTYPES[t]) for n, t in T.GlioStaticOpts._fields_]
    assert header_fields("glio_static_info") == [(n, CTYPES[t]) for n, t in T.GlioStaticInfo._fields_]
    text = stripped("glio_static.h")
    for name, value in (("GLIO_STATIC_MAX_VIEWS", T.STATIC_MAX_VIEWS), ("GLIO_STATIC_LDS_LIMIT", T.STATIC_LDS_LIMIT), ("GLIO_STATIC_PATH_AUTO", T.STATIC_PATH_AUTO),
                        ("GLIO_STATIC_PATH_GLOBAL", T.STATIC_PATH_GLOBAL)):
        assert re.search(r"#define %s (\d+)" % name, text).group(1) == str(value)
    assert T.STATIC_MAX_VIEWS == 32 and T.STATIC_LDS_LIMIT == 160 * 1024


def test_defaults(lib):
    from glio_amd import capi
    o = capi.static_opts()
    assert (o.rows, o.cols_per_quadrant, o.neighbourhood, o.min_votes, o.max_views, o.image_path) == (44, 90, 1, 2, 16, 0)
    assert (o.elev_min_deg, o.elev_max_deg, o.min_range, o.max_range) == (-31.0, 13.0, 1.0, 80.0)
    assert (o.range_gain, o.range_margin) == (C.c_float(1.05).value, C.c_float(0.3).value)
    # the default image is 44 x 360 floats and fits the LDS path with its tables
    assert 4 * o.rows * 4 * o.cols_per_quadrant == 63360 and 63360 + 4 * (o.rows + 1 + 8 * o.cols_per_quadrant) <= 160 * 1024
    o = capi.static_opts(rows=4, cols_per_quadrant=2)
    assert (o.rows, o.cols_per_quadrant, o.min_votes) == (4, 2, 2)
    from glio_amd import static_map
    assert static_map.MIN_BASELINE == 0.5


def test_bad_options_and_null_handles_are_refused(lib):
    from glio_amd import capi
    import numpy as np
    from glio_amd import ctypes_types as T
    h, o = C.c_void_p(), capi.static_opts()
    assert lib.glio_static_create(None, C.byref(o), C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_static_create_on_dense(None, C.byref(o), C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_gmap_create_on_static(None, None, C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_static_classify(None, 1, None, None, None, None, None) == capi.E_ARG
    assert lib.glio_static_read_image(None, 0, None, None) == capi.E_ARG
    lib.glio_static_destroy(None)
    s2, d = np.zeros(600, np.float32), np.zeros((4096, 2), np.float32)
    for bad in (dict(rows=0), dict(rows=257), dict(cols_per_quadrant=0), dict(cols_per_quadrant=513), dict(neighbourhood=2), dict(min_votes=0), dict(max_views=33),
                dict(min_votes=17), dict(elev_min_deg=13.0), dict(elev_max_deg=89.5), dict(min_range=0.0), dict(max_range=0.5), dict(range_gain=-1.0),
                dict(range_margin=float("nan")), dict(image_path=2)):
        ob = capi.static_opts(**bad)
        assert lib.glio_static_tables(C.byref(ob), T.fptr(s2), T.fptr(d)) == capi.E_ARG, bad
    assert lib.glio_static_tables(C.byref(o), None, T.fptr(d)) == capi.E_ARG
    p = np.array([0.0, 0, 0, 1, 0, 0, 0])
    out = np.zeros(12, np.float32)
    for k, v in ((0, np.nan), (2, np.inf), (3, np.nan)):
        q = p.copy(); q[k] = v
        assert lib.glio_static_relative_pose(T.dptr(q), T.dptr(p), T.fptr(out)) == capi.E_ARG
        assert lib.glio_static_relative_pose(T.dptr(p), T.dptr(q), T.fptr(out)) == capi.E_ARG
    z = p.copy(); z[3] = 0.0
    assert lib.glio_static_relative_pose(T.dptr(p), T.dptr(z), T.fptr(out)) == capi.E_ARG and not out.any()
    assert lib.glio_static_relative_pose(T.dptr(p), T.dptr(p), None) == capi.E_ARG


def test_the_header_states_the_contract():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "glio_static.h")).read().replace("\n * ", " "))
    for phrase in ("UNPINNED", "bit for bit", "no atan2f and no sqrtf", "formed in double", "ONE host function, glio_static_relative_pose",
                   "ONE host function, glio_static_tables", "while hi - lo > 1 { mid = (lo + hi) >> 1;", "if (s2[mid] rho2 <= a) lo = mid; else hi = mid;",
                   "if ((d.x y) - (d.y x) >= 0) lo = mid; else hi = mid;", "An empty cell is +0", "columns wrap", "F > (g2 r2') + m2 (strict)",
                   "DYNAMIC iff through >= min_votes", "No atomic takes part in a sum that is not an integer", "in their original order", "163840",
                   "ONE host wait per glio_static_classify", "leave the object's store, counts and votes exactly as they were", "NOT BUILT", "\"revert\" stage",
                   "range images kept across calls"):
        assert phrase in text, phrase


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    for h in ("glio_hip.h", "glio_types.h", "glio_place.h"):
        assert "glio_static" not in stripped(h), h
    from glio_amd import build
    assert "static_kernels.hip" in build.SOURCES and any(h.endswith("glio_static.h") for h in build.HEADERS)
    src = open(os.path.join(ROOT, "glio_amd", "csrc", "static_kernels.hip")).read()
    assert "getenv" not in src and "glio_switch" not in src          # no new environment switch
    assert "atan2" not in src and "sqrtf" not in src and "fp contract(off)" in src
    assert "asm" not in src


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    for name in ("static_map_restated.py", "static_map_cases.py"):
        src = open(os.path.join(ROOT, "tests", name)).read()
        assert "ctypes" not in src and "oracle" not in src and "glio_amd" not in src and "capi" not in src, name
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "static_map_restated" not in open(os.path.join(dirpath, f)).read(), f

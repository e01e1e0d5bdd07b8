"""CPU checks of the dense store's boundary: the symbols of include/glio_dense.h are exported with the argument types the header documents (and the ctypes
prototypes say the same), the struct that crosses with them (glio_gmap_opts, for glio_gmap_create_on_dense) has the size the library has, and null handles are
refused, not dereferenced."""
import ctypes as C
import os
import re

from glio_amd import ctypes_types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["glio_dense_create", "glio_dense_set_frame_strided", "glio_dense_set_frame", "glio_dense_set_frame_from_features", "glio_dense_read_frame",
         "glio_dense_frame_count", "glio_dense_last_device_ms", "glio_dense_world_cloud", "glio_gmap_create_on_dense"]


def _header_args(name):
    hdr = open(os.path.join(ROOT, "include", "glio_dense.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/glio_dense.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        ptr = "*" in a or "[" in a
        if "**" in a:
            out.append(T.c_void_pp)
        elif any(t in a for t in ("glio_dense", "glio_ctx", "glio_gmap_opts")) or ("void" in a and ptr):
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
    from glio_amd import build, capi, mapping
    build.build()
    lib = capi.load()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert T.DENSE_PROTOTYPES[n] == _header_args(n), n
        assert getattr(lib, n).argtypes == T.DENSE_PROTOTYPES[n] and getattr(lib, n).restype is C.c_int
    assert hasattr(lib, "glio_dense_destroy")
    assert sorted(T.DENSE_PROTOTYPES) == sorted(NAMES)
    # the documented shapes, spelled out once
    assert T.DENSE_PROTOTYPES["glio_dense_set_frame_strided"] == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, T.c_double_p, T.c_double_p,
                                                                  T.c_int_p]
    assert T.DENSE_PROTOTYPES["glio_dense_world_cloud"] == [C.c_void_p, T.c_double_p, T.c_float_p, C.c_int, T.c_int_p]
    # the struct that crosses with glio_gmap_create_on_dense
    sizes = (C.c_int32 * 2)()
    assert lib.glio_gmap_struct_sizes(sizes, 2) == 2 and sizes[0] == C.sizeof(T.GlioGmapOpts) and sizes[1] == C.sizeof(T.GlioGmapInfo)
    # the Python surface
    for m in ("set_frame", "set_frame_from_features", "read_frame", "frame_count", "world_cloud", "last_device_ms"):
        assert callable(getattr(mapping.DenseClouds, m)), m
    # null handles and bad sizes are refused before anything touches a device
    n, h = C.c_int(-7), C.c_void_p()
    opts = mapping.default_opts()
    assert lib.glio_dense_create(0, 0, 10, 10, C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_dense_create(0, 2, 10, 0, C.byref(h)) == capi.E_ARG and not h
    assert lib.glio_dense_create(0, 2, 10, 10, None) == capi.E_ARG
    assert lib.glio_dense_set_frame(None, 0, None, 0, 0.4, None, None, C.byref(n)) == capi.E_ARG
    assert lib.glio_dense_set_frame_from_features(None, 0, None, 0.4, None, None, C.byref(n)) == capi.E_ARG
    assert lib.glio_dense_read_frame(None, 0, None, 0, C.byref(n)) == capi.E_ARG
    assert lib.glio_dense_frame_count(None, 0, C.byref(n)) == capi.E_ARG
    assert lib.glio_dense_world_cloud(None, None, None, 0, C.byref(n)) == capi.E_ARG
    assert lib.glio_dense_last_device_ms(None, None) == capi.E_ARG
    assert lib.glio_gmap_create_on_dense(None, C.byref(opts), C.byref(h)) == capi.E_ARG and not h
    assert n.value == -7
    lib.glio_dense_destroy(None)


def test_the_wave_emit_is_the_dense_store_s_alone():
    """the flag that selects k_lm_emit_wave is set in dense_cloud_kernels.hip and nowhere else: the local map, the keyframe cloud and the loop closure's
    submaps launch what they launched"""
    csrc = os.path.join(ROOT, "glio_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith(".hip") and re.search(r"glio_vg_set_wave_emit\s*\(", open(os.path.join(csrc, f)).read())]
    assert users == ["dense_cloud_kernels.hip", "localmap_kernels.hip"]          # the caller and the definition
    from glio_amd import build
    assert "dense_cloud_kernels.hip" in build.SOURCES

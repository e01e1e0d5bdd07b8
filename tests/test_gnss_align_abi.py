"""CPU: the GNSS frame estimate's share of the boundary (include/glio_align.h): its entry points declared and exported, its struct layouts and defaults
against the ctypes mirrors, what the header must say, and what must NOT have moved."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_align_opts_default", "glio_align_struct_sizes", "glio_align_create", "glio_align_destroy", "glio_align_set_opts", "glio_align_set_factors",
                "glio_align_set_positions", "glio_align_solve", "glio_align_cost", "glio_align_read_coarse", "glio_align_last_device_ms"]


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def header_fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), stripped("glio_align.h"), re.S).group(1)
    out = []
    for ctype, decl in re.findall(r"\b(int32_t|double)\s+([^;]+);", body):
        for f in re.split(r"\s*,\s*", decl.strip()):
            m = re.match(r"(\w+)(?:\[(\w+)\])?$", f)
            n = {None: 1, "GLIO_ALIGN_MAX_ROUNDS": 8}.get(m.group(2)) or int(m.group(2))
            out.append((m.group(1), ctype, n))
    return out


def mirror_fields(cls):
    out = []
    for name, t in cls._fields_:
        n = getattr(t, "_length_", 1)
        base = t._type_ if n > 1 or hasattr(t, "_length_") else t
        out.append((name, {C.c_int32: "int32_t", C.c_double: "double"}[base], n))
    return out


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_align_[a-z_0-9]+)\s*\(", stripped("glio_align.h")))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_layouts(lib):
    from glio_amd import ctypes_types as T
    out = (C.c_int32 * 2)()
    assert lib.glio_align_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioAlignOpts), C.sizeof(T.GlioAlignInfo)] == [104, 312]
    assert header_fields("glio_align_opts") == mirror_fields(T.GlioAlignOpts)
    assert header_fields("glio_align_info") == mirror_fields(T.GlioAlignInfo)
    text = stripped("glio_align.h")
    for name, value in (("GLIO_ALIGN_MAX_ROUNDS", T.ALIGN_MAX_ROUNDS), ("GLIO_ALIGN_MAX_HYPOTHESES", T.ALIGN_MAX_HYPOTHESES), ("GLIO_ALIGN_MAX_ITERATIONS", T.ALIGN_MAX_ITERATIONS)):
        assert re.search(r"#define %s (\d+)" % name, text).group(1) == str(value)
    assert re.search(r"GLIO_ALIGN_OK = 0, GLIO_ALIGN_WEAK = 1, GLIO_ALIGN_UNOBSERVABLE = 2", text)
    assert (T.ALIGN_OK, T.ALIGN_WEAK, T.ALIGN_UNOBSERVABLE) == (0, 1, 2)


def test_defaults(lib):
    """the batch stage's threshold schedule (Estimator.cpp:2764-2767), 72 hypotheses; the restatement runs with the same"""
    import gnss_align_restated as R
    from glio_amd import capi
    o = capi.align_opts()
    assert (o.n_hypotheses, o.n_rounds, o.max_iterations_per_round, o.reserved_) == (72, 4, 10, 0) == (R.H_DEFAULT, len(R.DEFAULT_THRESHOLDS), R.MAX_ITERATIONS, 0)
    assert tuple(o.thresholds) == (1e9, 10.0, 8.0, 6.0, 0.0, 0.0, 0.0, 0.0) and tuple(o.thresholds[:4]) == R.DEFAULT_THRESHOLDS
    assert (o.yaw_tolerance, o.pos_tolerance, o.max_yaw_sigma) == (1e-8, 1e-6, 0.0) == (R.YAW_TOLERANCE, R.POS_TOLERANCE, 0.0)
    o = capi.align_opts(thresholds=[5.0, 4.0], n_hypotheses=0)
    assert (o.n_rounds, o.n_hypotheses, o.thresholds[0], o.thresholds[1]) == (2, 0, 5.0, 4.0)


def test_the_header_states_the_contract():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "glio_align.h")).read().replace("\n * ", " "))
    for phrase in ("LEAVES OUT the dependence of ecef2rotation(a) on a", "FIXED POINT of this iteration", "LOWEST h on a tie", "BEFORE the whitening",
                   "1e-9 H_psipsi", "bit for bit", "(-pi, pi]", "unit-variance rows", "ONE host wait", "No atomic takes part in any sum", "Estimator.cpp:1434-1448",
                   "glio_set_gnss / glio_batch_set_small_factors unchanged", "last linearisation"):
        assert phrase in text, phrase


def test_what_did_not_move(lib):
    assert lib.glio_abi_version() == 5
    assert "glio_align" not in stripped("glio_hip.h") and "glio_align" not in stripped("glio_types.h")


def test_the_formula_has_one_definition():
    """the row and the device ecef2rotation live in factor_math.h; the kernels call them and write out neither again"""
    fm = open(os.path.join(ROOT, "glio_amd", "csrc", "factor_math.h")).read()
    k = open(os.path.join(ROOT, "glio_amd", "csrc", "align_kernels.hip")).read()
    body = fm[fm.index("void fm_align_row("):]
    body = body[:body.index("\n}\n")]
    assert "#pragma clang fp contract(off)" in body and "fm_dd_position(" in body and "fm_dd_satellite(" in body and "fm_dd_row(" in body
    assert "fm_align_row(" in k and "fm_dd_whiten(" in k and "fm_ecef2rotation(" in k
    assert "0.05" not in k and "atan2" not in k and "6378137" not in k
    cap = open(os.path.join(ROOT, "glio_amd", "csrc", "capi.hip")).read()
    tab = open(os.path.join(ROOT, "glio_amd", "csrc", "window_tables.h")).read()
    assert "static inline void ecef2rotation_host(" in tab and "ecef_local_rotation(" in cap          # the host function stays (capi.hip's host arithmetic: window_tables.h)


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "gnss_align_restated.py")).read()
    assert "ctypes" not in src and "oracle" not in src and "glio_amd.align" not in src and "capi" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "gnss_align_restated" not in open(os.path.join(dirpath, f)).read(), f

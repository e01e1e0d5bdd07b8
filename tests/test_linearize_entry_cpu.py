"""Host side of the linearisation launch's entry form, CPU only: the span tables of the prior by keyframe (csrc/window_tables.h, prior_span_tables) through
the library's CPU-callable hook, and the same arithmetic with the exact-zero check of a caller's Jacobian as a stand-alone program under the address and
undefined-behaviour sanitizers (glio_amd/host/host_linearize_entry_test.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "glio_amd", "host", "host_linearize_entry_test.cpp")
TRANS, QUAT, SB = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def standard(W, extra_sb=0):
    slot, kind, idx, at = [], [], [], 0
    for s in range(W - 1):
        for k in range(3 if s == 0 else 2):
            slot.append(s); kind.append(k); idx.append(at)
            at += 9 if k == SB else 3
    for j in range(extra_sb):
        slot.append(1 + j); kind.append(SB); idx.append(at)
        at += 9
    return at, slot, kind, idx


def spans(lib, W, layout):
    n, slot, kind, idx = layout
    a = [np.ascontiguousarray(v, np.int32) for v in (slot, kind, idx)]
    out = np.full((n, 4), -7, np.int32)
    p = [v.ctypes.data_as(C.POINTER(C.c_int32)) for v in a]
    rc = lib.glio_debug_prior_spans(W, n, len(slot), p[0], p[1], p[2], out.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, out


def expected(W, layout):
    """by the definition: the columns of a keyframe's blocks, and those of the keyframe below"""
    n, slot, kind, idx = layout
    cols = {}
    for s, k, i in zip(slot, kind, idx):
        cols.setdefault(s, []).extend(range(i, i + (9 if k == SB else 3)))
    out = np.zeros((n, 4), np.int32)
    ok = 1
    for s, c in cols.items():
        lo, hi = min(c), max(c) + 1
        if hi - lo != len(c) or len(c) > 16:
            ok = 0
        below = cols.get(s - 1)
        for j in c:
            out[j] = (lo, hi, min(below) if below else 0, max(below) + 1 if below else 0)
    return ok, out


@pytest.mark.parametrize("W,extra", [(2, 0), (3, 0), (5, 0), (20, 0), (64, 0), (5, 2), (27, 25)])
def test_span_tables(lib, W, extra):
    layout = standard(W, extra)
    rc, got = spans(lib, W, layout)
    ok, want = expected(W, layout)
    assert rc == ok == (1 if extra == 0 else 0)
    assert np.array_equal(got, want)


def test_span_tables_refuse_bad_layouts(lib):
    from glio_amd import capi
    n, slot, kind, idx = standard(4)
    assert spans(lib, 4, (n, slot, kind, [i + 1 for i in idx]))[0] == capi.E_ARG          # a block past the last column
    assert spans(lib, 4, (n, slot[:-1], kind[:-1], idx[:-1]))[0] == capi.E_ARG            # columns no block covers
    assert spans(lib, 0, (n, slot, kind, idx))[0] == capi.E_ARG


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_linearize_entry_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    assert lines[0] == "W3 np 21 ok 1: [0 15 0 0] [15 21 0 15]"
    assert lines[2].startswith("W20 np 123 ok 1: [0 15 0 0] [15 21 0 15] [21 27 15 21]") and lines[2].endswith("[117 123 111 117]")
    assert lines[4].startswith("W64 np 387 ok 1:")
    assert lines[6] == "W4 reversed np 27 ok 1: [0 15 0 0] [15 21 0 15] [21 27 15 21]"
    assert lines[8].startswith("W5 loop np 51 ok 0:")
    # block diagonal: exact; a negative zero outside the blocks: still exact; 1e-300 there: not
    assert [ln.split(" exact ")[1] for ln in lines[1::2]] == ["1 1 0"] * 5

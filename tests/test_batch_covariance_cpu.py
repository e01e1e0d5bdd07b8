"""CPU: the numpy restatement of the batch stage's selected inversion (batch_covariance_restated.py) through the SAME assertion the device goes
through -- against np.linalg.inv of the oracle's dense H with the anchor's rows and columns deleted -- on the fixed list of cases; the singular
problems detected; and the new header's share of the boundary (include/glio_batch_cov.h)."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import batch_covariance_problems as problems
import batch_covariance_restated as restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["glio_batch_cov_struct_sizes", "glio_batch_covariance", "glio_batch_covariance_last_device_ms", "glio_batch_covariance_last_stage_ms"]
CASES = restated.cases()


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] != "singular"], ids=lambda c: c["name"])
def test_restatement_against_the_dense_inverse(case):
    p = problems.build(case)
    diag, nxt = restated.selected_inverse(p["H"], p["K"], p["B"], p["sbk"], p["anchor"])
    a = p["anchor"]
    if a >= 0:          # the anchor's pose rows and columns: exact zeros
        assert not diag[a][:6, :].any() and not diag[a][:, :6].any()
        assert (a == 0 or not nxt[a - 1][:, :6].any()) and (a == p["K"] - 1 or not nxt[a][:6, :].any())
    assert all(np.array_equal(d, d.T) for d in diag)
    if case["expect"] == "floor":          # kappa_s ~ 6e9: the bound says nothing; the restatement's own error is the device's floor (printed)
        want_diag, want_next, kappa, n = restated.reference_blocks(p["H"], p["K"], p["B"], a)
        err = restated.scaled_error(diag, nxt, want_diag, want_next, p["H"])
        print(f"{case['name']}: n {n}, kappa_s {kappa:.4e}, restatement's scaled error {err:.2e}, 8 n kappa_s eps {8 * n * kappa * restated.EPS:.2e} (not gated)")
        assert np.isfinite(err) and kappa > 1e8
        return
    restated.assert_blocks_within_bound(diag, nxt, p["H"], a, case["name"], restated.GUARD_GNSS if case["expect"] == "gate_gnss" else restated.GUARD)


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "singular"], ids=lambda c: c["name"])
def test_singular_problems_are_detected(case):
    """without GNSS and without an anchor the gauge is free: kappa_s of the scaled H is beyond 1 / eps and the factorisation must end in a bad pivot"""
    p = problems.build(case)
    d = np.sqrt(np.diag(p["H"]))
    assert np.linalg.cond(p["H"] / d[:, None] / d[None, :]) > 1e15
    try:
        diag, nxt = restated.selected_inverse(p["H"], p["K"], p["B"], p["sbk"], -1)
    except restated.NotPositiveDefinite as e:
        assert 0 <= e.keyframe < p["K"]
        return
    # rounding may leave the last pivot a tiny positive number instead: then the numbers must be recognisably meaningless (the device's pivots are not
    # the restatement's, its own test asserts GLIO_E_NUMERIC)
    assert np.abs(diag).max() * np.diag(p["H"]).min() > 1e10


def stripped(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def test_entry_points_resolve_and_are_declared(lib):
    declared = set(re.findall(r"\b(glio_batch_cov[a-z_0-9]*)\s*\(", stripped("glio_batch_cov.h")))
    assert declared == set(ENTRY_POINTS)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n


def test_struct_size_and_fields(lib):
    from glio_amd import ctypes_types as T
    out = (C.c_int32 * 1)()
    assert lib.glio_batch_cov_struct_sizes(out, 1) == 1
    assert list(out) == [C.sizeof(T.GlioBatchCovInfo)] == [40]
    body = re.search(r"typedef struct glio_batch_cov_info \{(.*?)\} glio_batch_cov_info;", stripped("glio_batch_cov.h"), re.S).group(1)
    fields = [f for decl in re.findall(r"\b(?:int32_t|double)\s+([^;]+);", body) for f in re.split(r"\s*,\s*", decl.strip())]
    assert fields == [f[0] for f in T.GlioBatchCovInfo._fields_]


def test_pinned_headers_are_byte_for_byte_untouched(lib):
    """glio_hip.h / glio_types.h as they were before this header came (length and SHA-256 of their bytes), and no word of the new entry points in them"""
    assert lib.glio_abi_version() == 5
    for name in ("glio_hip.h", "glio_types.h"):
        assert "glio_batch_cov" not in open(os.path.join(ROOT, "include", name)).read()
    sizes = {n: (len(open(os.path.join(ROOT, "include", n), "rb").read()), hashlib.sha256(open(os.path.join(ROOT, "include", n), "rb").read()).hexdigest()[:16])
             for n in ("glio_hip.h", "glio_types.h")}
    assert sizes == PINNED, sizes


PINNED = {"glio_hip.h": (70807, "b6f4100e950231ad"), "glio_types.h": (22719, "4482f1b1fcf87103")}


def test_the_header_states_the_contract():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "glio_batch_cov.h")).read().replace("\n * ", " "))
    for phrase in ("glio_batch_solve_tr2 linearises", "no mu D^2", "no 1e-12", "glio_batch_linearize_full", "orc_batch2.c:20", "half-angle", "ANCHOR", "POSE columns",
                   "exact zeros", "no large diagonal", "GLIO_E_NUMERIC", "no regularisation", "bad_keyframe", "GLIO_E_STATE", "sharded", "symmetric to the bit",
                   "next may be NULL", "ONE host wait", "pinned memory", "allocates nothing"):
        assert phrase in text, phrase


def test_the_restatement_and_the_kernel_do_not_know_each_other():
    src = open(os.path.join(ROOT, "tests", "batch_covariance_restated.py")).read()
    assert "glio_amd" not in src and "ctypes" not in src and "import oracle" not in src and "from oracle" not in src
    for dirpath, _, files in os.walk(os.path.join(ROOT, "glio_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                assert "batch_covariance_restated" not in open(os.path.join(dirpath, f)).read(), f

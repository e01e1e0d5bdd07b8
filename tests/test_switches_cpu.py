"""The library's environment switches (glio_amd/csrc/glio_switches.h): one table, one parse rule, two read rules.  CPU only: the hooks are host code.

The expectations of the parse table are the expressions the sources used before the table existed, one per switch, written out below -- not the
table's own normalisations."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXTS = [None, "", "0", "1", "2", "3", "4", "7", "-1", "256", "x"]


def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def on_unless_zero(e):          # !(getenv(N) && atoi(getenv(N)) == 0), (!e || atoi(e) != 0)
    return int(not (e is not None and atoi(e) == 0))


def on_if_nonzero(e):           # e && atoi(e) != 0
    return int(e is not None and atoi(e) != 0)


def number_or(dflt):            # getenv(N) ? atoi(getenv(N)) : dflt
    return lambda e: atoi(e) if e is not None else dflt


def knn_mode(e):                # m = e ? atoi(e) : 0; return m >= 0 && m <= 3 ? m : 0
    m = atoi(e) if e is not None else 0
    return m if 0 <= m <= 3 else 0


# name -> (scope, the expression of the source that read it)
EXPECT = {
    "GLIO_KNN_MODE": ("PROCESS", knn_mode),
    "GLIO_BATCH_MOMENTS": ("PROCESS", number_or(1)),
    "GLIO_BCR_ELIM": ("PROCESS", number_or(-1)),
    "GLIO_DEBUG_FILL": ("PROCESS", number_or(-1)),
    "GLIO_DEBUG_LDS_POISON": ("PROCESS", number_or(0)),
    "GLIO_DEBUG_POISON_ALLOC": ("PROCESS", number_or(0)),
    "GLIO_ROCTX": ("PROCESS", on_if_nonzero),                                               # if (!e || atoi(e) == 0) return;
    "GLIO_CHAIN_FAST": ("PROCESS", lambda e: atoi(e) & 3 if e is not None else 3),          # e ? atoi(e) & 3 : 3
    "GLIO_SOLVE_ENDS": ("PROCESS", lambda e: atoi(e) & 6 if e is not None else 6),          # e ? atoi(e) & 6 : 6
    "GLIO_CHAIN_FRONTS": ("PROCESS", number_or(4)),
    "GLIO_CHAIN_HELPERS": ("PROCESS", on_unless_zero),                                      # helpers_off = e && atoi(e) == 0
    "GLIO_CHAIN_HELPER_POLLS": ("PROCESS", number_or(256)),
    "GLIO_CHAIN_FAT": ("PROCESS", on_unless_zero),
    "GLIO_MARG_SPLIT": ("PROCESS", on_unless_zero),
    "GLIO_BASSOC_LOCAL_TABLES": ("PROCESS", on_unless_zero),
    "GLIO_BASSOC_LOCAL_RATIO": ("PROCESS", number_or(16)),
    "GLIO_BASSOC_SHARED_BINS": ("PROCESS", on_unless_zero),
    "GLIO_EARLY_UPLOAD": ("CREATE", on_unless_zero),
    "GLIO_UNSTAGE_IN_STREAM": ("CREATE", on_if_nonzero),                                    # unstage_up = (w && atoi(w) != 0) ? 0 : 1
    "GLIO_EARLY_UPLOAD_WAIT": ("CREATE", on_if_nonzero),
    "GLIO_CTX_PRIORITY": ("CREATE", on_unless_zero),
    "GLIO_BASSOC_PRIORITY": ("CREATE", on_unless_zero),
    "GLIO_LM_SORT": ("CREATE", on_if_nonzero),
    "GLIO_LM_REBUILD_TIMING": ("CREATE", on_if_nonzero),
    "GLIO_KFCLOUD_TIMING": ("CREATE", on_if_nonzero),
    "GLIO_DENSE_TIMING": ("CREATE", on_if_nonzero),
}
# what the issue of this table spelled out, as a check of the expressions above
SPOT = {("GLIO_CHAIN_FAST", None): 3, ("GLIO_CHAIN_FAST", "7"): 3, ("GLIO_CHAIN_FAST", "-1"): 3, ("GLIO_KNN_MODE", "4"): 0, ("GLIO_KNN_MODE", "3"): 3, ("GLIO_KNN_MODE", "-1"): 0,
        ("GLIO_CHAIN_HELPERS", ""): 0, ("GLIO_CHAIN_HELPERS", "x"): 0, ("GLIO_CHAIN_HELPERS", "0"): 0, ("GLIO_CHAIN_HELPERS", "-1"): 1, ("GLIO_CHAIN_HELPERS", None): 1,
        ("GLIO_BCR_ELIM", None): -1, ("GLIO_DEBUG_FILL", None): -1, ("GLIO_CHAIN_HELPER_POLLS", None): 256, ("GLIO_BASSOC_LOCAL_RATIO", None): 16, ("GLIO_SOLVE_ENDS", "7"): 6}


@pytest.fixture(scope="module")
def lib():
    from glio_amd import build, capi
    build.build()
    return capi.load()


def parse(lib, name, text):
    v = C.c_int(12345)
    rc = lib.glio_debug_switch_parse(name.encode(), None if text is None else text.encode(), C.byref(v))
    assert rc == 0, (name, text, rc)
    return v.value


def test_parse_table(lib):
    from glio_amd import capi
    rows = capi.switches()
    assert sorted(r["name"] for r in rows) == sorted(EXPECT)
    for (name, text), want in SPOT.items():
        assert EXPECT[name][1](text) == want, (name, text)
    for r in rows:
        scope, expr = EXPECT[r["name"]]
        assert r["scope"] == scope and r["default"] == expr(None) and r["doc"], r
        for text in TEXTS:
            assert parse(lib, r["name"], text) == expr(text), (r["name"], text)


def test_names_resolve(lib):
    from glio_amd import capi
    v = C.c_int()
    assert lib.glio_debug_switch_value(b"GLIO_nonexistent", C.byref(v)) == capi.E_ARG
    assert lib.glio_debug_switch_value(None, C.byref(v)) == capi.E_ARG
    assert lib.glio_debug_switch_parse(b"GLIO_nonexistent", b"1", C.byref(v)) == capi.E_ARG
    for r in capi.switches():
        assert lib.glio_debug_switch_value(r["name"].encode(), C.byref(v)) == 0 and v.value == r["value"], r


CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1])
from glio_amd import capi
def values():
    return {r["name"]: r["value"] for r in capi.switches()}
first = values()
os.environ["GLIO_CHAIN_FAST"] = "2"; os.environ["GLIO_BCR_ELIM"] = "1"; del os.environ["GLIO_BASSOC_LOCAL_RATIO"]; os.environ["GLIO_KNN_MODE"] = "2"
os.environ["GLIO_LM_SORT"] = "0"; os.environ["GLIO_CTX_PRIORITY"] = "0"
print(json.dumps([first, values()]))
"""


def test_process_rows_are_one_snapshot_and_create_rows_follow_the_environment(lib):
    """PROCESS rows: what the environment held at the first query, whatever happens to it afterwards.  CREATE rows: what the environment holds now
    (through the hook only: no context, store or map can be created without a device)."""
    from glio_amd import capi
    env = dict(os.environ, GLIO_NO_TORCH_PRELOAD="1", GLIO_CHAIN_FAST="1", GLIO_BCR_ELIM="0", GLIO_BASSOC_LOCAL_RATIO="3", GLIO_LM_SORT="1")
    for k in ("GLIO_KNN_MODE", "GLIO_CTX_PRIORITY"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    first, later = json.loads(out.stdout.strip().splitlines()[-1])
    assert (first["GLIO_CHAIN_FAST"], first["GLIO_BCR_ELIM"], first["GLIO_BASSOC_LOCAL_RATIO"], first["GLIO_KNN_MODE"]) == (1, 0, 3, 0)
    assert (first["GLIO_LM_SORT"], first["GLIO_CTX_PRIORITY"]) == (1, 1)
    scope = {r["name"]: r["scope"] for r in capi.switches()}
    for name in first:
        if scope[name] == "PROCESS":
            assert later[name] == first[name], name
    assert (later["GLIO_LM_SORT"], later["GLIO_CTX_PRIORITY"]) == (0, 0)


def test_create_rows_through_the_hook(lib, monkeypatch):
    v = C.c_int()
    for name, (scope, expr) in EXPECT.items():
        if scope != "CREATE":
            continue
        for text in TEXTS:
            if text is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, text)
            assert lib.glio_debug_switch_value(name.encode(), C.byref(v)) == 0 and v.value == expr(text), (name, text)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the table's host code (glio_switches.h + switches.hip) as a program of its own, address and undefined-behaviour sanitizers on: the same parse
    table, and the snapshot against an environment that changes under it"""
    exe = str(tmp_path / "host_switches_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "glio_amd", "host", "host_switches_test.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("GLIO_")}
    out = subprocess.run([exe] + [t for t in TEXTS if t is not None], env=env, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    got = {}
    for ln in lines:
        if ln.startswith("parse "):
            _, name, rest = ln.split(" ", 2)
            text, value = rest.rsplit(" ", 1)
            got[(name, None if text == "-" else text)] = int(value)
    assert got == {(name, text): expr(text) for name, (_, expr) in EXPECT.items() for text in TEXTS}
    assert lines[-3:] == ["first 1 0 1", "later 1 0 0", "set 1 0"]


ALLOWED = {"GLIO_HIP_LIB", "GLIO_NO_TORCH_PRELOAD", "GLIO_DEV_STAMPS", "GLIO_EXTRA_DEFS", "GLIO_POISON_PASS_CHILD", "GLIO_LOCALMAP_ACC"}
ALLOWED_PREFIXES = ("GLIO_BENCH_",)
TABLE_IDS = re.compile(r"GLIO_" r"SW_[A-Z_]+")          # the table's own enumerators (csrc/glio_switches.h): in the stand-alone program only


def test_documentation_names_the_table(lib):
    from glio_amd import capi
    names = {r["name"] for r in capi.switches()}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^##[^\n]*Environment switches[^\n]*\n(.*?)(?=^## |\Z)", doc, flags=re.S | re.M)
    assert m, "INTEGRATION.md has no section 'Environment switches'"
    assert set(re.findall(r"GLIO_[A-Z0-9_]+", m.group(1))) == names
    for r in capi.switches():          # every row with its default and scope on its line
        line = next(ln for ln in m.group(1).splitlines() if f"`{r['name']}`" in ln)
        cells = [c.strip() for c in line.strip("|").split("|")]
        assert cells[1] == str(r["default"]) and cells[3] == r["scope"], line
    # every GLIO_* token of the scripts, tests, Python sources, host programs and the README is a switch of the table, a macro or enumerator
    # of include/, a header guard of glio_amd/host, or one of the few variables above that are not the library's
    declared = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        code = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(h).read(), flags=re.S)
        declared |= set(re.findall(r"GLIO_[A-Z0-9_]+", code))
    files = [os.path.join(ROOT, "README.md")] + glob.glob(os.path.join(ROOT, "glio_amd", "*.py"))
    for d in ("scripts", "tests", os.path.join("glio_amd", "host")):
        for dirpath, _, fs in os.walk(os.path.join(ROOT, d)):
            files += [os.path.join(dirpath, f) for f in fs if f.endswith((".py", ".sh", ".md", ".cpp", ".hpp", ".h", ".txt"))]
    stray = {}
    for f in files:
        text = open(f, errors="replace").read()
        if f.endswith(os.path.join("host", "host_switches_test.cpp")):
            text = TABLE_IDS.sub("", text)
        for tok in set(re.findall(r"GLIO_[A-Z0-9_]+", text)):
            if tok in names or tok in declared or tok in ALLOWED or tok.startswith(ALLOWED_PREFIXES) or (tok.endswith("_HPP_") and f.endswith(".hpp")):
                continue
            if tok.endswith("_") and any(d.startswith(tok) for d in declared | names):          # "GLIO_E_*": a family of declared names
                continue
            stray.setdefault(tok, []).append(os.path.relpath(f, ROOT))
    assert not stray, stray

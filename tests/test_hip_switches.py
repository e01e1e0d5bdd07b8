"""The environment switches no other test reaches through the environment (glio_amd/csrc/glio_switches.h; INTEGRATION.md, "Environment switches").
One child process per case (tests/switches_child.py): the smallest cycle through the code behind the switch, one sha256 over what it computed.
Every switch here selects another route to the same bytes, so each case's hash equals the default child's -- and each child reports through
capi.switches() the value the library saw.  GLIO_CHAIN_FRONTS=2 is the exception: at W = 3 the chain takes two fronts whatever the switch says (four
need W >= 12), so for that case only the value the library saw is checked here; two against four fronts differ in rounding (another elimination order) and are
compared by test_hip_parity.py::test_four_front_elimination through glio_debug_chain_fronts.  (The list of equal-bytes cases held with the library before the table as well: profiles/switch_table_ab.txt.)"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_CASES = [("GLIO_UNSTAGE_IN_STREAM", 1), ("GLIO_EARLY_UPLOAD_WAIT", 1), ("GLIO_CTX_PRIORITY", 0), ("GLIO_CHAIN_FAST", 0), ("GLIO_CHAIN_FRONTS", 2), ("GLIO_KNN_MODE", 3)]
BASSOC_CASES = [("GLIO_BASSOC_SHARED_BINS", 0), ("GLIO_BASSOC_LOCAL_RATIO", 1), ("GLIO_BASSOC_PRIORITY", 0)]
ALL = [n for n, _ in WINDOW_CASES + BASSOC_CASES]


def child(part, name=None, value=None):
    env = {k: v for k, v in os.environ.items() if k not in ALL}
    if name:
        env[name] = str(value)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switches_child.py"), part], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (name, out.stderr[-2000:])
    return json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("{")))


@pytest.fixture(scope="module")
def defaults():
    from glio_amd import capi
    dflt = {r["name"]: r["default"] for r in capi.switches()}
    got = {part: child(part) for part in ("window", "bassoc")}
    for part in got:
        for n in ALL:
            assert got[part]["switches"][n] == dflt[n], (part, n)
    return got


@pytest.mark.parametrize("name,value", WINDOW_CASES)
def test_window_switch_is_seen_and_changes_no_byte(defaults, name, value):
    got = child("window", name, value)
    assert got["switches"][name] == value != defaults["window"]["switches"][name]
    assert got["sha256"] == defaults["window"]["sha256"]


@pytest.mark.parametrize("name,value", BASSOC_CASES)
def test_batch_association_switch_is_seen_and_changes_no_byte(defaults, name, value):
    got = child("bassoc", name, value)
    assert got["switches"][name] == value != defaults["bassoc"]["switches"][name]
    assert got["sha256"] == defaults["bassoc"]["sha256"]

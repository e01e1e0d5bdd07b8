"""A SECOND pass over the parity and solver tests with every CU's LDS and every device allocation of the library poisoned with NaN patterns
(GLIO_DEBUG_LDS_POISON=1, GLIO_DEBUG_POISON_ALLOC=1, GLIO_DEBUG_FILL=255: read when the library loads, hence a child process), so that the
driver's `pytest -m gpu` exercises the ordering / initialisation hazards round 3 found by accident: a kernel that reads LDS or device memory it
(or a predecessor it is ordered behind) has not written now computes NaNs and fails its parity assertion instead of passing on leftovers."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["tests/test_hip_parity.py", "tests/test_hip_marg.py", "tests/test_hip_batch_tr.py", "tests/test_hip_streaming.py", "tests/test_golden_ref.py",
         "tests/test_hip_factor_branches.py", "tests/test_hip_localmap_limits.py"]


def test_parity_suites_pass_with_lds_and_allocations_poisoned():
    if os.environ.get("GLIO_POISON_PASS_CHILD"):
        pytest.skip("already inside the poisoned pass")
    env = dict(os.environ)
    env.update(GLIO_DEBUG_LDS_POISON="1", GLIO_DEBUG_POISON_ALLOC="1", GLIO_DEBUG_FILL="255", GLIO_POISON_PASS_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + FILES, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout or "")[-2500:] + (r.stderr or "")[-500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout, tail

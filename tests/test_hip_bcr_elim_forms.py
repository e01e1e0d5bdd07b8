"""Both forms of the block-cyclic reduction's elimination at every node size.  By size the library takes the register-step form (k_bcr_elim) at
M = 36 and the blocked form (k_bcr_elim2) from M = 54 on, so k_bcr_elim<54/72/90> and k_bcr_elim2<36> run only when GLIO_BCR_ELIM forces them.
The switch is read when the library loads: every case is a child process.  The pose solve is held to the sequential banded solve by
test_block_cyclic_reduction_equals_sequential_banded_solve itself (M = 36 at (37, 3), M = 72 at (50, 12)); the solve with the IMU chain is held to
the oracle with the assertions and tolerances of test_ragged_last_super_block_with_the_imu_chain (M = 54 at K = 13 band 6, M = 90 at K = 50 band 12,
the latter built as test_imu_chain_under_the_references_end_windows_band_12 builds it)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_HEAD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from glio_amd import batch
from glio_amd import ctypes_types as T
"""

_POSE = _HEAD + r"""
from test_hip_batch import test_block_cyclic_reduction_equals_sequential_banded_solve as check
check(%d, %d)
print("ELIM_OK")
"""

_IMU = _HEAD + r"""
from oracle import pyoracle as po
from test_hip_batch_tr import _imu_problem, _stage
K, band = %d, %d
if band == 6:
    gt, init, con, dq, dd, frame, imu, sb0 = _imu_problem(K, band, per_kf=100, seed=59)
else:
    sr = 6
    gt, init = batch.make_poses(K, seed=77 + K, perturb=(0.08, 0.004))
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 156, band, seed=77 + K, search_range=sr)
    con = (ci, cj, cp.numpy(), nc.numpy(), score.numpy())
    rng = np.random.default_rng(77 + K)
    odo = gt.copy(); odo[:, :3] += rng.normal(0, 0.02, (K, 3))
    dq = batch.delta_q_pairs(odo, sr)
    dd, frame = batch.make_batch_gnss(gt, seed=77 + K)
    for f in dd:
        f.threshold = 10.0
    imu, _, sb0 = batch.make_batch_imu(K, seed=77 + K)
opts = T.batch_tr_opts(max_iterations=12)
P = po.BatchProblem(K, band, *con, dq=dq, dd=dd, frame=frame, imu=imu)
want, wsb, wsum = P.solve2(init, opts, sb0)
st = _stage(K, band, con, dq, dd, frame, imu=imu)
poses, sb, summ = st.solve_tr(init, opts, speed_bias=sb0)
st.close()
assert summ.iterations == wsum.iterations and summ.termination == wsum.termination, (summ.as_dict(), wsum.as_dict())
assert np.isclose(summ.final_cost, wsum.final_cost, rtol=1e-8)
assert np.abs(poses - want).max() < 1e-7 and np.abs(sb - wsb).max() < 1e-6
print("ELIM_OK")
"""


@pytest.mark.parametrize("elim", ["0", "1"])
@pytest.mark.parametrize("script,K,band", [(_POSE, 37, 3), (_POSE, 50, 12), (_IMU, 13, 6), (_IMU, 50, 12)],
                         ids=["pose_M36", "pose_M72", "imu_M54", "imu_M90"])
def test_either_elimination_form_at_every_node_size(script, K, band, elim):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GLIO_BCR_ELIM=elim)
    p = subprocess.run([sys.executable, "-c", script % (root, os.path.join(root, "tests"), K, band)], env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert p.returncode == 0 and "ELIM_OK" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]

"""The problems behind batch_covariance_restated.cases(): built with the generators of test_hip_batch_tr.py, the oracle's dense H computed once per
case and shared (read only) by the CPU and the GPU tests."""
import numpy as np

from glio_amd import batch
from test_hip_batch_tr import _imu_problem, _problem

_BUILT = {}


def _end_windows_problem(K):
    """the band-12 form of test_imu_chain_under_the_references_end_windows_band_12 (windows=True)"""
    band, sr = 12, 6
    gt, init = batch.make_poses(K, seed=77 + K, perturb=(0.08, 0.004))
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 156, band, seed=77 + K, search_range=sr)
    rng = np.random.default_rng(77 + K)
    odo = gt.copy(); odo[:, :3] += rng.normal(0, 0.02, (K, 3))
    dq = batch.delta_q_pairs(odo, sr)
    dd, frame = batch.make_batch_gnss(gt, seed=77 + K)
    for f in dd:
        f.threshold = 10.0
    imu, _, sb0 = batch.make_batch_imu(K, seed=77 + K)
    return gt, init, (ci, cj, cp.numpy(), nc.numpy(), score.numpy()), dq, dd, frame, imu, sb0


def build(case):
    """dict(K, band, B, sbk, con, dq, dd, frame, imu, init, sb0, anchor, H): H the oracle's dense matrix at (init, sb0)"""
    key = (case["family"], case["K"], case["band"], case["gnss"])
    if key not in _BUILT:
        from oracle import pyoracle as po
        K, band = case["K"], case["band"]
        if case["family"] == "imu":
            # (with GNSS the generator's own defaults, at which the conditioning behind GUARD_GNSS was measured: kappa_s 3.0e7 .. 4.1e7)
            gt, init, con, dq, dd, frame, imu, sb0 = _end_windows_problem(K) if band == 12 and not case["gnss"] else _imu_problem(K, band)
        else:
            gt, init, con, dq, dd, frame = _problem(K, band)
            for f in dd:
                f.threshold = 10.0
            imu, sb0 = None, None
        if not case["gnss"]:
            dd = []
        P = po.BatchProblem(K, band, *con, dq=dq, dd=dd, frame=frame, imu=imu)
        H = P.linearize_dense(init, sb0)[0]
        H.setflags(write=False)
        _BUILT[key] = dict(K=K, band=band, B=15 if imu is not None else 6, sbk=6 if band <= 6 else 12, con=con, dq=dq, dd=dd, frame=frame, imu=imu,
                           init=init, sb0=sb0, H=H)
    return dict(_BUILT[key], anchor=case["anchor"])


def stage(p):
    from test_hip_batch_tr import _stage
    return _stage(p["K"], p["band"], p["con"], p["dq"], p["dd"], p["frame"], imu=p["imu"])

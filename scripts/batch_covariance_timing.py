"""Timing of the batch stage's per-keyframe marginal covariance (glio_batch_covariance, csrc/batch_cov_kernels.hip), medians of --reps, nothing gated.  The
workload: K = 2000 keyframes x 60 plane constraints, band 6, delta_q and DD pseudoranges at threshold 10, one rank; once as the pose problem (B = 6,
36 x 36 nodes) and once with the ImuFactor chain (B = 15, 54 x 54 nodes after the pre-elimination).  Per problem the whole call (host clock, and the
device time by HIP events) and its stages by HIP events: linearise, factor, down-sweep (with the triangular solves and the pre-eliminated blocks),
gather, copy -- with and without the (k, k + 1) blocks.
Beside them, from the same session and NOT the code under test: one banded solve of the pose problem at the same K (glio_batch_time_solve: factor + back
substitution of the block cyclic reduction) and one threshold round (glio_batch_solve_tr2 at threshold 10).  The expectation, stated in DESIGN section 9
before measuring and reported as MET or NOT MET: the down-sweep costs a small multiple (at most 4 x) of the factorisation it follows.  Prints ONE JSON line.
    python scripts/batch_covariance_timing.py [--reps 10] [--keyframes 2000] [--out profiles/batch_covariance_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glio_amd import batch  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

STAGES = ["linearise", "factor", "down_sweep", "gather", "copy"]


def stats(v):
    v = np.asarray(v, float)
    return {"median": round(float(np.median(v)), 5), "min": round(float(v.min()), 5), "max": round(float(v.max()), 5)}


def time_covariance(st, init, sb, anchor, cross, reps):
    for _ in range(2):
        st.covariance(init, sb, anchor=anchor, cross=cross)
    wall, dev, stage = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = st.covariance(init, sb, anchor=anchor, cross=cross)
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(st.covariance_last_device_ms())
        stage.append(st.covariance_last_device_ms(stages=True))
    stage = np.array(stage)
    info = r[-1]
    return {"call_ms": stats(wall), "device_ms": stats(dev), "stages_device_ms": {n: stats(stage[:, i]) for i, n in enumerate(STAGES)},
            "levels": int(info.levels), "min_pivot": float(info.min_pivot), "max_pivot": float(info.max_pivot),
            "largest_sigma_t_m": float(np.sqrt(max(np.diag(d)[:3].max() for d in r[0])))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K, band = a.keyframes, 6
    gt, init = batch.make_poses(K)
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 60, band)
    con = (ci, cj, cp.numpy(), nc.numpy(), score.numpy())
    dd, frame = batch.make_batch_gnss(gt)
    dq = batch.delta_q_pairs(gt, 3)
    res = {"metric": "batch_keyframe_covariance", "device": "MI355X (gfx950)", "reps": a.reps, "keyframes": K, "band": band, "constraints": int(len(ci)), "ranks": 1}
    # ---- the parent's yardsticks: one banded solve, one threshold round (pose problem)
    st = batch.BatchStage(K, band, len(ci))
    st.set_constraints(*con)
    st.set_small_factors(dq, dd, frame, threshold=10.0)
    Hg = st.new_hg()
    st.linearize(init, Hg)
    res["banded_solve_ms"] = stats([st.time_solve(Hg, 1e-4, 5) for _ in range(a.reps)])
    opts = T.batch_tr_opts(max_iterations=100)
    wall, summ = [], None
    for r in range(2 + max(3, a.reps // 2)):
        t0 = time.perf_counter()
        summ = st.solve_tr(init, opts)[1]
        wall.append(1e3 * (time.perf_counter() - t0))
    res["threshold_round"] = {"call_ms": stats(wall[2:]), "iterations": int(summ.iterations),
                              "note": "planes + delta_q + DD at threshold 10, no IMU chain; host clock around glio_batch_solve_tr2"}
    # ---- B = 6
    res["pose_B6"] = {"diag": time_covariance(st, init, None, -1, False, a.reps), "diag_and_next": time_covariance(st, init, None, -1, True, a.reps),
                      "anchored_diag_and_next": time_covariance(st, init, None, 0, True, a.reps)}
    # ---- B = 15
    imu, _, sb0 = batch.make_batch_imu(K)
    st.set_imu(imu)
    res["imu_B15"] = {"diag": time_covariance(st, init, sb0, -1, False, a.reps), "diag_and_next": time_covariance(st, init, sb0, -1, True, a.reps),
                      "anchored_diag_and_next": time_covariance(st, init, sb0, 0, True, a.reps)}
    st.close()
    exp = {}
    for key in ("pose_B6", "imu_B15"):
        s = res[key]["diag_and_next"]["stages_device_ms"]
        ratio = s["down_sweep"]["median"] / s["factor"]["median"]
        exp[key] = {"factor_ms": s["factor"]["median"], "down_sweep_ms": s["down_sweep"]["median"], "ratio": round(ratio, 2), "verdict": "MET" if ratio <= 4.0 else "NOT MET"}
    res["expectation"] = {"statement": "the down-sweep costs at most 4 x the factorisation it follows", **exp}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

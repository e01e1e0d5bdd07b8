"""Timing of the GNSS frame estimate (glio_align_*, csrc/align_kernels.hip), medians of --reps, nothing gated.  The workload: K = 2000 keyframes x 2 systems x
10 satellites (3 998 factors, 35 982 rows, 16.9 MB of glio_dd_psr), H = 360, the trajectory turned by 2.1 rad and moved by (35, -20, 4) m.  Per stage, the
call on the host clock and (where the library records it) the device time by HIP events:
  set_factors      the factor upload and the unpack into row records
  one_iteration    a solve without a search, one round, one iteration: the start kernel, one linearisation, one step
  coarse_search    a solve with H = 360, one round, one iteration, MINUS one_iteration
  solve            the whole solve at the defaults with H = 360
  refresh          the whole solve with H = 0 from the previous estimate
Beside them, from the same session: one threshold round of the batch stage (planes + delta_q + DD at threshold 10, no IMU chain, glio_batch_solve_tr2) on the
same K, and the numpy restatement of the solve on the measuring host (context only).  The expectation reported as MET or NOT MET: the solve's device time is
below one batch round.  Prints ONE JSON line.
    python scripts/gnss_align_timing.py [--reps 10] [--keyframes 2000] [--out profiles/gnss_align_timing.json] [--no-batch] [--no-restatement]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glio_amd import align, batch, capi  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402


def stats(v):
    v = np.asarray(v, float)
    return {"median": round(float(np.median(v)), 5), "min": round(float(v.min()), 5), "max": round(float(v.max()), 5)}


def timed(fn, reps, device_ms=None):
    for _ in range(2):
        fn()
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append(1e3 * (time.perf_counter() - t0))
        if device_ms:
            dev.append(device_ms())
    out = {"call_ms": stats(wall)}
    if device_ms:
        out["device_ms"] = stats(dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--hypotheses", type=int, default=360)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-batch", action="store_true")
    ap.add_argument("--no-restatement", action="store_true")
    a = ap.parse_args()
    K, H = a.keyframes, a.hypotheses
    gt, init = batch.make_poses(K)
    dd, frame = batch.make_batch_gnss(gt)
    c21, s21 = np.cos(2.1), np.sin(2.1)
    local = np.ascontiguousarray((gt[:, :3] - np.array([35.0, -20.0, 4.0])) @ np.array([[c21, -s21, 0], [s21, c21, 0], [0, 0, 1]]))
    arr = (T.GlioDdPsr * len(dd))(*dd)
    res = {"metric": "gnss_frame_alignment", "device": "MI355X (gfx950)", "reps": a.reps, "keyframes": K, "factors": len(dd), "rows": sum(f.n_sat - 1 for f in dd),
           "hypotheses": H, "factor_bytes": len(dd) * T.C.sizeof(T.GlioDdPsr)}
    al = align.GnssAlignment(len(dd), K)
    res["set_factors"] = timed(lambda: al.set_factors(arr), a.reps)
    al.set_positions(local)
    dev = al.last_device_ms

    def solve(start, **kw):
        al.set_opts(**kw)
        return lambda: al.solve(start)

    one = timed(solve(frame, n_hypotheses=0, thresholds=[1e9], max_iterations_per_round=1), a.reps, dev)
    both = timed(solve(frame, n_hypotheses=H, thresholds=[1e9], max_iterations_per_round=1), a.reps, dev)
    res["one_iteration"] = one
    res["coarse_search"] = {"device_ms_median": round(both["device_ms"]["median"] - one["device_ms"]["median"], 5), "with_one_iteration": both}
    res["solve"] = timed(solve(frame, n_hypotheses=H), a.reps, dev)
    est = al.solve(frame)
    res["solve"]["result"] = {"status": est.info["status_name"], "winner": est.info["winner"], "yaw": est.yaw, "yaw_sigma": est.info["yaw_sigma"],
                              "rounds": [list(r) for r in est.info["rounds"]]}
    res["refresh"] = timed(solve(est.frame, n_hypotheses=0), a.reps, dev)
    al.close()
    if not a.no_batch:
        band = 6
        ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 60, band)
        st = batch.BatchStage(K, band, len(ci))
        st.set_constraints(ci, cj, cp.numpy(), nc.numpy(), score.numpy())
        st.set_small_factors(batch.delta_q_pairs(gt, 3), dd, frame, threshold=10.0)
        opts = T.batch_tr_opts(max_iterations=100)
        summ = []
        res["batch_round"] = timed(lambda: summ.append(st.solve_tr(init, opts)[1]), max(3, a.reps // 2))
        res["batch_round"].update(iterations=int(summ[-1].iterations), constraints=int(len(ci)),
                                  note="one threshold round: planes + delta_q + DD at threshold 10, no IMU chain; host clock around glio_batch_solve_tr2")
        st.close()
        lo = res["batch_round"]["call_ms"]["median"]
        res["expectation"] = {"statement": "the solve's device time is below one batch round", "solve_device_ms": res["solve"]["device_ms"]["median"], "batch_round_ms": lo,
                              "verdict": "MET" if res["solve"]["device_ms"]["median"] < lo else "NOT MET"}
    if not a.no_restatement:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import gnss_align_restated as R
        fs = R.Factors([R.factor_dict(f) for f in dd])
        t0 = time.perf_counter()
        r = R.solve(fs, local, 0.0, np.array(frame.anc_ecef[:]), H=H)
        res["restatement_on_the_measuring_host_s"] = round(time.perf_counter() - t0, 3)
        res["restatement_agrees"] = bool(r["winner"] == est.info["winner"] and abs(r["psi"] - est.yaw) < 1e-7)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

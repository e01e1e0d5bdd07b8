"""Timing of the window's marginal covariance (glio_covariance_*, csrc/covariance_kernels.hip), medians of --reps, nothing gated:
  (i)  synthetic windows of n = 75 (the released configuration), 313 (C2: W = 20 + 13 epochs), 799 (C5-sized: W = 52 + 19 epochs) and 928 (the limit):
       the newest slot's 15 columns and all n columns -- the call on the host clock and its device time by HIP events (state upload, linearisation,
       assembly, factorisation, substitution, Gram product and the result's copy);
  (ii) beside each: the existing one-workgroup dense factorisation at the same n (glio_debug_chol_time, skip = 0) plus one GLIO_KERNEL_LINEARIZE_ALL launch;
  (iii) host_demo_stream's keyframe cycle at the released configuration with and without cov=1, the two alternated in one session.
The expectation reported as MET or NOT MET: the newest-slot call's device time is no more than (ii) at n = 75 and less than it at n >= 313, the margin the
spread of the runs.  Prints ONE JSON line.
    python scripts/covariance_timing.py [--reps 10] [--stream-reps 5] [--out profiles/covariance_timing.json] [--no-stream]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import capi, synth  # noqa: E402

# W, clock-drift epochs wanted (the GNSS generator decides; the n that results is what is reported)
SHAPES = [(5, 0), (20, 13), (52, 19), (61, 13)]


def stats(v):
    v = np.asarray(v, float)
    return {"median": round(float(np.median(v)), 5), "min": round(float(v.min()), 5), "max": round(float(v.max()), 5)}


def windows(reps):
    out, lib = {}, capi.load()
    for W, nd in SHAPES:
        kw = dict(with_gnss=True, gnss_epoch_dt=0.4 * (W - 1) / nd) if nd else dict(with_prior=True)
        win = synth.make_window(W=W, pts_per_scan=1024, seed=synth.SEED_BASE + 730 + W, **kw)
        corr = synth.analytic_correspondences(win)
        ctx = capi.Context(win.opts)
        ctx.load_window(win, corr, use_gnss=bool(nd), use_prior=not nd)
        st = win.init.copy()
        if not nd:
            st.n_ddt = 0
        n = 15 * W + st.n_ddt
        rec = {"window": W, "epochs": int(st.n_ddt)}
        for name, ask in (("newest_slot", dict(slots=[W - 1])), ("all_columns", dict(columns=np.arange(n)))):
            for _ in range(3):
                cov, info = ctx.covariance(st, **ask)
            wall, dev = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.covariance(st, **ask)
                wall.append(1e3 * (time.perf_counter() - t0)); dev.append(ctx.covariance_last_device_ms())
            rec[name] = {"call_ms": stats(wall), "device_ms": stats(dev), "n_free": info.n_free, "pivot_range": [info.min_pivot, info.max_pivot]}
        ctx.linearize(st)                   # (glio_time_kernel launches at the epochs of the last linearisation)
        chol, lin = [], []
        ms = C.c_float()
        for _ in range(reps):
            capi._check(lib.glio_debug_chol_time(ctx._h, n, 1, 0, C.byref(ms))); chol.append(ms.value)
            lin.append(ctx.time_kernel(capi.KERNEL_LINEARIZE_ALL, reps=1))
        rec["one_workgroup_cholesky_ms"] = stats(chol)
        rec["linearize_all_launch_ms"] = stats(lin)
        both = np.asarray(chol) + np.asarray(lin)
        rec["cholesky_plus_linearize_ms"] = stats(both)
        new = rec["newest_slot"]["device_ms"]
        spread = max(new["max"] - new["min"], float(both.max() - both.min()))
        rec["spread_ms"] = round(spread, 5)
        if n <= 88:
            rec["expectation"] = "MET" if new["median"] <= float(np.median(both)) + spread else "NOT MET"
        else:
            rec["expectation"] = "MET" if new["median"] < float(np.median(both)) else "NOT MET"
        out[f"n_{n}"] = rec
        ctx.close()
    return out


def stream(reps):
    from glio_amd.host import window_io
    import tempfile
    W, n_fill, tm, pts = 5, 50, 8, 4096
    NK = n_fill + tm
    long = synth.make_window(W=W + NK, pts_per_scan=pts, with_gnss=False, with_prior=False, seed=synth.SEED_BASE + 77)
    wins = [synth.sub_window(long, j, W) for j in range(NK + 1)]
    wins[0].opts.max_map_points = 1 << 18
    out, dev = {"default": [], "cov": []}, []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "released.bin")
        window_io.write_stream(path, long, wins, W, NK, pts, lm_width=50, leaf=0.4)
        kw = dict(device=0, search_range=6, feature_res_num=100, timed=tm, ahead=True, map_ahead=True)
        window_io.run_demo_stream(path, **kw)
        for _ in range(reps):
            for name, cv in (("default", False), ("cov", True)):
                r = window_io.run_demo_stream(path, cov=cv, **kw)
                out[name].append(r["cycle_ms"])
                if cv:
                    dev.append(r["covariance_last_device_ms"])
    d, g = stats(out["default"]), stats(out["cov"])
    return {"cycle_ms_default": d, "cycle_ms_with_cov_1": g, "covariance_device_ms_in_that_session": stats(dev), "cycle_growth_ms": round(g["median"] - d["median"], 5),
            "spread_of_the_alternated_runs_ms": round(max(d["max"] - d["min"], g["max"] - g["min"]), 5), "runs_each": reps,
            "note": "released configuration (bench.py: bench_released_config), scan and map sent ahead; cov=1 asks for the newest keyframe's 15 x 15 block after every solve"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stream-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    res = {"metric": "window_marginal_covariance", "device": "MI355X (gfx950)", "reps": a.reps}
    res["windows"] = windows(a.reps)
    res["expectation"] = {k: v["expectation"] for k, v in res["windows"].items()}
    if not a.no_stream:
        res["host_demo_stream_released_config"] = stream(a.stream_reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

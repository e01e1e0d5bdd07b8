"""Device time of the raw-scan feature extraction (glio_features_extract) per synthetic 16 / 32 / 64-line scan, from the host call to the counts and
by HIP events around the kernels; and the front end per scan from raw scans (run_raw) vs from host-side features (run).  Prints ONE JSON line.
    python scripts/features_timing.py [--reps 30] [--out profiles/features_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import capi, features, odometry, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402


def extraction(n_scans, n_az, reps):
    raw = sl.make_scan(n_scans, n_az, sweep_yaw=0.05, seed=5)
    ctx = capi.Context(synth.default_opts(1, pts=1 << 16, map_pts=1 << 16))
    ctx.features_config(features.default_opts(n_scans))
    q = np.array([np.cos(0.025), 0, 0, np.sin(0.025)])
    for _ in range(3):
        ctx.features_extract(raw, q)
    host, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        c = ctx.features_extract(raw, q)
        host.append(1e3 * (time.perf_counter() - t0))
        dev.append(ctx.features_last_device_ms())
    ctx.close()
    return {"points": len(raw), "counts": c.as_dict(), "call_to_counts_ms_median": round(float(np.median(host)), 4),
            "device_kernels_ms_median": round(float(np.median(dev)), 4), "device_kernels_ms_min": round(float(np.min(dev)), 4)}


def front_end(n_frames=10):
    scans = sl.drive(n_frames=n_frames, n_scans=32, n_az=1800)
    q = np.array([1.0, 0, 0, 0])
    o = odometry.frontend_opts(1 << 15, 1 << 17)
    a, b = capi.Context(o), capi.Context(o)
    a.features_config(features.default_opts(32))
    b.features_config(features.default_opts(32))
    ra, rb = odometry.ScanToMapOdometry(a), odometry.ScanToMapOdometry(b)
    t_raw, t_run = [], []
    for k, raw in enumerate(scans):
        t0 = time.perf_counter()
        ra.run_raw(raw, q, max_points=o.max_points_per_scan)
        t1 = time.perf_counter()
        b.features_extract(raw, q)                    # (not timed: the features of run() come from the host in the reference's layout)
        b.features_to_scan(0, odometry.LOCAL_MAP_LEAF)
        ds = b.features_read(T.FEAT_LAST_SCAN)
        t2 = time.perf_counter()
        rb.run(ds, max_points=o.max_points_per_scan)
        t3 = time.perf_counter()
        if k >= 3:
            t_raw.append(1e3 * (t1 - t0)); t_run.append(1e3 * (t3 - t2))
    a.close(); b.close()
    return {"scans": n_frames, "points_per_scan": len(scans[0]), "run_raw_ms_median": round(float(np.median(t_raw)), 4),
            "run_ms_median": round(float(np.median(t_run)), 4), "note": "run(): the 0.2 m-filtered surf cloud handed in from the host; run_raw(): the raw scan"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "features_extract_per_scan", "device": "MI355X (gfx950)"}
    for n, az in ((16, 1800), (32, 1800), (64, 1800)):
        res[f"lines_{n}"] = extraction(n, az, a.reps)
    res["front_end"] = front_end()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Device time of the IMU pre-integration from raw samples (glio_imu_integrate, HIP events around the kernel) for one edge of 40 / 160 / 400 samples and
for 1999 edges of 40 samples in one launch; the same 1999 edges through glio_batch_set_imu (host digest + copy) and glio_batch_set_imu_from_store; the host
integration of the same edges (numpy restatement, and the reference's class where oracle/_ref holds it); the C2 window association of the same session,
which the new keyframe's edge is integrated beside.  Prints ONE JSON line.
    python scripts/imu_timing.py [--reps 30] [--out profiles/imu_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import batch, capi, imu, synth  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402


def make_edge(rng, n):
    smp = np.zeros((n, 7))
    smp[:, 0] = 0.4 / max(n, 1)
    smp[:, 1:4] = np.array([0, 0, 9.8]) + rng.normal(0, 0.3, (n, 3))
    smp[:, 4:7] = rng.normal(0, 0.1, (n, 3))
    return smp, np.r_[0, 0, 9.8, np.zeros(9)]


def med(v):
    return round(float(np.median(v)), 5)


def single_edges(reps):
    out = {}
    rng = np.random.default_rng(1)
    for n in (40, 160, 400):
        st = imu.ImuStore(1, n)
        e = make_edge(rng, n)
        for _ in range(5):
            st.integrate(0, [e]); st.last_device_ms()
        dev, call = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            st.integrate(0, [e])
            call.append(1e3 * (time.perf_counter() - t0))
            dev.append(st.last_device_ms())
        t_np = []
        for _ in range(3):
            t0 = time.perf_counter()
            synth.preintegrate(np.vstack([e[1][0:3], e[0][:, 1:4]]), np.vstack([e[1][3:6], e[0][:, 4:7]]), e[0][:, 0], np.zeros(3), np.zeros(3))
            t_np.append(1e3 * (time.perf_counter() - t0))
        row = {"device_ms_median": med(dev), "device_ms_min": round(float(np.min(dev)), 5), "enqueue_call_ms_median": med(call), "numpy_host_ms_median": med(t_np)}
        try:
            from oracle import pyref
            if pyref.available():
                t_ref = []
                for _ in range(10):
                    t0 = time.perf_counter()
                    pyref.preintegrate(e[1][0:3], e[1][3:6], np.zeros(3), np.zeros(3), e[0][:, 0], e[0][:, 1:4], e[0][:, 4:7])
                    t_ref.append(1e3 * (time.perf_counter() - t0))
                row["cpp_reference_class_ms_median"] = med(t_ref)
        except Exception:
            pass
        out[f"samples_{n}"] = row
        st.close()
    return out


def batch_edges(reps, K=2000, n=40):
    rng = np.random.default_rng(2)
    edges = [make_edge(rng, n) for _ in range(K - 1)]
    st = imu.ImuStore(K - 1, n)
    for _ in range(3):
        st.integrate(0, edges); st.last_device_ms()
    offs = np.arange(K, dtype=np.int32) * n
    smp = np.concatenate([e[0] for e in edges]); start = np.array([e[1] for e in edges])
    dev, call = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        st.integrate_raw(0, offs, smp, start)
        call.append(1e3 * (time.perf_counter() - t0))
        dev.append(st.last_device_ms())
    arr = st.read_structs(0, K - 1)
    stage = batch.BatchStage(K, 6, 16)
    lib = capi.load()
    host, from_store = [], []
    for _ in range(max(5, reps // 4)):
        t0 = time.perf_counter()
        capi._check(lib.glio_batch_set_imu(stage._h, K - 1, arr, C.c_double(synth.GRAVITY)))
        host.append(1e3 * (time.perf_counter() - t0))
    for _ in range(reps):
        t0 = time.perf_counter()
        stage.set_imu_from_store(st, 0)
        capi._check(lib.glio_batch_synchronize(stage._h))
        from_store.append(1e3 * (time.perf_counter() - t0))
    stage.close(); st.close()
    return {"edges": K - 1, "samples_per_edge": n, "device_ms_median": med(dev), "device_ms_min": round(float(np.min(dev)), 5), "enqueue_call_ms_median": med(call),
            "glio_batch_set_imu_host_digest_and_copy_ms_median": med(host), "glio_batch_set_imu_from_store_with_wait_ms_median": med(from_store),
            "note": "glio_batch_set_imu additionally needs the 1999 edges integrated on the host first (the per-edge host rows above, times 1999)"}


def window_association(reps, W=20, pts=65536):
    win = synth.make_window(W=W, pts_per_scan=pts)
    ctx = capi.Context(win.opts)
    ctx.set_map(win.map_pts)
    for s in range(W):
        ctx.set_scan(s, win.scans[s])
    poses = [capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s]) for s in range(W)]
    q2s, t2s = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    for _ in range(3):
        ctx.associate_window(q2s, t2s)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.associate_window(q2s, t2s)
        t.append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    return {"window": W, "points_per_scan": pts, "map_points": int(len(win.map_pts)), "associate_window_call_ms_median": med(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-assoc", action="store_true")
    a = ap.parse_args()
    res = {"metric": "imu_preintegration_from_raw_samples", "device": "MI355X (gfx950)", "reps": a.reps}
    res["one_edge"] = single_edges(a.reps)
    res["batch_1999_edges"] = batch_edges(a.reps)
    if not a.no_assoc:
        res["window_association_same_session"] = window_association(a.reps)
        res["edge_160_under_window_association"] = bool(res["one_edge"]["samples_160"]["device_ms_median"] < res["window_association_same_session"]["associate_window_call_ms_median"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

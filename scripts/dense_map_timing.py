"""What the dense map costs (glio_dense_*, glio_gmap_create_on_dense), measured, nothing gated.  Medians of 10 with the spread, the two routes of every
comparison alternated in the same process after a warm-up.  Prints ONE JSON line.
    python scripts/dense_map_timing.py [--reps 10] [--out profiles/dense_map_timing.json]

  (a) emit    the cut cloud of a 57.6 k-point 32-line synthetic scan at leaf 0.4 and 0.9: the store's VoxelGrid stage (glio_dense_last_device_ms [1]: the staged
              VoxelGrid with the wavefront-per-long-list emit; [1] + [2] with the copy into the store) against the same cloud through the keyframe cloud's route
              (glio_set_scan_filtered, stage [1] of glio_scan_filter_last_device_ms: the staged VoxelGrid with the one-thread-per-list emit, and the copy into the
              row).  The outputs are compared byte for byte first.
  (b) beside  a raw-scan drive: ScanToMapOdometry.run_raw + KeyframeGate per scan, with and without DenseClouds.set_frame_from_features on every keyframe
              (host clock around the loop; run_raw ends in a device synchronise)
  (c) map     51 dense frames at 0.2 m through one glio_gmap_add_frames: device time per call and per stage"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GLIO_KFCLOUD_TIMING", "1")
os.environ.setdefault("GLIO_DENSE_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import capi, features, mapping, odometry, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

TRANS = (0.6, -0.05, 0.02)
IDENTITY = np.array([1.0, 0, 0, 0])


def stats(v):
    v = np.asarray(v, float)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def emit(reps):
    raw = sl.drive(n_frames=1, n_scans=32, n_az=1800)[0]
    fe = capi.Context(synth.default_opts(1, pts=1 << 14, map_pts=1 << 14))
    fe.features_config(features.default_opts(32, max_raw_points=1 << 16))
    fe.features_extract(raw, IDENTITY)
    cut = fe.features_read(T.FEAT_CUT_CLOUD)
    fe.close()
    store = mapping.DenseClouds(1, 1 << 16, 1 << 16)
    win = capi.Context(synth.default_opts(1, pts=1 << 16, map_pts=1 << 14))
    win.scan_filter_config(1 << 16)
    out = {"raw_points": len(raw), "cut_points": len(cut)}
    for leaf in (0.4, 0.9):
        n = store.set_frame(0, cut, leaf, TRANS)
        assert n == win.set_scan_filtered(0, cut, leaf, TRANS)
        a, b = store.read_frame(0), win.get_scan(0)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for _ in range(3):
            store.set_frame(0, cut, leaf, TRANS); win.set_scan_filtered(0, cut, leaf, TRANS)
        new, old = [], []
        for _ in range(reps):
            store.set_frame(0, cut, leaf, TRANS); new.append(store.last_device_ms())
            win.set_scan_filtered(0, cut, leaf, TRANS); old.append(win.scan_filter_last_device_ms())
        new, old = np.array(new), np.array(old)
        vg, vgc, par = stats(new[:, 1]), stats(new[:, 1] + new[:, 2]), stats(old[:, 1])
        out[f"leaf_{leaf}"] = {"n_out": n, "identical_bytes": True, "dense_voxel_grid": vg, "dense_voxel_grid_and_copy": vgc, "dense_deskew_and_box": stats(new[:, 0]),
                               "keyframe_cloud_voxel_grid_and_copy": par, "ratio_of_medians": round(par["median_ms"] / vgc["median_ms"], 2),
                               "no_slower": "MET" if vgc["median_ms"] <= par["median_ms"] else "NOT MET"}
    out["faster_at_0.9"] = "MET" if out["leaf_0.9"]["dense_voxel_grid_and_copy"]["max_ms"] < out["leaf_0.9"]["keyframe_cloud_voxel_grid_and_copy"]["min_ms"] else "NOT MET"
    store.close(); win.close()
    return out


def beside(reps, n_frames=12):
    scans = sl.drive(n_frames=n_frames, n_scans=32, n_az=1800)
    o = odometry.frontend_opts(1 << 14, 1 << 16)
    fo = features.default_opts(32, max_raw_points=1 << 16)
    store = mapping.DenseClouds(n_frames, 1 << 16, 1 << 16)

    def run(with_dense):
        fe = capi.Context(o)
        fe.features_config(fo)
        od = odometry.ScanToMapOdometry(fe, scan_match_cnt=2)
        gate = odometry.KeyframeGate()
        nk = 0
        t0 = time.perf_counter()
        for s in scans:
            od.run_raw(s, IDENTITY, max_points=o.max_points_per_scan)
            if gate.update_from(od):
                if with_dense:
                    store.set_frame_from_features(nk, fe, 0.4, od.rel_pose[4:].copy())
                nk += 1
        ms = 1e3 * (time.perf_counter() - t0) / len(scans)
        store.read_frame(0)                      # (the store's stream is drained outside the timed loop)
        fe.close()
        return ms, nk
    run(True); run(False)
    w, wo, nk = [], [], 0
    for _ in range(reps):
        a, nk = run(True); w.append(a)
        b, _ = run(False); wo.append(b)
    sw, so = stats(w), stats(wo)
    spread = max(sw["max_ms"] - sw["min_ms"], so["max_ms"] - so["min_ms"])
    diff = sw["median_ms"] - so["median_ms"]
    return {"scans": len(scans), "keyframes": nk, "per_scan_with_dense": sw, "per_scan_without": so, "difference_of_medians_ms": round(diff, 4),
            "spread_ms": round(spread, 4), "inside_the_spread": "MET" if abs(diff) <= spread else "NOT MET"}


def the_map(reps, n_frames=51):
    raw = sl.drive(n_frames=1, n_scans=32, n_az=1800)[0]
    fe = capi.Context(synth.default_opts(1, pts=1 << 14, map_pts=1 << 14))
    fe.features_config(features.default_opts(32, max_raw_points=1 << 16))
    fe.features_extract(raw, IDENTITY)
    store = mapping.DenseClouds(n_frames, 1 << 16, 1 << 16)
    sizes = [store.set_frame_from_features(k, fe, 0.4, (0.6 + 0.001 * k, -0.05, 0.02)) for k in range(n_frames)]
    poses = np.array([[0.6 * k, 0.05 * k, 0.0, np.cos(0.005 * k), 0.0, 0.0, np.sin(0.005 * k)] for k in range(n_frames)])
    gm = mapping.GlobalMap(store, mapping.default_opts(leaf=0.2))
    frames = list(range(n_frames))
    call, dev, stage = [], [], []
    info = None
    for r in range(reps + 2):
        gm.clear()
        t0 = time.perf_counter()
        info = gm.add(frames, poses)
        ms = 1e3 * (time.perf_counter() - t0)
        if r >= 2:
            call.append(ms); dev.append(gm.last_device_ms()); stage.append(gm.last_stage_ms())
    stage = np.array(stage)
    out = {"frames": n_frames, "points": int(sum(sizes)), "voxels": info.n_voxels, "radix_passes": info.radix_passes, "call_host": stats(call), "call_device": stats(dev),
           "stage_device": {n: stats(stage[:, i]) for i, n in enumerate(("transform", "sort", "runs_and_sums", "merge"))},
           "context": "the surf map of 51 keyframes (profiles/global_map_timing.json) takes 0.50 ms: about 3 k points per keyframe against these"}
    gm.close(); store.close(); fe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert capi.device_count() >= 1, "no HIP device: nothing here can be measured without one"
    res = {"metric": "dense_map", "device": "MI355X (gfx950)", "reps": a.reps, "deskew_trans": list(TRANS), "emit": emit(a.reps), "beside_the_cycle": beside(a.reps),
           "map": the_map(a.reps)}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

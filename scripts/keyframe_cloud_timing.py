"""What the keyframe cloud's device stage costs (glio_set_scan_filtered*, glio_set_scan_from_features*), measured, nothing gated.  Medians of 10 with the
spread, the two routes of every comparison alternated in the same process after a warm-up.  Prints ONE JSON line.
    python scripts/keyframe_cloud_timing.py [--reps 10] [--out profiles/keyframe_cloud_timing.json] [--no-stream]

  (i)   host source: the call against glio_set_scan of the ALREADY filtered cloud of the same output size (the copy and presort the new call cannot
        avoid); the difference is the cost of filtering on the device
  (ii)  resident source: the call against glio_features_read(GLIO_FEAT_SURF) + glio_set_scan of the filtered cloud -- the route it replaces, with the host's
        VoxelGrid left out in the old route's favour
  per stage: HIP events around de-skew + bounding box, the VoxelGrid (+ the copy into the row), the presort (GLIO_KFCLOUD_TIMING=1)
  (iii) host_demo_stream at the released configuration with filter=0.9 against its default (the filtered stream carries fewer points per scan from
        there on: the stage `slide_and_new_scan` is the like-for-like figure, the cycle is context)"""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("GLIO_KFCLOUD_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import capi, features, synth, synth_lidar as sl  # noqa: E402
from glio_amd import ctypes_types as T  # noqa: E402

TRANS = (0.6, -0.05, 0.02)


def stats(v):
    v = np.asarray(v, float)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def big_cloud(n=65536):
    """65 k returns of a 64-line turn with the front end's intensity convention (ring + 0.1 relTime)"""
    raw = sl.make_scan(64, 1800, seed=9)
    ok = np.isfinite(raw[:, :3]).all(1) & (np.linalg.norm(raw[:, :3], axis=1) > 3.0)
    p = raw[ok][:n].copy()
    rng = np.random.default_rng(9)
    p[:, 3] = (rng.integers(0, 64, len(p)) + 0.1 * rng.uniform(0, 1, len(p))).astype(np.float32)
    return np.ascontiguousarray(p)


def case(ctx, fe, cloud, leaf, reps, resident):
    """cloud: the host array (host source) or None (resident: fe holds the extraction)"""
    call = (lambda: ctx.set_scan_from_features(fe, 0, leaf, TRANS)) if resident else (lambda: ctx.set_scan_filtered(0, cloud, leaf, TRANS))
    n_out = call()
    filtered = ctx.get_scan(0)
    if resident:
        old = lambda: (fe.features_read(T.FEAT_SURF), ctx.set_scan(0, filtered))
    else:
        old = lambda: ctx.set_scan(0, filtered)
    for _ in range(3):
        call(); old()
    new_ms, old_ms, stage = [], [], []
    for _ in range(reps):
        new_ms.append(timed(call))
        stage.append(ctx.scan_filter_last_device_ms())
        old_ms.append(timed(old))
    st = np.median(np.asarray(stage), axis=0)
    return {"leaf": leaf, "n_out": int(n_out), "new_call": stats(new_ms), "old_route": stats(old_ms),
            "difference_of_medians_ms": round(float(np.median(new_ms) - np.median(old_ms)), 4),
            "device_stage_ms_median": {"deskew_and_box": round(float(st[0]), 4), "voxel_grid_and_copy": round(float(st[1]), 4), "presort": round(float(st[2]), 4)}}


def stream(reps):
    from glio_amd.host import window_io
    import tempfile
    W, n_fill, tm, pts = 5, 50, 8, 4096
    NK = n_fill + tm
    long = synth.make_window(W=W + NK, pts_per_scan=pts, with_gnss=False, with_prior=False, seed=synth.SEED_BASE + 77)
    wins = [synth.sub_window(long, j, W) for j in range(NK + 1)]
    wins[0].opts.max_map_points = 1 << 18
    out = {"default": [], "filter_0.9": []}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "released.bin")
        window_io.write_stream(path, long, wins, W, NK, pts, lm_width=50, leaf=0.4)
        kw = dict(device=0, search_range=6, feature_res_num=100, timed=tm, ahead=True, map_ahead=True)
        window_io.run_demo_stream(path, **kw)
        for _ in range(reps):
            for name, f in (("default", None), ("filter_0.9", 0.9)):
                r = window_io.run_demo_stream(path, filter=f, **kw)
                out[name].append((r["cycle_ms"], r["stages_ms"]["slide_and_new_scan"], r["stages_ms"]["marginalize"]))
    res = {}
    for name, v in out.items():
        v = np.asarray(v)
        res[name] = {"cycle": stats(v[:, 0]), "slide_and_new_scan": stats(v[:, 1]), "marginalize_with_the_next_scan_sent_ahead": stats(v[:, 2])}
    res["note"] = "released configuration (bench.py: bench_released_config), scan and map sent ahead; with filter=0.9 the 4096-point clouds shrink, so later stages carry fewer points"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-stream", action="store_true")
    a = ap.parse_args()
    res = {"metric": "keyframe_cloud_device_stage", "device": "MI355X (gfx950)", "reps": a.reps, "deskew_trans": list(TRANS)}
    raw = sl.make_scan(32, 1800, seed=5)
    fe = capi.Context(synth.default_opts(1, pts=1 << 16, map_pts=1 << 16))
    fe.features_config(features.default_opts(32))
    cnt = fe.features_extract(raw, np.array([1.0, 0, 0, 0]))
    surf = fe.features_read(T.FEAT_SURF)
    ctx = capi.Context(synth.default_opts(2, pts=1 << 16, map_pts=1 << 16))
    ctx.scan_filter_config(1 << 16)
    big = big_cloud()
    res["surf_of_a_32_line_scan"] = {"raw_points": len(raw), "surf_points": int(cnt.surf)}
    res["big_cloud_points"] = len(big)
    for leaf in (0.9, 0.4):
        res[f"host_source_surf_leaf_{leaf}"] = case(ctx, fe, surf, leaf, a.reps, False)
        res[f"host_source_65k_leaf_{leaf}"] = case(ctx, fe, big, leaf, a.reps, False)
        res[f"resident_source_surf_leaf_{leaf}"] = case(ctx, fe, None, leaf, a.reps, True)
    ctx.close(); fe.close()
    if not a.no_stream:
        res["host_demo_stream_released_config"] = stream(max(3, a.reps // 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The local map rebuilt from 49 resident keyframes (glio_localmap_rebuild_from_frames: what a keyframe call of the reference does after its first loop closure,
Estimator.cpp:3545-3579) at two shapes -- C2 (49 x 65536 points) and the released size (49 x ~4 k points), leaf 0.4 -- against
  (a) the route it replaces on the same inputs: glio_localmap_config + 49 x glio_localmap_push of host clouds + glio_localmap_build;
  (c) host_demo_stream map_rebuild=1 against the default keyframe call (with --stream).
Wall time of the call and the device time of the rebuild's own two launches (HIP events, GLIO_LM_REBUILD_TIMING=1), median of --reps runs after --warmup.
The kernel's point rate is recorded beside its atomics per point (one 64-bit compare-and-swap on the key, four 64-bit adds, one 32-bit add; one more 32-bit add
per NEW voxel).  Prints ONE JSON line.
    python scripts/localmap_rebuild_timing.py [--reps 30] [--warmup 5] [--stream] [--out profiles/localmap_rebuild_timing.json]"""
import argparse
import json
import os
import sys
import time

os.environ["GLIO_LM_REBUILD_TIMING"] = "1"          # (before the library makes its first ring)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glio_amd import batch, capi, synth  # noqa: E402

N_FRAMES, WIDTH, LEAF = 49, 50, 0.4


def med(v):
    return round(float(np.median(v)), 4)


def frames_of(pts, n=N_FRAMES):
    """keyframe clouds in their own frames around a moving sensor + their poses [n][7] = t, q"""
    rng = np.random.default_rng(3)
    scene = synth.make_scene()
    clouds, poses = [], []
    for k in range(n):
        c = np.array([40.0, 0.5, 1.8]) + k * np.array([0.5, 0.02, 0.0])
        p, _ = synth.sample_scene(scene, pts, rng, centre=c, radius=35.0)
        clouds.append(np.ascontiguousarray(np.c_[p - c, np.zeros(pts)], np.float32))
        poses.append(np.r_[c, synth.rotvec_q(np.array([0.0, 0.0, 0.004 * k]))])
    return clouds, np.array(poses)


def shape(name, pts, reps, warmup):
    clouds, poses = frames_of(pts)
    cap = pts
    o = synth.default_opts(1, pts=cap, map_pts=1 << 20)
    ba = batch.BatchAssociation(N_FRAMES, cap, 16)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    frames = np.arange(N_FRAMES, dtype=np.int32)
    moved = poses.copy()
    out = {"frames": N_FRAMES, "points_per_frame": pts, "points": N_FRAMES * pts, "leaf": LEAF}
    # the fused call
    ctx = capi.Context(o)
    ctx.localmap_config(WIDTH, LEAF, cap)
    wall, dev = [], []
    for r in range(warmup + reps):
        moved[:, :3] = poses[:, :3] + 0.01 * (r % 7)                  # (a corrected pose set per call)
        t0 = time.perf_counter()
        n = ctx.localmap_rebuild_from_frames(ba, frames, moved)
        t1 = time.perf_counter()
        if r >= warmup:
            wall.append(1e3 * (t1 - t0)); dev.append(ctx.localmap_last_rebuild_device_ms())
    fused_map = ctx.localmap_read().copy()
    out["rebuild_from_frames"] = {"call_ms_median": med(wall), "call_ms_min": round(float(np.min(wall)), 4), "two_launches_device_ms_median": med(dev),
                                  "map_points": int(n), "points_per_us_in_the_two_launches": round(N_FRAMES * pts / (1e3 * med(dev)), 1),
                                  "atomics_per_point": "1 x 64-bit CAS + 4 x 64-bit add + 1 x 32-bit add (+ 1 x 32-bit add per new voxel)",
                                  "atomic_bytes_added_per_point": 36,
                                  "atomic_GB_per_s": round(36 * N_FRAMES * pts / (1e6 * med(dev)), 1)}
    # (a) the route it replaces: a fresh ring, 49 uploads + pushes, one build
    wall_a = []
    for r in range(max(2, warmup // 2) + max(5, reps // 3)):
        t0 = time.perf_counter()
        ctx.localmap_config(WIDTH, LEAF, cap)
        for k in range(N_FRAMES):
            ctx.localmap_push(clouds[k], moved[k, 3:], moved[k, :3])
        na = ctx.localmap_build()
        t1 = time.perf_counter()
        if r >= max(2, warmup // 2):
            wall_a.append(1e3 * (t1 - t0))
    same = bool(na == n and np.array_equal(ctx.localmap_read(), fused_map))
    # ... and without the re-configuration (pushes into a ring of width 49 evict nothing on the first round only: priced apart)
    t0 = time.perf_counter(); ctx.localmap_config(WIDTH, LEAF, cap); t_cfg = 1e3 * (time.perf_counter() - t0)
    out["config_49_pushes_build"] = {"call_ms_median": med(wall_a), "call_ms_min": round(float(np.min(wall_a)), 4), "of_which_config_ms": round(t_cfg, 4),
                                     "same_map_bit_for_bit": same}
    out["ratio_a"] = round(med(wall_a) / med(wall), 2)
    out["ratio_a_without_config"] = round((med(wall_a) - t_cfg) / med(wall), 2)
    ctx.close(); ba.close()
    return name, out


def stream_ab(W=20, pts=65536, n_keyframes=12):
    """(c): host_demo_stream map_rebuild=1 against the default keyframe call"""
    import tempfile
    from glio_amd.host import window_io
    long = synth.make_window(W=W + n_keyframes, pts_per_scan=pts, with_gnss=True, with_prior=False, seed=synth.SEED_BASE + 12)
    wins = [synth.sub_window(long, j, W) for j in range(n_keyframes + 1)]
    opts = wins[0].opts
    opts.max_ddt_epochs = max(w.init.n_ddt for w in wins) + 8
    opts.max_map_points = 1 << 18
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "stream.bin")
        window_io.write_stream(path, long, wins, W, n_keyframes, pts)
        plain = min((window_io.run_demo_stream(path) for _ in range(2)), key=lambda r: r["cycle_ms"])
        reb = min((window_io.run_demo_stream(path, map_rebuild=True) for _ in range(2)), key=lambda r: r["cycle_ms"])
    return {"window": W, "points_per_scan": pts, "keyframes": n_keyframes,
            "default_call": {"cycle_ms": plain["cycle_ms"], "local_map_ms": plain["stages_ms"]["local_map"], "map_points": plain["map_points"]},
            "map_rebuild_every_call": {"cycle_ms": reb["cycle_ms"], "local_map_ms": reb["stages_ms"]["local_map"], "map_points": reb["map_points"],
                                       "frames_per_rebuild": WIDTH - 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "localmap_rebuild_from_frames", "device": "MI355X (gfx950)", "reps": a.reps, "warmup": a.warmup}
    for name, pts in (("c2", 65536), ("released", 4096)):
        k, v = shape(name, pts, a.reps, a.warmup)
        res[k] = v
    if a.stream:
        res["host_demo_stream"] = stream_ab()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

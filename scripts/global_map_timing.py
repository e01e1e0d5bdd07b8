"""The global map (glio_gmap_add_frames, csrc/globalmap_kernels.hip) against the only route to a map before it -- glio_loop_build_submap with
max_frames_per_submap raised to the frame count -- on the same resident clouds, poses and leaf:
  (a) 51 frames x 32768 points at leaf 0.4 (the loop object's own shape: 2 lc_map_width + 1 frames);
  (b) 667 frames x 32768 points (2000 keyframes at mapping_interval 3) at leaf 0.2, added in chunks of max_points_per_add;
  (c) 3 more frames appended to the map of (b) (the submap route has no append: it rebuilds from 670 frames).
Both calls return when their kernels are done, so the two routes are compared by the wall time of the call; the global map's own device time (HIP events around
its kernels) is recorded beside it, by stage -- transform, sort, runs + sums, merge -- each with a MODEL of the bytes it moves (stated in "bytes_model") over the
time against 8 TB/s.  Medians of --reps runs after --warmup, with min and max as the spread.  Where the submap route does not fit its limits (4096 frames, 2^24
voxels) that is recorded instead of a time.  The keyframe clouds are 16 synthetic scans reused along a straight drive.  Prints ONE JSON line.
    python scripts/global_map_timing.py [--reps 10] [--warmup 2] [--out profiles/global_map_timing.json] [--skip-b]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glio_amd import batch, capi, loop, mapping, synth  # noqa: E402

PTS, DISTINCT, HBM = 32768, 16, 8e12


def spread(v):
    v = np.asarray(v, float)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "n": len(v)}


def drive(n_frames, step):
    rng = np.random.default_rng(3)
    scene = synth.make_scene()
    c0 = np.array([40.0, 0.5, 1.8])
    scans = []
    for k in range(DISTINCT):
        p, _ = synth.sample_scene(scene, PTS, rng, centre=c0, radius=35.0)
        scans.append(np.ascontiguousarray(np.c_[p - c0, np.zeros(PTS)], np.float32))
    poses = np.array([np.r_[c0 + k * np.array([step, 0.02 * step, 0.0]), synth.rotvec_q(np.array([0.0, 0.0, 0.002 * k]))] for k in range(n_frames)])
    return scans, poses


def bytes_model(n, passes, runs, nv_old):
    """per stage: transform reads 16 n, writes 28 n; a sort pass reads 8 n (histogram) + 12 n and writes 12 n (scatter); runs + sums read 8 n + 8 n keys, 4 n ranks,
    16 n points and write 12 n of scan scratch and 44 B per run; the merge reads and writes 44 B per old voxel.  Counter tables and binary searches are left out."""
    return {"transform": 44 * n, "sort": 32 * n * passes, "runs_sums": 48 * n + 44 * runs, "merge": 88 * nv_old}


def gmap_case(ba, frames, poses, leaf, max_voxels, ppa, reps, warmup, append=None):
    gm = mapping.GlobalMap(ba, mapping.default_opts(leaf=leaf, max_voxels=max_voxels, max_points_per_add=ppa))
    per_chunk = max(1, ppa // PTS)
    wall, dev, stages, wall_c, dev_c, stages_c = [], [], [], [], [], []
    info = None
    for r in range(warmup + reps):
        gm.clear()
        w = d = 0.0
        st = np.zeros(4); by = {"transform": 0, "sort": 0, "runs_sums": 0, "merge": 0}
        for a in range(0, len(frames), per_chunk):
            nv_old = gm.size()
            t0 = time.perf_counter()
            info = gm.add(frames[a:a + per_chunk], poses[a:a + per_chunk])
            w += 1e3 * (time.perf_counter() - t0)
            d += gm.last_device_ms(); st += np.array(gm.last_stage_ms())
            n = PTS * len(frames[a:a + per_chunk])
            for k, v in bytes_model(n, info.radix_passes, n, nv_old).items():       # (runs <= n: the model's upper bound)
                by[k] += v
        if r >= warmup:
            wall.append(w); dev.append(d); stages.append(st)
        if append is not None:
            nv_old = gm.size()
            t0 = time.perf_counter()
            ic = gm.add(append[0], append[1])
            wc = 1e3 * (time.perf_counter() - t0)
            if r >= warmup:
                wall_c.append(wc); dev_c.append(gm.last_device_ms()); stages_c.append(np.array(gm.last_stage_ms()))
            by_c = bytes_model(PTS * len(append[0]), ic.radix_passes, PTS * len(append[0]), nv_old)
    names = ("transform", "sort", "runs_sums", "merge")

    def stage_rows(st_list, by_):
        st_list = np.array(st_list)
        return {nm: {"ms": spread(st_list[:, i]), "bytes_model": int(by_[nm]),
                     "fraction_of_8TBps": round(by_[nm] / (1e-3 * max(float(np.median(st_list[:, i])), 1e-6)) / HBM, 4)} for i, nm in enumerate(names)}
    out = {"frames": len(frames), "points": PTS * len(frames), "leaf": leaf, "chunks": (len(frames) + per_chunk - 1) // per_chunk, "voxels": info.n_voxels,
           "radix_passes_last_chunk": info.radix_passes, "call_wall_ms": spread(wall), "device_ms": spread(dev), "stages": stage_rows(stages, by)}
    res_c = None
    if append is not None:
        res_c = {"frames": len(append[0]), "points": PTS * len(append[0]), "voxels_after": ic.n_voxels, "radix_passes": ic.radix_passes, "call_wall_ms": spread(wall_c),
                 "device_ms": spread(dev_c), "stages": stage_rows(stages_c, by_c)}
    full = gm.read() if info.n_voxels <= (1 << 22) else None
    gm.close()
    return out, res_c, full


def submap_case(ba, frames, poses, leaf, reps, warmup, compare=None):
    if len(frames) > 4096:
        return {"fits": False, "why": "more than 4096 frames"}
    try:
        lp = loop.LoopClosure(ba, loop.default_opts(leaf=leaf, max_frames_per_submap=len(frames), max_target_points=1 << 24, max_source_points=1))
    except capi.GlioError as e:
        return {"fits": False, "why": str(e)[:200]}
    wall, n = [], 0
    try:
        for r in range(warmup + reps):
            t0 = time.perf_counter()
            n = lp.build_submap(loop.TARGET, frames, poses)
            if r >= warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
    except capi.GlioError as e:
        lp.close()
        return {"fits": False, "why": str(e)[:200]}
    out = {"fits": True, "voxels": n, "call_wall_ms": spread(wall)}
    if compare is not None:
        out["same_map_bit_for_bit"] = bool(n == len(compare) and np.array_equal(lp.read_submap(loop.TARGET), compare))
    lp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "global_map", "device": "MI355X (gfx950)", "reps": a.reps, "warmup": a.warmup, "points_per_frame": PTS,
           "compared_by": "wall time of the synchronous call (both routes); device_ms and stages: HIP events inside glio_gmap_add_frames"}
    # (a)
    scans, poses = drive(51, 0.5)
    ba = batch.BatchAssociation(51, PTS, 16)
    for k in range(51):
        ba.set_frame(k, scans[k % DISTINCT])
    frames = list(range(51))
    g, _, full = gmap_case(ba, frames, poses, 0.4, 1 << 22, 1 << 21, a.reps, a.warmup)
    s = submap_case(ba, frames, poses, 0.4, a.reps, a.warmup, compare=full)
    res["a_51_frames_leaf_0.4"] = {"gmap": g, "submap_route": s,
                                   "gmap_over_submap_wall": round(g["call_wall_ms"]["median"] / s["call_wall_ms"]["median"], 3) if s.get("fits") else None}
    ba.close()
    print("(a) done", file=sys.stderr, flush=True)
    # (b), (c)
    if not a.skip_b:
        nb = 667
        scans, poses = drive(nb + 3, 1.5)
        ba = batch.BatchAssociation(nb + 3, PTS, 16)
        for k in range(nb + 3):
            ba.set_frame(k, scans[k % DISTINCT])
        frames = list(range(nb))
        g, c, _ = gmap_case(ba, frames, poses[:nb], 0.2, 1 << 24, 1 << 22, a.reps, a.warmup, append=(list(range(nb, nb + 3)), poses[nb:]))
        print("(b), (c) done for the global map", file=sys.stderr, flush=True)
        sreps = max(2, a.reps // 4)
        s = submap_case(ba, frames, poses[:nb], 0.2, sreps, 1)
        res["b_667_frames_leaf_0.2"] = {"gmap": g, "submap_route": s,
                                        "gmap_over_submap_wall": round(g["call_wall_ms"]["median"] / s["call_wall_ms"]["median"], 4) if s.get("fits") else None}
        s3 = submap_case(ba, list(range(nb + 3)), poses, 0.2, sreps, 1) if s.get("fits") else {"fits": False, "why": "as (b)"}
        res["c_append_3_frames"] = {"gmap": c, "submap_route_rebuild_of_670_frames": s3,
                                    "gmap_over_submap_wall": round(c["call_wall_ms"]["median"] / s3["call_wall_ms"]["median"], 5) if s3.get("fits") else None}
        ba.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Loop closure on the device (glio_loop_*): the submap build at the released size (6 + 51 keyframes of ~4 k surf points) and at C2 frame size
(65536 points per keyframe), glio_loop_align on the known-answer case, on the independently sampled ~9 k / ~33 k pair and on the submaps of the drive
(ms per call, device ms, ms per round, the share of queries the brute-force scan answered per round), and the same alignments by the numpy restatement
(tests/loop_restated.py) on this host, with the differences between the two.  Prints ONE JSON line.
    python scripts/loop_timing.py [--reps 10] [--out profiles/loop_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loop_restated as lr  # noqa: E402
from glio_amd import batch, loop, synth, synth_lidar  # noqa: E402

Q_BL = synth.rotvec_q(np.array([0.01, -0.02, 0.015]))
T_BL = np.array([0.05, -0.02, 0.1])


def med(v):
    return round(float(np.median(v)), 4)


def drive_frames(n=57):
    scans = synth_lidar.drive(n_frames=n, n_scans=16, n_az=900, step=(0.5, 0.02, 0.0), yaw_step=0.004)
    clouds = [np.ascontiguousarray(sc[np.isfinite(sc[:, :3]).all(axis=1)][::3], np.float32) for sc in scans]
    info = np.array([np.r_[np.array([40.0, 0.5, 1.8]) + k * np.array([0.5, 0.02, 0.0]), synth.rotvec_q(np.array([0.0, 0.0, 0.004 * k]))] for k in range(n)])
    return clouds, info


def big_frames(n=57, pts=65536):
    """C2 frame size: 65536 points per keyframe, sampled from the scene around the moving sensor, in the sensor frame"""
    rng = np.random.default_rng(3)
    scene = synth.make_scene()
    clouds, info = [], []
    for k in range(n):
        c = np.array([40.0, 0.5, 1.8]) + k * np.array([0.5, 0.02, 0.0])
        p, _ = synth.sample_scene(scene, pts, rng, centre=c, radius=35.0)
        clouds.append(np.ascontiguousarray(np.c_[p - c, np.zeros(pts)], np.float32))
        info.append(np.r_[c, 1.0, 0.0, 0.0, 0.0])
    return clouds, np.array(info)


def time_builds(clouds, info, cap, reps):
    ba = batch.BatchAssociation(len(clouds), cap, 16)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    lp = loop.LoopClosure(ba, loop.default_opts(max_target_points=1 << 20, max_source_points=1 << 19))
    src_f, tgt_f = list(range(56, 50, -1)), list(range(0, 51))
    sp, tp = loop.frame_poses(info[src_f], Q_BL, T_BL), loop.frame_poses(info[tgt_f], Q_BL, T_BL)
    out = {"points_per_frame_mean": int(np.mean([len(c) for c in clouds]))}
    for name, which, fr, ps in (("source_6_frames", loop.SOURCE, src_f, sp), ("target_51_frames", loop.TARGET, tgt_f, tp)):
        for _ in range(2):
            n = lp.build_submap(which, fr, ps)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            lp.build_submap(which, fr, ps)
            t.append(1e3 * (time.perf_counter() - t0))
        out[name] = {"points_in": int(sum(len(clouds[k]) for k in fr)), "points_out": n, "call_ms_median": med(t), "call_ms_min": round(float(np.min(t)), 4)}
    return out, lp, ba


def time_align(lp, reps):
    for _ in range(2):
        r = lp.align()
    call, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = lp.align()
        call.append(1e3 * (time.perf_counter() - t0))
        dev.append(lp.last_device_ms())
    fb = lp.fallbacks()
    n_src = len(lp.read_submap(loop.SOURCE))
    rounds = max(1, len(fb) - 1)
    return r, {"iterations": r.iterations, "state": r.state_name, "converged": r.converged, "fitness": r.fitness, "source_points": n_src,
               "target_points": len(lp.read_submap(loop.TARGET)), "call_ms_median": med(call), "call_ms_min": round(float(np.min(call)), 4),
               "device_ms_median": med(dev), "device_ms_per_round": round(med(dev) / rounds, 4),
               "enqueued_rounds": int(lp.opts.max_iterations),
               "fallback_share_per_round": [round(float(x) / n_src, 5) for x in fb[:-1]], "fallback_share_fitness_search": round(float(fb[-1]) / n_src, 5)}


def restated(src, tgt, brute=False):
    t0 = time.perf_counter()
    w = lr.icp(src, tgt)
    t_acc = 1e3 * (time.perf_counter() - t0)
    out = {"numpy_restatement_kdtree_ms": round(t_acc, 1)}
    if brute:
        t0 = time.perf_counter()
        cur = np.ascontiguousarray(src, np.float32)
        for _ in range(2):
            lr.nn_brute(cur, tgt)
        out["numpy_brute_force_search_ms_per_round"] = round(1e3 * (time.perf_counter() - t0) / 2, 1)
    return w, out


def compare(r, w, lp, tgt):
    dt, dr = lr.pose_error(r.transform, w["transform"])
    fit = lr.fitness(lp.read_current(), tgt, lr.make_tree(tgt))
    return {"iterations_device": r.iterations, "iterations_restated": w["iterations"], "state_device": r.state, "state_restated": w["state"],
            "transform_dt_m": dt, "transform_dR_rad": dr, "fitness_device": r.fitness, "fitness_restated_on_device_cloud": fit,
            "fitness_rel_diff": abs(r.fitness - fit) / fit if fit else 0.0, "fitness_of_the_restatement": w["fitness"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "loop_closure_submaps_and_icp", "device": "MI355X (gfx950)", "reps": a.reps}
    clouds, info = drive_frames()
    res["submap_build_released_size"], lp, ba = time_builds(clouds, info, 8192, a.reps)
    r, row = time_align(lp, a.reps)
    src, tgt = lp.read_submap(loop.SOURCE), lp.read_submap(loop.TARGET)
    w, host = restated(src, tgt)
    row.update(host); row["vs_restatement"] = compare(r, w, lp, tgt)
    res["align_drive_submaps"] = row
    lp.close(); ba.close()
    bc, bi = big_frames()
    res["submap_build_c2_frame_size"], lp, ba = time_builds(bc, bi, 65536, max(3, a.reps // 2))
    lp.close(); ba.close()
    ba = batch.BatchAssociation(2, 64, 16)
    for name, case, brute in (("known_answer", lr.known_answer_case()[:2], True), ("independent_pair", lr.independent_pair(), False)):
        src, tgt = case
        lp = loop.LoopClosure(ba)
        lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
        r, row = time_align(lp, a.reps)
        w, host = restated(src, tgt, brute)
        row.update(host); row["vs_restatement"] = compare(r, w, lp, tgt)
        res["align_" + name] = row
        lp.close()
    ba.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Chooses the places of the end-to-end place-recognition tests (tests/test_hip_place_e2e.py) on the CPU, with the numpy restatement only, and writes the list
to tests/golden/place_scenes.json.

Places are scans by synth_lidar.make_scan in synth.make_scene scenes of DIFFERENT seed and size (tests/place_scenes.py).  Scans along one corridor do not
work as distinct places: 8 m apart they are as close as 0.075 in scan-context distance -- closer than a revisit with 0.8 m of offset -- because the
corridor looks the same from everywhere; `--corridor` repeats that trial.  A candidate place is KEPT when
  * its revisit (offset <= 0.5 m, arbitrary heading) has a restated distance <= 0.2 to it (the threshold place.detect_candidate_by_appearance defaults to), and
  * the revisit's best wrong place (among all candidates' places) is at least 0.05 further away.
The list states how many candidates were refused.  For the alignment test one kept revisit with a heading near 90 deg is chosen such that the restated ICP
(tests/loop_restated.py) from place.initial_guess converges with a fitness below lc_icp_thres (0.2) and the same pair without the heading does not.

    python scripts/search_place_cases.py [--candidates 24] [--corridor]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loop_restated as lr          # noqa: E402
import place_restated as R          # noqa: E402
import place_scenes as S            # noqa: E402
from glio_amd import synth          # noqa: E402

MAX_RADIUS, LIDAR_HEIGHT = 80.0, 2.0
DIST_THRES, MARGIN, ICP_THRES = 0.2, 0.05, 0.2


def unit(cloud, tabs):
    h, m = R.descriptor(cloud, tabs[0], tabs[1], LIDAR_HEIGHT)
    return R.unit_columns(h, m)


def world_cloud(cloud, origin, yaw):
    """the cloud at pose (origin, Rz(yaw)), voxel-averaged at the loop submaps' leaf (what glio_loop_build_submap makes of it, near enough to decide a case)"""
    c, s = math.cos(yaw), math.sin(yaw)
    p = cloud[:, :3].astype(np.float64)
    w = np.stack([c * p[:, 0] - s * p[:, 1] + origin[0], s * p[:, 0] + c * p[:, 1] + origin[1], p[:, 2] + origin[2]], axis=1)
    ds = synth.voxel_average(w, 0.4).astype(np.float32)
    return np.ascontiguousarray(np.c_[ds, np.zeros(len(ds), np.float32)], np.float32)


def corridor_trial(tabs):
    from glio_amd import synth_lidar
    scene = synth.make_scene()
    scans = [synth_lidar.make_scan(16, 360, origin=(40.0 + 8.0 * k, 0.5, 1.8), scene=scene, seed=k, close_frac=0.0) for k in range(6)]
    us = [unit(s, tabs) for s in scans]
    d = [float(R.pair(us[a][0], us[a][1], us[b][0], us[b][1])[0]) for a in range(6) for b in range(a + 1, 6)]
    print(f"one corridor, scans 8 m apart: pairwise distances {min(d):.3f} .. {max(d):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=24)
    ap.add_argument("--corridor", action="store_true")
    a = ap.parse_args()
    tabs = R.tables(MAX_RADIUS)
    if a.corridor:
        corridor_trial(tabs)
    seeds = list(range(1, a.candidates + 1))
    params = {s: S.parameters(s) for s in seeds}
    places = {s: S.place_scan(params[s]) for s in seeds}
    visits = {s: S.revisit_scan(params[s]) for s in seeds}
    up, uv = {s: unit(places[s], tabs) for s in seeds}, {s: unit(visits[s], tabs) for s in seeds}
    between = [float(R.pair(up[x][0], up[x][1], up[y][0], up[y][1])[0]) for x in seeds for y in seeds if x < y]
    print(f"{len(seeds)} places of different scenes: pairwise distances {min(between):.3f} .. {max(between):.3f}")
    kept, refused, rows = [], [], {}
    for s in seeds:
        d_true, shift = R.pair(uv[s][0], uv[s][1], up[s][0], up[s][1])
        d_wrong = min(float(R.pair(uv[s][0], uv[s][1], up[o][0], up[o][1])[0]) for o in seeds if o != s)
        yaw_err = S.angle_diff(float(R.yaw_of_shift(shift)), params[s]["yaw"])
        ok = float(d_true) <= DIST_THRES and d_wrong - float(d_true) >= MARGIN
        print(f"seed {s:3d}: revisit {float(d_true):.4f} (shift {shift}, yaw error {math.degrees(yaw_err):.2f} deg), best wrong place {d_wrong:.4f} -> {'kept' if ok else 'REFUSED'}")
        (kept if ok else refused).append(s)
        rows[s] = dict(distance=float(d_true), shift=int(shift), best_wrong=d_wrong, yaw_error=yaw_err)
    assert len(kept) >= 12, kept
    # the alignment case: a kept revisit with a heading near 90 deg; the restated ICP with the guess reaches the fitness, without it does not
    align = None
    for s in sorted(kept, key=lambda s: abs(params[s]["yaw"] - math.pi / 2)):
        if abs(params[s]["yaw"] - math.pi / 2) > math.radians(15):
            break
        tgt = world_cloud(places[s], params[s]["origin"], 0.0)
        with_guess = lr.icp(world_cloud(visits[s], params[s]["origin"], float(R.yaw_of_shift(rows[s]["shift"]))), tgt)
        without = lr.icp(world_cloud(visits[s], params[s]["origin"], 0.0), tgt)
        print(f"seed {s}: ICP with the guess converged {with_guess['converged']} fitness {with_guess['fitness']:.4f} ({with_guess['iterations']} rounds); "
              f"without {without['converged']} fitness {without['fitness']:.4f} ({without['iterations']} rounds)")
        if with_guess["converged"] and with_guess["fitness"] < 0.5 * ICP_THRES and not (without["converged"] and without["fitness"] < 2.0 * ICP_THRES):
            align = dict(seed=s, fitness_with_guess=with_guess["fitness"], fitness_without=without["fitness"])
            break
    assert align is not None
    out = dict(candidates=len(seeds), refused=refused, seeds=kept, max_radius=MAX_RADIUS, lidar_height=LIDAR_HEIGHT, distance_threshold=DIST_THRES, margin=MARGIN,
               restated={str(s): rows[s] for s in kept}, align=align)
    with open(S.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"kept {len(kept)} of {len(seeds)} candidates ({len(refused)} refused: {refused}); alignment case seed {align['seed']} -> {S.GOLDEN}")


if __name__ == "__main__":
    main()

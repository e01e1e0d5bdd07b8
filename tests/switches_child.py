"""Child process of tests/test_hip_switches.py: one small cycle through the code behind the library's environment switches, one JSON line with a
sha256 over what it computed and the switch values the library reports (capi.switches(); absent with a library that predates the table).
    python tests/switches_child.py window | bassoc"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glio_amd import batch, capi, synth  # noqa: E402


def digest(h, *arrays):
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())


def window(h):
    """W = 3, 512 points per scan, a 4 k-point map, LiDAR + IMU + GNSS + prior; set_imu / set_gnss while the searches run, one solve, one marginalisation"""
    win = synth.make_window(W=3, pts_per_scan=512, seed=synth.SEED_BASE + 61, with_gnss=True, with_prior=True, scan_radius=14.0, map_density=1.0)
    step = max(1, -(-len(win.map_pts) // 4096))
    map_pts = np.ascontiguousarray(win.map_pts[::step])
    c = capi.Context(win.opts)
    c.set_map(map_pts)
    c.set_prior(win.prior)
    for s in range(win.W):
        c.set_scan(s, win.scans[s])
    poses = [capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s]) for s in range(win.W)]
    c.associate_window_async(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
    c.set_imu(win.preints); c.set_gnss(win.frame, win.dd, win.dop)
    sol, summ = c.solve(win.init)
    counts = c.associate_window_counts()
    assert counts.sum() > 0.3 * 512 * win.W and summ.iterations >= 1, (counts, summ.as_dict())
    digest(h, counts, [summ.iterations, summ.termination], [summ.initial_cost, summ.final_cost], sol.trans, sol.quat, sol.speed_bias)
    for s in range(win.W):
        digest(h, *c.get_correspondences(s))
    m = c.marginalize(sol)
    digest(h, m["lin_jac"], m["lin_res"], m["blk_slot"], m["blk_kind"], m["blk_idx"], m["blk_x0"])
    c.close()


def bassoc(h):
    """K = 4 frames of 512 points, 3 pairs, run twice (the second run at moved poses)"""
    win = synth.make_window(W=4, pts_per_scan=512, seed=synth.SEED_BASE + 62, perturb=(0.03, 0.2, 0.0), scan_radius=14.0, map_density=1.0)
    tlb = np.array(win.opts.t_lb)
    poses = np.c_[win.init.trans, win.init.quat]
    moved = poses.copy(); moved[:, :3] += np.random.default_rng(62).normal(0, 0.05, (4, 3))
    ba = batch.BatchAssociation(4, 1024, 100000)
    for k in range(4):
        sc = win.scans[k].copy(); sc[:, :3] -= tlb.astype(np.float32)
        ba.set_frame(k, np.ascontiguousarray(sc))
    ci = np.array([3, 3, 3], np.int32); cj = np.array([0, 1, 2], np.int32)
    total = 0
    for P in (poses, moved):
        counts, n = ba.run(P, ci, cj)
        total += n
        digest(h, counts, *ba.read())
    assert total > 100, total
    ba.close()


if __name__ == "__main__":
    h = hashlib.sha256()
    {"window": window, "bassoc": bassoc}[sys.argv[1]](h)
    seen = {r["name"]: r["value"] for r in capi.switches()} if hasattr(capi, "switches") and hasattr(capi.load(), "glio_debug_switch_row") else None
    print(json.dumps({"sha256": h.hexdigest(), "switches": seen}))

"""The covariance of every pose-graph node (glio_pgraph_covariance_all, include/glio_pgraph_cov.h) timed beside what it replaces, one session:
  3 500 frames with 1 and 8 loop edges, 65 536 frames with 1 loop edge (one node per frame, the drives of scripts/pose_graph_timing.py), and the local graph
  of 700 keyframes with 100 GPS factors.
Per graph, medians of --reps runs after --warmup (min and max as the spread), every run on the same freshly rebuilt graph at its initial estimate:
  all_nodes      the call with diag and next: wall time of the synchronous call, device time and the five stages by HIP events inside it
                 (linearise, segments + separator factor, separator inversion, segment down-sweep, copy)
  one_iteration  one undamped iteration of glio_pgraph_solve (max_iterations = 1): its device time
  per_node       glio_pgraph_marginal_covariance over a sample of 16 nodes spread over the graph: wall time per call; `all_nodes_extrapolated_ms` is that
                 median x N -- an EXTRAPOLATION, nobody ran N calls
and the two expectations of the change: the call within about three undamped iterations; cheaper than the per-node route from a handful of nodes on.
Prints ONE JSON line.
    python scripts/pose_graph_cov_timing.py [--reps 10] [--warmup 2] [--out profiles/pose_graph_cov_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from glio_amd import posegraph  # noqa: E402
from pose_graph_timing import drive, loops_of, spread  # noqa: E402

STAGES = ("linearise", "segments_separator_factor", "separator_inversion", "down_sweep", "copy")


def timed(n, build, reps, warmup, **caps):
    pg = posegraph.PoseGraph(posegraph.fixed_iterations(1, max_nodes=n, **caps))
    sample = [int(v) for v in np.linspace(0, n - 1, 16)]
    wall, dev, stages, it_dev, node_wall, info = [], [], [], [], [], None
    for r in range(warmup + reps):
        pg.clear()
        build(pg)
        pg.read_poses(0, 1)                        # the uploads are not part of any of the three
        t0 = time.perf_counter()
        _, _, info = pg.marginal_covariances(next=True, with_info=True)
        t1 = time.perf_counter()
        ms, st = pg.marginal_covariances_ms()
        per = []
        for k in sample:
            t2 = time.perf_counter()
            pg.marginal_covariance(k)
            per.append(1e3 * (time.perf_counter() - t2))
        si = pg.solve()
        if r >= warmup:
            wall.append(1e3 * (t1 - t0)); dev.append(ms); stages.append(st); it_dev.append(si.device_ms); node_wall.append(float(np.median(per)))
    pg.close()
    st = np.array(stages)
    all_ms, it_ms, node_ms = float(np.median(dev)), float(np.median(it_dev)), float(np.median(node_wall))
    return {"plan": {k: info[k] for k in ("n_nodes", "separators", "full_row_separators", "segment_nodes")},
            "min_pivot": info["min_pivot"], "max_pivot": info["max_pivot"],
            "all_nodes": {"wall_ms": spread(wall), "device_ms": spread(dev), "stage_ms": {k: spread(st[:, i]) for i, k in enumerate(STAGES)}},
            "one_iteration": {"device_ms": spread(it_dev)},
            "per_node": {"sample": sample, "wall_ms_per_call": spread(node_wall), "all_nodes_extrapolated_ms": round(node_ms * n, 1),
                         "note": "EXTRAPOLATED: the sample's median x N; N calls were not run"},
            "iterations_per_call": round(all_ms / it_ms, 2), "within_three_iterations": "MET" if all_ms <= 3.0 * it_ms else "NOT MET",
            "break_even_nodes": round(all_ms / node_ms, 1), "cheaper_from_a_handful_of_nodes": "MET" if all_ms <= 8 * node_ms else "NOT MET"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"metric": "pose_graph_covariance_all", "device": "MI355X (gfx950)", "reps": a.reps, "warmup": a.warmup, "cases": {},
           "compared_by": "HIP events inside the calls (all_nodes, one_iteration), wall time of the synchronous per-node call; one session",
           "expectations": "all_nodes.device_ms <= 3 x one_iteration.device_ms; break_even_nodes (all_nodes.device_ms / per-node wall ms) a handful (<= 8)"}
    for n, count in ((3500, 1), (3500, 8), (65536, 1)):
        truth, x0 = drive(n, 31)
        loops = loops_of(truth, n, count)

        def build(p, x0=x0, loops=loops):
            p.set_prior(x0[0])
            p.append(x0)
            for lp in loops:
                p.add_between(*lp)
        res["cases"][f"global_{n}_frames_{count}_loops"] = timed(n, build, a.reps, a.warmup, max_loops=32, max_unary=1)
    n = 700
    truth, x0 = drive(n, 32)
    rng = np.random.default_rng(33)
    gps = [(k, truth[k, :3] + rng.normal(0, 1.0, 3), np.array([1.0, 1.0, 4.0])) for k in range(6, n, 7)][:100]

    def build_local(p):
        p.set_prior(x0[0])
        p.append(x0)
        for gp in gps:
            p.add_gps(*gp)
    res["cases"]["local_700_keyframes_100_gps"] = timed(n, build_local, a.reps, a.warmup, max_loops=1, max_unary=len(gps))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

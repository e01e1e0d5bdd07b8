"""The pose graph (glio_pgraph_solve, csrc/posegraph_kernels.hip) timed where the reference uses it:
  (global) a solve after loop closures on a graph of one node per frame -- 3 500 frames (the length of the reference's result/*.csv), 36 000 and 65 536 frames,
           each with 1, 8 and 32 loop edges;
  (local)  700 keyframes with 100 GPS factors: the solve, and the marginal covariance of the last node.
Every case: the wall time of the synchronous call, the device time of the whole solve and of the FIRST iteration by stage (HIP events inside the call:
linearise, segments, separator system, back-substitution + update), the iterations.  Medians of --reps runs after --warmup, min and max as the spread; every
run solves the same freshly rebuilt graph.  Nothing existed before this object to compare against.  As CONTEXT ONLY, beside each case: one linear solve of the
restatement (tests/pose_graph_restated.py: scipy.sparse J^T J + splu) on the host this script runs on -- another machine, another algorithm, one thread.
  (damped) the same global graphs through glio_pgraph_solve_damped: trials, accepted and rejected counts, the whole solve, ms per trial -- and next to each the
           undamped solve of the same graph in the same session (iterations, ms per iteration, its initial and final error).
Prints ONE JSON line.
    python scripts/pose_graph_timing.py [--reps 10] [--warmup 2] [--out profiles/pose_graph_timing.json] [--sizes 3500,36000,65536] [--only-damped]
--only-damped: the damped section alone; with --out, it is merged into the file that is there (the other sections stay as they were measured)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_graph_restated as W  # noqa: E402
from glio_amd import posegraph  # noqa: E402


def spread(v):
    v = np.asarray(v, float)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "n": len(v)}


def drive(n, seed):
    """laps of a 60 m circle at 0.5 m per frame, climbing slowly; dead reckoning with 1e-3 rad / 3e-3 m per edge"""
    turns = n * 0.5 / (2 * np.pi * 60.0)
    truth = W.circle_truth(n, radius=60.0, turn=turns, z_amp=1.0)
    return truth, W.noisy_odometry(truth, np.random.default_rng(seed), 1e-3, 3e-3)


def loops_of(truth, n, count):
    step = max(1, n // (4 * count))
    return [(n - 1 - k * step, k * step, W.between(truth[n - 1 - k * step], truth[k * step]), np.full(6, 0.05)) for k in range(count)]


def timed(pg, build, reps, warmup, covariance_of=None):
    wall, dev, stages, its, cov_wall, info = [], [], [], [], [], None
    for r in range(warmup + reps):
        pg.clear()
        build(pg)
        pg.read_poses(0, 1)                        # the uploads are not part of the solve
        t0 = time.perf_counter()
        info = pg.solve()
        t1 = time.perf_counter()
        if covariance_of is not None:
            pg.marginal_covariance(covariance_of)
        t2 = time.perf_counter()
        if r >= warmup:
            wall.append(1e3 * (t1 - t0)); dev.append(info.device_ms); stages.append(info.stage_ms); its.append(info.iterations); cov_wall.append(1e3 * (t2 - t1))
    st = np.array(stages)
    out = {"solve_wall_ms": spread(wall), "solve_device_ms": spread(dev), "iterations": int(np.median(its)), "termination": info.termination_name,
           "separators": info.separators, "segments": info.segments, "initial_error": info.initial_error, "final_error": info.final_error,
           "first_iteration_stage_ms": {k: spread(st[:, i]) for i, k in enumerate(("linearise", "segments", "separator_system", "backsub_update"))}}
    if covariance_of is not None:
        out["marginal_covariance_wall_ms"] = spread(cov_wall)
    return out


def timed_damped(pg, build, reps, warmup):
    """the damped solve, and the undamped one of the same graph beside it"""
    d_wall, d_dev, u_dev, di, ui = [], [], [], None, None
    for r in range(warmup + reps):
        pg.clear()
        build(pg)
        pg.read_poses(0, 1)
        ui = pg.solve()
        pg.clear()
        build(pg)
        pg.read_poses(0, 1)
        t0 = time.perf_counter()
        di = pg.solve_damped()
        t1 = time.perf_counter()
        if r >= warmup:
            d_wall.append(1e3 * (t1 - t0)); d_dev.append(di.device_ms); u_dev.append(ui.device_ms)
    return {"trials": di.trials, "accepted": di.accepted, "rejected": di.rejected, "invalid": di.invalid, "termination": di.termination_name,
            "initial_error": di.initial_error, "final_error": di.final_error, "final_radius": di.final_radius, "separators": di.separators,
            "solve_wall_ms": spread(d_wall), "solve_device_ms": spread(d_dev), "device_ms_per_trial": spread(np.array(d_dev) / max(di.trials, 1)),
            "undamped": {"iterations": ui.iterations, "termination": ui.termination_name, "initial_error": ui.initial_error, "final_error": ui.final_error,
                         "solve_device_ms": spread(u_dev), "device_ms_per_iteration": spread(np.array(u_dev) / max(ui.iterations, 1))}}


def witness_linear_solve(x0, loops, gps=()):
    g = W.Graph()
    g.add_prior(0, x0[0])
    g.add_chain(x0)
    for lp in loops:
        g.add_between(*lp)
    for gp in gps:
        g.add_gps(*gp)
    r, J = g.linearize(x0, sparse=True)
    t0 = time.perf_counter()
    W.step_sparse(J, r)
    return {"context_only": "one linear solve (J^T J, COLAMD, splu) of the numpy restatement on this script's host CPU, one thread", "ms": round(1e3 * (time.perf_counter() - t0), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="3500,36000,65536")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-damped", action="store_true")
    a = ap.parse_args()
    res = {"metric": "pose_graph", "device": "MI355X (gfx950)", "reps": a.reps, "warmup": a.warmup, "cases": {},
           "compared_by": "nothing existed before this object; wall time of the synchronous call, device times from HIP events inside it"}
    damped = {"reps": a.reps, "warmup": a.warmup, "what": "glio_pgraph_solve_damped on the global graphs, the undamped solve of the same graph beside it, one session",
              "cases": {}}
    for n in [int(s) for s in a.sizes.split(",") if s]:
        truth, x0 = drive(n, 31)
        pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=n, max_loops=32, max_unary=1))
        for count in (1, 8, 32):
            loops = loops_of(truth, n, count)

            def build(p, loops=loops):
                p.set_prior(x0[0])
                p.append(x0)
                for lp in loops:
                    p.add_between(*lp)
            damped["cases"][f"global_{n}_frames_{count}_loops"] = timed_damped(pg, build, a.reps, a.warmup)
        pg.close()
    if a.only_damped:
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
        res["damped"] = damped
        line = json.dumps(res)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(json.dumps(damped))
        return
    res["damped"] = damped
    for n in [int(s) for s in a.sizes.split(",") if s]:
        truth, x0 = drive(n, 31)
        pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=n, max_loops=32, max_unary=1))
        for count in (1, 8, 32):
            loops = loops_of(truth, n, count)

            def build(p, loops=loops):
                p.set_prior(x0[0])
                p.append(x0)
                for lp in loops:
                    p.add_between(*lp)
            c = timed(pg, build, a.reps, a.warmup)
            c["witness"] = witness_linear_solve(x0, loops)
            res["cases"][f"global_{n}_frames_{count}_loops"] = c
        pg.close()
    n = 700
    truth, x0 = drive(n, 32)
    rng = np.random.default_rng(33)
    gps = [(k, truth[k, :3] + rng.normal(0, 1.0, 3), np.array([1.0, 1.0, 4.0])) for k in range(6, n, 7)][:100]
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=n, max_loops=1, max_unary=len(gps)))

    def build_local(p):
        p.set_prior(x0[0])
        p.append(x0)
        for gp in gps:
            p.add_gps(*gp)
    c = timed(pg, build_local, a.reps, a.warmup, covariance_of=n - 1)
    c["witness"] = witness_linear_solve(x0, [], gps)
    res["cases"]["local_700_keyframes_100_gps"] = c
    pg.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

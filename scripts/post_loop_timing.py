"""The windows after a loop closure: wall time of glio_solve and glio_marginalize_keep for the first window (speed-bias priors installed, no prior), for each
transient window (the wider resident prior, one speed-bias block fewer per keyframe) and for the steady state beside them, with the step path each solve took
(glio_debug_solver_path: 2 keyframe chain, 1 arrow, 0 dense) and the prior's width, at two shapes: W = 5 / 4096 points per scan and W = 20 / 65536.  The window's
content is reused from keyframe to keyframe (analytic correspondences; only the prior changes), as tests/test_hip_post_loop.py does.  Median of --reps runs of
the whole sequence after --warmup.  Prints ONE JSON line.
    python scripts/post_loop_timing.py [--reps 10] [--warmup 2] [--out profiles/post_loop_timing.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glio_amd import capi, synth  # noqa: E402


def med(v):
    return round(float(np.median(v)), 4)


def sequence(ctx, win, armed, n_windows):
    """[(solve ms, marginalize_keep ms, step path, n of the prior the NEXT window finds)] over n_windows keyframe calls from a context without a prior"""
    lib = capi.load()
    ctx.set_prior(None)
    st = win.init.copy(); st.n_ddt = 0
    rows = []
    for k in range(n_windows):
        if armed and k == 0:
            ctx.set_speed_bias_priors(st.speed_bias[:win.W - 1])
        t0 = time.perf_counter()
        sol, summ = ctx.solve(st)
        t1 = time.perf_counter()
        n_next = ctx.marginalize_size()[0]
        t2 = time.perf_counter()
        ctx.marginalize_keep(sol)
        t3 = time.perf_counter()
        rows.append(((t1 - t0) * 1e3, (t3 - t2) * 1e3, lib.glio_debug_solver_path(ctx._h), n_next, summ.iterations))
        st = sol
    return rows


def shape(W, pts, reps, warmup):
    win = synth.make_window(W=W, pts_per_scan=pts, with_prior=False, seed=synth.SEED_BASE + 7)
    corr = synth.analytic_correspondences(win)
    ctx = capi.Context(win.opts)
    ctx.load_window(win, corr, use_gnss=False, use_prior=False)
    n_windows = W + 1                                    # the first window, W - 2 transient ones, then the standard layout again
    runs = {True: [], False: []}
    for r in range(warmup + reps):
        for armed in (True, False):
            rows = sequence(ctx, win, armed, n_windows)
            if r >= warmup:
                runs[armed].append(rows)
    ctx.close()

    def table(all_rows):
        out = []
        for k in range(n_windows):
            out.append({"window": k, "solve_ms": med([rr[k][0] for rr in all_rows]), "marginalize_keep_ms": med([rr[k][1] for rr in all_rows]),
                        "step_path": all_rows[0][k][2], "kept_n": all_rows[0][k][3], "iterations": all_rows[0][k][4]})
        return out
    return {"W": W, "points_per_scan": pts, "standard_n": 6 * (W - 1) + 9, "after_loop_closure": table(runs[True]), "steady_state": table(runs[False])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_loop_timing.json"))
    a = ap.parse_args()
    assert capi.device_count() >= 1, "no HIP device"
    res = {"what": "post_loop_timing", "reps": a.reps, "shapes": [shape(5, 4096, a.reps, a.warmup), shape(20, 65536, a.reps, a.warmup)]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

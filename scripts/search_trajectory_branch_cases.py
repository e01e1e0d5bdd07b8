"""CPU only: the search behind tests/trajectory_restated.py::branch_cases() and resolve_cases(), kept for whoever must pick seeds again.

    python scripts/search_trajectory_branch_cases.py push [n_trials]       one JSON line per trial that holds its margins and its one-ulp condition
    python scripts/search_trajectory_branch_cases.py far [n_trials]        push trials of more than one pass with jumps of 2e4 .. 1e6 m (seeds from 1000):
                                                                           the Cauchy branch is rare below that
    python scripts/search_trajectory_branch_cases.py resolve [n_trials]    the same for loop-closure-sized corrections of a resolve

A push trial is make_gap(seed, n_frames, samples_per_segment=1, right_jump=...) with n_frames drawn from the pass-boundary sizes, the jump's length
log-uniform in 1 .. 1e6 m and its angle uniform up to 3.1 rad, each rounded to four digits so that the line can be pasted into the list as it stands.
Every line names the dogleg branches and radius rules the restated solve took, its end, and -- for a run that is still NO_CONVERGENCE after 32 iterations --
whether the 32nd step was accepted.  A resolve trial starts from one fixed left row; in resolve_cases() a gap's left row is what the gaps before it made
of row 0, which moves the roundings, so a pasted line still has to hold its margins there (building the list asserts them) -- take the next line if not.
Nothing here touches a device."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import np_ceres  # noqa: E402
import trajectory_restated as tr  # noqa: E402

SIZES = (1, 2, 3, 9, 10, 18, 19, 27, 28, 32)


def r4(v):
    return float(f"{v:.4g}")


def judged(name, c, max_iterations=15):
    """the restated solve with its margins and its one-ulp condition, or None"""
    try:
        res = tr.restate(c, max_iterations)
        tr.assert_margins(name, res[3])
        floor, _ = tr.noise_floor(name, lambda: tr.restate(tr.gap_one_ulp_up(c), max_iterations)[2:4], res[2:4])
    except AssertionError:
        return None
    return res[3], floor


def push_trial(seed, sizes=SIZES, decades=(0.0, 6.0)):
    rng = np.random.RandomState(100000 + seed)
    N = int(sizes[rng.randint(len(sizes))])
    length = 10.0 ** rng.uniform(*decades)
    d = rng.randn(3)
    d = d / np.linalg.norm(d) * length
    jump = (r4(d[0]), r4(d[1]), r4(d[2]), r4(rng.uniform(0.0, 3.1)))
    kw = dict(seed=seed, n_frames=N, samples_per_segment=1, right_jump=jump)
    c = tr.make_gap(**kw)
    out = judged(str(seed), c)
    if out is None:
        return None
    s, floor = out
    line = dict(kw=kw, term=s["termination"], iterations=s["iterations"], accepted=s["successful_steps"], census=sorted(set(map(tuple, s["census"]))),
                first=s["dogleg"][0]["branch"] if s["dogleg"] else None, c_positive=all(r["c"] > 0 for r in s["dogleg"] if r["branch"] == "interp"), floor=floor)
    if s["termination"] == np_ceres.NO_CONVERGENCE:
        out = judged(str(seed), c, 32)
        if out is not None and out[0]["termination"] == np_ceres.NO_CONVERGENCE and out[0]["iterations"] == 32:
            line["at_32"] = dict(accepted=out[0]["successful_steps"], last_accepted=bool(out[0]["accepted_mask"] >> 31), floor=out[1])
    return line


def resolve_trial(seed):
    """a stored gap solved again between a left keyframe row and a right one moved by metres to tens of metres and up to 2.5 rad (even seeds; the
    interpolated branch arises there) or by 1e4 .. 3e5 m (odd seeds; below that the Gauss-Newton step never leaves the initial radius of 1e4 far enough
    behind for the Cauchy branch)"""
    rng = np.random.RandomState(200000 + seed)
    N = int(SIZES[rng.randint(len(SIZES))])
    d = rng.randn(3)
    d = d / np.linalg.norm(d) * (rng.uniform(2.0, 40.0) if seed % 2 == 0 else 10.0 ** rng.uniform(4.0, 5.5))          # the Cauchy branch needs the far ones
    jump = (r4(d[0]), r4(d[1]), r4(d[2]), r4(rng.uniform(0.1, 2.5)))
    spec = dict(seed=seed, n_frames=N, kind="closure", jump=jump)
    try:
        g = tr.resolve_gap(spec, np.array([0.3, -0.2, 0.1, 1.0, 0, 0, 0]))
        tr.assert_margins(str(seed), g["summary"])
        floor, _ = tr.noise_floor(str(seed), lambda: tr.resolve_restated(g, ulp=True), (g["poses"], g["summary"]))
    except AssertionError:
        return None
    s = g["summary"]
    return dict(spec=spec, term=s["termination"], iterations=s["iterations"], census=sorted(set(map(tuple, s["census"]))), floor=floor)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "push"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    for seed in range(n):
        if what == "far":
            line = push_trial(1000 + seed, (10, 18, 19, 27, 28, 32), (4.3, 6.0))
        else:
            line = push_trial(seed) if what == "push" else resolve_trial(seed)
        if line is not None:
            print(json.dumps(line), flush=True)

"""One steady-state window (W = 20, 256 points per keyframe, GNSS, the prior of the device's own marginalization) solved with the new ends of the
solve (GLIO_SOLVE_ENDS at its default: no staging launch, the result published from LDS) and with the old ones (0: k_stage_in, finalize()), from
the given start and from a far one whose steps are mostly rejected.  Prints one JSON line with a hash per solve.  The helper switches
(GLIO_CHAIN_HELPERS, GLIO_CHAIN_FAT) are read once per process: tests/test_hip_solve_ends.py runs this file under each of them and compares the
hashes with those of run() in its own process."""
import copy
import ctypes as C
import hashlib
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from glio_amd import synth, capi  # noqa: E402


def digest(sol, summ):
    h = hashlib.sha256()
    for a in (sol.trans, sol.quat, sol.speed_bias, sol.rcv_ddt[:sol.n_ddt]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(json.dumps(summ.as_dict(), sort_keys=True).encode())
    return h.hexdigest()[:16]


def run(W=20, pts=256):
    lib = capi.load()
    stream = synth.make_window(W=W + 1, pts_per_scan=pts, with_gnss=True, seed=synth.SEED_BASE + 320)
    first = synth.sub_window(stream, 0, W)
    c0 = capi.Context(first.opts)
    c0.load_window(first, synth.analytic_correspondences(first))
    s0, _ = c0.solve(first.init)
    prior = c0.marginalize(s0)
    c0.close()
    win = synth.sub_window(stream, 1, W)
    win.prior = prior
    corr = synth.analytic_correspondences(win)
    far = win.init.copy()
    far.trans = far.trans + np.random.default_rng(5).normal(0, 0.4, far.trans.shape)
    opts2 = copy.copy(win.opts)
    opts2.min_relative_decrease, opts2.max_iterations = 1.05, 30
    new = lib.glio_debug_solve_ends(0)          # (returns what was set: the default, every new path on)
    out = {"helpers": os.environ.get("GLIO_CHAIN_HELPERS"), "fat": os.environ.get("GLIO_CHAIN_FAT"), "new_mask": new}
    try:
        for name, mask in (("new", new), ("old", 0)):
            lib.glio_debug_solve_ends(mask)
            ctx = capi.Context(win.opts)
            ctx.load_window(win, corr)
            hashes = [digest(*ctx.solve(st)) for st in (win.init, far, win.init)]
            stamps = (C.c_longlong * 320)()
            lib.glio_debug_arrow_stamps(ctx._h, stamps)
            path = int(lib.glio_debug_solver_path(ctx._h))
            ctx.close()
            ctx = capi.Context(opts2)
            ctx.load_window(win, corr)
            sol, summ = ctx.solve(far)
            hashes.append(digest(sol, summ))
            ctx.close()
            out[name] = {"hashes": hashes, "fat_steps": int(stamps[300]), "path": path, "rejected": int(summ.iterations - summ.successful_steps)}
    finally:
        lib.glio_debug_solve_ends(new)
    return out


if __name__ == "__main__":
    print(json.dumps(run()))

"""One round of the association's timings, for A/B runs of two builds of the library (GLIO_HIP_LIB selects one; a fresh process per build and round): one JSON
line.  Every figure after its own warm-up; a figure is the median of several timings.
  map_build_us, associate_scan_us   K1 of the C2 map and the lone-scan association of slot 0, device events (glio_assoc_time_hooks, 10 repetitions; 5 timings)
  window_one_call_ms                the one-call window association of the C2 window (20 x 65536 queries), wall time of the call (9 timings)
  bassoc_12_pairs_ms                a keyframe call's batch association: the newest of 16 keyframes of 32768 points against its 6 predecessors, both directions,
                                    wall time of glio_bassoc_run_append (9 timings; the object is reset in between)
  keyframe_cycle_ms                 bench.py's keyframe_pipeline (replay of one keyframe: slide, local map, association, factors, solve, marginalisation)
    GLIO_HIP_LIB=<library> python scripts/assoc_speed_ab.py [bassoc]        (bassoc: that figure alone)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from glio_amd import batch, capi, synth
import bench

W, PTS = 20, 65536
ONLY_BASSOC = sys.argv[1:] == ["bassoc"]
out = {"lib": os.path.basename(os.environ.get("GLIO_HIP_LIB", "libglio_hip.so"))}
if not ONLY_BASSOC:
    stream = synth.make_window(W=W + 1, pts_per_scan=PTS, with_gnss=True, with_prior=False, seed=synth.SEED_BASE)
    win = synth.sub_window(stream, 1, W)
    ctx = capi.Context(win.opts)
    ctx.set_map(win.map_pts)
    for s in range(W):
        ctx.set_scan(s, win.scans[s])
    poses = [capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s]) for s in range(W)]
    q2s, t2s = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    for _ in range(3):
        ctx.associate_window(q2s, t2s)
    tw = []
    for _ in range(9):
        t0 = time.perf_counter(); ctx.associate_window(q2s, t2s); tw.append(time.perf_counter() - t0)
    out["window_one_call_ms"] = round(float(np.median(tw)) * 1e3, 4)
    ctx.time_kernel(capi.KERNEL_ASSOCIATE, 10); ctx.time_kernel(capi.KERNEL_MAP_BUILD, 10)
    out["associate_scan_us"] = round(float(np.median([ctx.time_kernel(capi.KERNEL_ASSOCIATE, 10) for _ in range(5)])) * 1e3, 2)
    out["map_build_us"] = round(float(np.median([ctx.time_kernel(capi.KERNEL_MAP_BUILD, 10) for _ in range(5)])) * 1e3, 2)
    ctx.close()

K, BP, SR = 16, 32768, 6
bw = synth.make_window(W=K, pts_per_scan=BP, seed=synth.SEED_BASE + 61, perturb=(0.03, 0.2, 0.0), scan_radius=25.0, map_density=0.5)
tlb = np.array(bw.opts.t_lb, np.float32)
bposes = np.c_[bw.init.trans, bw.init.quat]
prev = np.arange(K - 1 - SR, K - 1, dtype=np.int32); new = np.full(SR, K - 1, np.int32)
ci, cj = np.r_[new, prev], np.r_[prev, new]
ba = batch.BatchAssociation(K, BP, 12 * BP)
for k in range(K):
    sc = bw.scans[k].copy(); sc[:, :3] -= tlb
    ba.set_frame(k, sc)
tb = []
for r in range(12):
    ba.reset()
    t0 = time.perf_counter(); ba.run_append(bposes, ci, cj); dt = time.perf_counter() - t0
    if r >= 3:
        tb.append(dt)
out["bassoc_12_pairs_ms"] = round(float(np.median(tb)) * 1e3, 4)
ba.close()

if not ONLY_BASSOC:
    bench.bench_keyframe_pipeline(0, stream, W)
    out["keyframe_cycle_ms"] = round(float(np.median([bench.bench_keyframe_pipeline(0, stream, W)["cycle_ms"] for _ in range(3)])), 4)
print(json.dumps(out))

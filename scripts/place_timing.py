"""What place recognition costs (glio_place_*), measured, nothing gated: medians of 10 by HIP events (glio_place_last_device_ms) into
profiles/place_timing.json.

Expectations, stated before measuring and recorded as MET / NOT MET:
  * one query against 3 500 places costs less than the released keyframe call (0.64 ms) and less than one glio_loop_align timed in the same session;
  * the all-pairs call (every one of 3 500 places against all earlier ones) is reported as a fraction of the MFMA issue bound -- 80 v_mfma_f32_16x16x4_f32
    issues (163 840 flop) per pair at 155 TF fp32; whatever is left is the diagonal pass through LDS, the operand loads and the selection.
Context only: the numpy restatement's time for one pair on the measuring host.

    python scripts/place_timing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from glio_amd import batch, loop, place          # noqa: E402

KEYFRAME_CALL_MS = 0.64
MFMA_TF, FLOP_PER_PAIR = 155.0, 64 * 64 * 20 * 2


def med(fn, ms, reps=10):
    out = []
    for _ in range(reps):
        fn()
        out.append(ms())
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), reps=reps)


def main():
    rng = np.random.default_rng(1)
    clouds = [np.c_[rng.uniform(-70, 70, (n, 2)), rng.uniform(-2, 6, n), np.zeros(n)].astype(np.float32) for n in (4096, 57344)]
    ba = batch.BatchAssociation(2, 57344, 16)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    import torch
    prop = torch.cuda.get_device_properties(0)
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "what": "medians of 10, HIP events"}
    pr = place.PlaceRecognition(ba, max_places=65536)
    out["add_frames_4k_points"] = med(lambda: pr.add_frames([0], [0], [0.0]), pr.last_device_ms)
    out["add_frames_57k_points"] = med(lambda: pr.add_frames([1], [0], [0.0]), pr.last_device_ms)
    # a store of distinct descriptors: random heights through glio_place_set_descriptor would take 65 536 calls; the pair kernel's time does not depend on the
    # values, so the two resident frames are described alternately in ONE launch
    for n_places in (3500, 65536):
        pr.clear()
        idx = np.arange(n_places, dtype=np.int32)
        pr.add_frames(idx % 2, idx, idx.astype(np.float64))
        out[f"add_frames_{n_places}_frames_one_launch_ms"] = pr.last_device_ms()
        out[f"query_one_against_{n_places}"] = med(lambda: pr.query(n_places - 1, 1.5, 8), pr.last_device_ms)
        if n_places == 3500:
            r = med(lambda: pr.query_many(0, n_places, 1.5, True, 8), pr.last_device_ms)
            pairs = sum(max(0, q - 1) for q in range(n_places))          # earlier places more than 1.5 away in time
            bound_ms = pairs * FLOP_PER_PAIR / (MFMA_TF * 1e12) * 1e3
            r.update(pairs=pairs, mfma_issue_bound_ms=bound_ms, fraction_of_mfma_issue_bound=bound_ms / r["median_ms"])
            out["query_many_3500_against_all_earlier"] = r
    pr.close()
    # one glio_loop_align in the same session
    import loop_restated as lr
    src, tgt, _ = lr.known_answer_case()
    lp = loop.LoopClosure(ba)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    out["loop_align_same_session"] = med(lp.align, lp.last_device_ms)
    lp.close(); ba.close()
    q = out["query_one_against_3500"]["median_ms"]
    out["expectations"] = {
        "query_3500_below_keyframe_call_0.64_ms": "MET" if q < KEYFRAME_CALL_MS else "NOT MET",
        "query_3500_below_one_loop_align": "MET" if q < out["loop_align_same_session"]["median_ms"] else "NOT MET",
    }
    # context: the numpy restatement, one pair
    import place_restated as R
    u = rng.uniform(0, 1, (R.RINGS, R.SECTORS)).astype(np.float32)
    t0 = time.perf_counter()
    for _ in range(20):
        R.pair(u, R.MASK60, u, R.MASK60)
    out["numpy_restatement_one_pair_ms_host"] = (time.perf_counter() - t0) / 20 * 1e3
    path = os.path.join(ROOT, "profiles", "place_timing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

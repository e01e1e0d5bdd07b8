"""What the static map costs (glio_static_*), measured, nothing gated: medians of 10 by HIP events (glio_static_last_device_ms, glio_gmap_last_device_ms)
into profiles/static_map_timing.json.

Two cases: 51 and 667 dense frames of a 32-line, 57.6 k-point scan (32 x 1800 rays inside a hall, the sensor on a 5 m circle, 0.5 m per frame) with the views
static_views(poses, 6) picks (12 per frame away from the ends).  Beside each, glio_gmap_add_frames of the same frames in the same session, and a byte model of
the vote kernel: every point read once (16 B) and its two counts written (2 B), every floor image read once (4 B per cell).

Expectations, stated before measuring and recorded as MET / NOT MET with the figures:
  * classifying costs less than building the map of the same frames;
  * the vote kernel reaches at least half of the byte model's rate, the model's bytes at 6.3 TB/s (what a float4 copy achieves on this part).

    python scripts/static_map_timing.py [--frames 51 667]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from glio_amd import mapping, static_map          # noqa: E402

LINES, AZIMUTHS = 32, 1800
HBM_TBS = 6.3
HALL_LO, HALL_HI = np.array([-35.0, -12.0, -1.8]), np.array([35.0, 12.0, 6.0])


def scan_at(pose):
    """32 x 1800 rays from the pose (t, yaw about z) to the inside of the hall: every ray returns"""
    el = np.deg2rad(-25.5 + np.arange(LINES))
    az = 2 * np.pi * (np.arange(AZIMUTHS) + 0.5) / AZIMUTHS
    E, A = np.meshgrid(el, az, indexing="ij")
    dl = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    yaw = 2.0 * np.arctan2(pose[6], pose[3])
    c, s = np.cos(yaw), np.sin(yaw)
    d = dl @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (HALL_HI - pose[:3]) / d, np.where(d < 0, (HALL_LO - pose[:3]) / d, np.inf)).min(axis=1)
    return np.ascontiguousarray(np.c_[dl * t[:, None], np.repeat(np.arange(LINES), AZIMUTHS)].astype(np.float32))


def circle_poses(n):
    a = 0.5 * np.arange(n) / 5.0
    yaw = a + np.pi / 2
    return np.c_[5.0 * np.cos(a), 5.0 * np.sin(a), np.zeros(n), np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)]


def med(fn, ms, reps=10):
    rows = []
    for _ in range(reps):
        fn()
        rows.append(ms())
    rows = np.array(rows, np.float64)
    return dict(median_ms=np.median(rows, axis=0).tolist(), min_ms=rows.min(axis=0).tolist(), max_ms=rows.max(axis=0).tolist(), reps=reps)


def case(n_frames):
    poses = circle_poses(n_frames)
    n_pts = LINES * AZIMUTHS
    dense = mapping.DenseClouds(n_frames, n_pts, n_pts)
    for k in range(n_frames):
        assert dense.set_frame(k, scan_at(poses[k]), 0.0) == n_pts
    off, views = static_map.static_views(poses, 6)
    st = static_map.StaticClouds(dense)
    frames = np.arange(n_frames, dtype=np.int32)
    info = st.classify(frames, poses, off, views)
    out = dict(frames=n_frames, points=info.n_points, views=int(len(views)), views_per_frame=len(views) / n_frames, tested=info.n_tested, dynamic=info.n_dynamic,
               lds_path=info.lds_path)
    r = med(lambda: st.classify(frames, poses, off, views), st.last_device_ms)
    stages = dict(zip(("images", "floor", "votes", "compaction"), r["median_ms"]))
    out["classify_stage_median_ms"] = stages
    out["classify_median_ms"] = float(sum(r["median_ms"]))
    out["classify_min_max_ms"] = [float(sum(r["min_ms"])), float(sum(r["max_ms"]))]
    cells = st.rows * st.cols
    model = info.n_points * 18 + n_frames * cells * 4
    out["vote_byte_model"] = dict(bytes=int(model), at_tb_per_s=HBM_TBS, model_ms=model / (HBM_TBS * 1e12) * 1e3,
                                  fraction_of_model_rate=(model / (HBM_TBS * 1e12) * 1e3) / stages["votes"],
                                  point_view_pairs_per_us=float(sum((off[f + 1] - off[f]) * n_pts for f in range(n_frames)) / (stages["votes"] * 1e3)))
    gm = mapping.GlobalMap(dense, mapping.default_opts(max_voxels=1 << 23, max_points_per_add=n_frames * n_pts))

    def add():
        gm.clear()
        gm.add(frames, poses)
    g = med(add, gm.last_device_ms)
    out["gmap_add_frames_same_frames"] = dict(median_ms=g["median_ms"], min_ms=g["min_ms"], max_ms=g["max_ms"], voxels=gm.size())
    out["expectations"] = {
        "classify_below_map_of_same_frames": "%s (%.3f ms against %.3f ms)" % ("MET" if out["classify_median_ms"] < g["median_ms"] else "NOT MET", out["classify_median_ms"],
                                                                              g["median_ms"]),
        "votes_at_least_half_the_byte_models_rate": "%s (%.3f of it)" % ("MET" if out["vote_byte_model"]["fraction_of_model_rate"] >= 0.5 else "NOT MET",
                                                                         out["vote_byte_model"]["fraction_of_model_rate"]),
    }
    gm.close(); st.close(); dense.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[51, 667])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_map_timing.json"))
    a = ap.parse_args()
    import torch
    prop = torch.cuda.get_device_properties(0)
    out = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "what": "medians of 10, HIP events; a 32 x 1800 scan per frame, 6 views on either side"}
    for n in a.frames:
        out["frames_%d" % n] = case(n)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The places of the end-to-end place-recognition tests: one spinning-LiDAR scan (synth_lidar.make_scan) in a synth.make_scene scene of its own seed and size
per place, and a revisit of it from up to 0.5 m away with an arbitrary heading.  Everything follows from the seed; scripts/search_place_cases.py decides which
seeds are kept (tests/golden/place_scenes.json).  CPU only."""
import json
import math
import os

import numpy as np

from glio_amd import synth, synth_lidar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "place_scenes.json")
N_SCANS, N_AZ = 16, 360


def parameters(seed):
    """scene size, sensor position, the revisit's offset (<= 0.5 m) and heading -- all from the seed.  Every fourth seed revisits with a heading near 90 deg."""
    rng = np.random.default_rng(seed)
    length, width, height = rng.uniform(60, 200), rng.uniform(12, 40), rng.uniform(8, 20)
    n_boxes = int(rng.integers(8, 31))
    origin = np.array([rng.uniform(0.3, 0.7) * length, rng.uniform(-0.25, 0.25) * width, 1.8])
    r, a = rng.uniform(0.1, 0.5), rng.uniform(0, 2 * math.pi)
    yaw = rng.uniform(0, 2 * math.pi)
    if seed % 4 == 0:
        yaw = math.radians(rng.uniform(80, 100))
    return dict(seed=int(seed), length=length, width=width, height=height, n_boxes=n_boxes, origin=origin, offset=np.array([r * math.cos(a), r * math.sin(a), 0.0]), yaw=yaw)


def _scan(p, origin, start_az, seed):
    scene = synth.make_scene(p["length"], p["width"], p["height"], p["n_boxes"], seed=p["seed"])
    s = synth_lidar.make_scan(N_SCANS, N_AZ, origin=origin, start_az=start_az, scene=scene, seed=seed, close_frac=0.0, max_range=100.0)
    return np.ascontiguousarray(s[np.all(np.isfinite(s[:, :3]), axis=1)], np.float32)


def place_scan(p):
    """the place: sensor axes along the world's, [n][4] float32 without the misses"""
    return _scan(p, p["origin"], 0.7, p["seed"])


def revisit_scan(p):
    """the same place from origin + offset with the sensor's heading turned by yaw: p_sensor = Rz(-yaw) p_world_aligned"""
    s = _scan(p, p["origin"] + p["offset"], 0.7 + p["yaw"], p["seed"] + 100000)
    c, sn = math.cos(p["yaw"]), math.sin(p["yaw"])
    x, y = s[:, 0].astype(np.float64), s[:, 1].astype(np.float64)
    out = s.copy()
    out[:, 0] = (c * x + sn * y).astype(np.float32)
    out[:, 1] = (-sn * x + c * y).astype(np.float32)
    return out


def kept():
    """the golden list: dict(seeds, align_seed, yaw_error_restated {seed: rad}, ...)"""
    with open(GOLDEN) as f:
        return json.load(f)


def angle_diff(a, b):
    return abs((a - b + math.pi) % (2 * math.pi) - math.pi)

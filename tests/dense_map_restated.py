"""What the dense map's tests need beside the existing restatements -- TEST INFRASTRUCTURE ONLY.  A dense frame IS keyframe_cloud_restated.keyframe_cloud(pts, leaf,
trans, quat) and the map IS global_map_restated.restated_voxel_grid; this file adds

  world_cloud(pts, trans, quat, pose)   pub_full_cloud_map (LidarOdometry.cpp:645-658): the de-skewed, UNFILTERED cloud moved by transformCloud (Estimator.cpp:1517-1546:
                                        double q * v + t in Eigen's order, stored as float) at pose = t[3], q[4] (w first)
  move(pts, pose)                       transformCloud alone (what the map does to a frame)
  wave_constants()                      the #defines of the wavefront-per-long-list emit (glio_amd/csrc/localmap_kernels.hip, LM_WAVE_*)
  one_voxel_cloud(n), long_list_cloud() the case builders; tests/test_dense_map_restated.py holds them to what they claim
"""
import os
import re

import numpy as np

import keyframe_cloud_restated as kr
from preproc_restated import F, _qrot

LEAF = 0.4                      # ds_filter_surf_map (Estimator.cpp:854)
BASE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)


def move(pts, pose):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    t = [float(v) for v in pose[:3]]
    q = tuple(float(v) for v in pose[3:7])
    out = pts.copy()
    for i in range(len(pts)):
        o = _qrot(q, [float(pts[i, 0]), float(pts[i, 1]), float(pts[i, 2])])
        for k in range(3):
            out[i, k] = F(o[k] + t[k])
    return out


def world_cloud(pts, trans, quat, pose):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    return move(pts.copy() if trans is None else kr.deskew(pts, trans, quat), pose)


def wave_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glio_amd", "csrc", "localmap_kernels.hip")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (LM_WAVE_[A-Z_]+) (\d+)\b", src)}


def one_voxel_cloud(n, seed=7, corner=(40.0, 40.0, 40.0)):
    """n points uniform in corner + [0, 0.39)^3 -- inside ONE voxel of the 0.4 m grid when the corner is a multiple of 0.4 -- with intensities in [0, 31.09)"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(corner)[None, :] + rng.uniform(0.0, 0.39, (n, 3))
    return np.ascontiguousarray(np.c_[xyz, rng.uniform(0.0, 31.09, n)].astype(np.float32))


def list_sizes():
    """the list lengths of long_list_cloud: the fixed ones and every LM_WAVE_* constant at -1, +0, +1"""
    sizes = list(BASE_SIZES)
    for c in sorted(wave_constants().values()):
        for s in (c - 1, c, c + 1):
            if s >= 1 and s not in sizes:
                sizes.append(s)
    return sizes


def long_list_cloud(seed=13):
    """one cloud whose voxels (0.4 m) hold list_sizes() points, voxel i at corner (8 i, 4 (i % 3), -4 (i % 2)) (multiples of 0.4 in float as in double: 8 = 20 x 0.4
    is held to the cell by the test), the points shuffled so that no list is contiguous in the input -> cloud, sizes, voxel id per point"""
    sizes = list_sizes()
    parts, ids = [], []
    for i, n in enumerate(sizes):
        parts.append(one_voxel_cloud(n, seed=100 + i, corner=(8.0 * i, 4.0 * (i % 3), -4.0 * (i % 2))))
        ids.append(np.full(n, i))
    pts, ids = np.vstack(parts), np.concatenate(ids)
    perm = np.random.default_rng(seed).permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), sizes, ids[perm]

"""CPU checks of the dense map's case builders (tests/dense_map_restated.py): they are what tests/test_hip_dense_map.py takes them for.  Above all: a one-voxel
cloud of 64 points or more has a float sum that DEPENDS on the order of its additions -- the restatement of the reversed cloud differs in at least one bit -- so a
kernel that summed a long list in another order could not pass the byte comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_map_restated as dr  # noqa: E402
import global_map_restated as gr  # noqa: E402
import keyframe_cloud_restated as kr  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [64, 65, 129, 4097])
def test_one_voxel_sum_depends_on_the_order(n):
    c = dr.one_voxel_cloud(n)
    a, b = kr.keyframe_cloud(c, dr.LEAF), kr.keyframe_cloud(c[::-1], dr.LEAF)
    assert a.shape == b.shape == (1, 4)
    assert not np.array_equal(_bits(a), _bits(b))


def test_one_voxel_cloud_is_one_voxel_of_both_restatements():
    c = dr.one_voxel_cloud(4097)
    assert len(np.unique(gr.voxel_keys(c, dr.LEAF))) == 1
    a = kr.keyframe_cloud(c, dr.LEAF)
    b, _ = gr.restated_voxel_grid(c, dr.LEAF)
    assert np.array_equal(_bits(a), _bits(b))                  # the oracle's VoxelGrid and the map's restatement sum alike


def test_wave_constants_are_read_and_enter_the_sizes():
    k = dr.wave_constants()
    assert set(k) >= {"LM_WAVE_VOX", "LM_WAVE_LIST_MIN", "LM_WAVE_LIST_LDS"} and all(v >= 1 for v in k.values())
    assert k["LM_WAVE_LIST_MIN"] < k["LM_WAVE_LIST_LDS"]
    sizes = dr.list_sizes()
    for v in k.values():
        assert {v - 1, v, v + 1} - {0} <= set(sizes)
    assert set(dr.BASE_SIZES) <= set(sizes) and len(set(sizes)) == len(sizes)


def test_long_list_cloud_is_what_it_claims():
    pts, sizes, ids = dr.long_list_cloud()
    assert len(pts) == sum(sizes) and 15000 < len(pts) <= 20480
    keys = gr.voxel_keys(pts, dr.LEAF)
    # one voxel per list, the lists as long as claimed
    assert len(np.unique(keys)) == len(sizes)
    for i, n in enumerate(sizes):
        assert len(np.unique(keys[ids == i])) == 1 and int((ids == i).sum()) == n
    # no list of two points or more is contiguous in the input
    for i, n in enumerate(sizes):
        if n >= 2:
            where = np.flatnonzero(ids == i)
            assert where[-1] - where[0] + 1 > n, (i, n)
    # the restatements agree on it, voxel by voxel, and every long list's sum depends on the order
    a = kr.keyframe_cloud(pts, dr.LEAF)
    b, _ = gr.restated_voxel_grid(pts, dr.LEAF)
    assert a.shape == (len(sizes), 4) and np.array_equal(_bits(a), _bits(b))
    r = kr.keyframe_cloud(pts[::-1], dr.LEAF)
    differ = (_bits(a) != _bits(r)).any(axis=1)
    order = np.argsort([gr.voxel_keys(pts[ids == i][:1], dr.LEAF)[0] for i in range(len(sizes))])
    for row, i in enumerate(order):
        if sizes[i] >= 64:
            assert differ[row], sizes[i]


def test_world_cloud_and_move():
    tab = kr.intensity_table()
    ident = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    assert np.array_equal(_bits(dr.move(tab, ident)), _bits(tab))
    trans = (0.6, -0.05, 0.02)
    assert np.array_equal(_bits(dr.world_cloud(tab, trans, None, ident)), _bits(kr.deskew(tab, trans)))
    pose = gr.pose_at(3.0, -2.0, 0.5, 0.3)
    w = dr.world_cloud(tab, trans, None, pose)
    d = kr.deskew(tab, trans)
    c, s = np.cos(0.3), np.sin(0.3)
    want = np.c_[c * d[:, 0] - s * d[:, 1] + 3.0, s * d[:, 0] + c * d[:, 1] - 2.0, d[:, 2] + 0.5]
    assert np.abs(w[:, :3] - want).max() < 1e-5 and np.array_equal(_bits(w[:, 3]), _bits(tab[:, 3]))

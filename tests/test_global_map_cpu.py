"""CPU: the rules the global map (glio_gmap_*, include/glio_hip.h) is built on, shown with the oracle alone -- a stable sort by the ABSOLUTE 63-bit voxel key and
sequential float32 sums reproduce pcl::VoxelGrid as the oracle restates it, bit for bit, on every case tests/test_hip_global_map.py runs on the device (the far case's
linear index passes 2^31: the key needs no bounding box); appending to a voxel's stored sum point by point equals a rebuild, adding a partial sum does not; and
glio::globalMapFrames (host/glio_map_backend.hpp) equals mapping.global_map_frames."""
import os
import subprocess

import numpy as np
import pytest

import global_map_restated as gr


def _moved(clouds, frames, poses):
    from oracle import pyoracle as po
    return np.vstack([po.transform_cloud(clouds[f], p[3:], p[:3]) for f, p in zip(frames, poses)])


@pytest.fixture(scope="module")
def window():
    return gr.window_case()


def _same(pts, leaf):
    from oracle import pyoracle as po
    want, _ = po.voxel_grid(pts, leaf)
    got, _ = gr.restated_voxel_grid(pts, leaf)
    assert len(got) == len(want) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return want


@pytest.mark.parametrize("leaf", [0.2, 0.4])
@pytest.mark.parametrize("frames", [[2, 3, 4, 5], [5, 2, 4, 3]], ids=["asc", "mixed"])
def test_restatement_equals_the_oracle_on_the_window(window, frames, leaf):
    clouds, _, new = window
    _same(_moved(clouds, frames, new[frames]), leaf)


def test_order_changes_the_sums_and_poses_change_the_map(window):
    from oracle import pyoracle as po
    clouds, old, new = window
    a = po.voxel_grid(_moved(clouds, [2, 3, 4, 5], new[[2, 3, 4, 5]]), 0.4)[0]
    b = po.voxel_grid(_moved(clouds, [5, 2, 4, 3], new[[5, 2, 4, 3]]), 0.4)[0]
    assert len(a) == len(b) and not np.array_equal(a, b)          # the frames overlap: the same voxels, other float sums
    c = po.voxel_grid(_moved(clouds, [2, 3, 4, 5], old[[2, 3, 4, 5]]), 0.4)[0]
    assert len(c) != len(a) or not np.array_equal(a, c)


def test_restatement_equals_the_oracle_on_the_extent_cases(window):
    from oracle import pyoracle as po
    clouds, _, new = window
    faces = gr.faces_cloud()
    assert (faces[:, :3] < 0).any()
    for leaf in (0.2, 0.4):
        _same(po.transform_cloud(faces, gr.IDENTITY[3:], gr.IDENTITY[:3]), leaf)
    assert np.array_equal(po.transform_cloud(faces, gr.IDENTITY[3:], gr.IDENTITY[:3]), faces)          # (the identity pose is exact: the points ARE on faces)
    fc, fp = gr.far_case()
    far = _moved(fc, [0, 1, 2], fp)
    assert gr.box_cells(far, 0.2) > 2 ** 31 - 1
    want = _same(far, 0.2)
    assert 0.9 * len(far) < len(want) < len(far)                 # sparse clouds: nearly a voxel per point, some shared by the two overlapping clouds
    one, pose = gr.one_voxel_case()
    assert len(_same(po.transform_cloud(one, pose[3:], pose[:3]), 0.2)) == 1
    frames, poses = gr.ring_case()
    assert len(frames) == 80 and len(set(frames)) == gr.K
    _same(_moved(clouds, frames, poses), 0.2)


def test_appending_point_by_point_equals_a_rebuild_and_a_partial_sum_does_not(window):
    """why k_gm_accum continues the stored sum one point at a time"""
    clouds, _, new = window
    first, second = _moved(clouds, [2, 3], new[[2, 3]]), _moved(clouds, [4, 5], new[[4, 5]])
    whole, keys = gr.restated_voxel_grid(np.vstack([first, second]), 0.4)
    k1, k2 = gr.voxel_keys(first, 0.4), gr.voxel_keys(second, 0.4)
    acc, cnt = {}, {}
    for k, p in zip(k1.tolist(), first):
        acc[k] = acc.get(k, np.zeros(4, np.float32)) + p; cnt[k] = cnt.get(k, 0) + 1
    part = {}
    for k, p in zip(k2.tolist(), second):
        part[k] = part.get(k, np.zeros(4, np.float32)) + p
    lump = {k: acc.get(k, np.zeros(4, np.float32)) + v for k, v in part.items()}          # old + (sum of new)
    for k, p in zip(k2.tolist(), second):                                                    # old, then the new points one at a time
        acc[k] = acc.get(k, np.zeros(4, np.float32)) + p; cnt[k] = cnt.get(k, 0) + 1
    seq = np.array([acc[k] / np.float32(cnt[k]) for k in keys.tolist()], np.float32)
    assert np.array_equal(seq.view(np.uint32), whole.view(np.uint32))
    differs = sum(not np.array_equal(lump[k], acc[k]) for k in lump)
    assert differs > 0


def test_sort_constants_are_what_the_gpu_test_names():
    c = gr.sort_constants()
    assert {"GM_SORT_TILE", "GM_SCAN_CHUNK", "GM_RUN_BLOCK", "GM_TOP_THREADS", "GM_TF_THREADS", "GM_TF_PER"} <= set(c)


def test_cpp_global_map_frames_equals_python(tmp_path):
    from glio_amd import mapping
    here = os.path.join(os.path.dirname(os.path.abspath(mapping.__file__)), "host")
    exe = str(tmp_path / "host_map_mirror_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", os.path.join(here, "host_map_mirror_test.cpp"), "-I" + os.path.join(here, "..", "..", "include"), "-o", exe])
    cases = [(k, m) for k in range(13) for m in range(1, 5)]
    out = subprocess.run([exe], input="".join(f"{k} {m}\n" for k, m in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (k, m), ln in zip(cases, out):
        assert [int(x) for x in ln.split()[1:]] == mapping.global_map_frames(k, m), (k, m)
    assert mapping.global_map_frames(7, 3) == [0, 3, 6] and mapping.global_map_frames(0, 3) == []


def test_struct_layouts_match():
    import ctypes as C
    from glio_amd import build, capi
    from glio_amd import ctypes_types as T
    build.build()
    lib = capi.load()
    out = (C.c_int32 * 2)()
    assert lib.glio_gmap_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioGmapOpts), C.sizeof(T.GlioGmapInfo)]
    assert lib.glio_abi_version() == 5
    o = mapping_default_opts()
    assert abs(o.leaf - 0.2) < 1e-7 and o.max_voxels > 0 and o.max_points_per_add > 0


def mapping_default_opts():
    from glio_amd import mapping
    return mapping.default_opts()

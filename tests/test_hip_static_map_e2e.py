"""GPU, end to end: the street of tests/static_map_cases.py (ground, two walls, a building across the end, a car-sized box that crosses the road ahead of a
sensor that drives along; 8 scans of 16 lines x 225 azimuths) through a dense store, glio_static_classify with the default options and the views static_views
picks, and glio_gmap_create_on_static at 0.2 m.  The device equals the restatement bit for bit, the map over the static store equals restated_voxel_grid of the
kept points moved to the world, and the car's trail thins out."""
import numpy as np
import pytest

import static_map_cases as Cs
import static_map_restated as R
from dense_map_restated import move
from global_map_restated import restated_voxel_grid

pytestmark = pytest.mark.gpu

CAP = 4096


@pytest.fixture(scope="module")
def world():
    from glio_amd import capi, mapping, static_map
    clouds, poses, labels = Cs.street()
    dense = mapping.DenseClouds(Cs.STREET_FRAMES, CAP, CAP)
    for k, c in enumerate(clouds):
        assert dense.set_frame(k, c, 0.0) == len(c)
    st = static_map.StaticClouds(dense)
    off, views = static_map.static_views(poses, Cs.HALF_WINDOW)
    assert np.array_equal(off, Cs.street_call(poses)[0]) and np.array_equal(views, Cs.street_call(poses)[1])
    info = st.classify(list(range(Cs.STREET_FRAMES)), poses, off, views)
    P = R.Params()
    tab = capi.static_tables(st.opts)
    rel = R.relative_poses(poses, off, views, capi.static_relative_pose)
    want, images = R.classify(clouds, rel, off, views, tab[0], tab[1], P)
    yield dict(clouds=clouds, poses=poses, labels=labels, dense=dense, st=st, off=off, info=info, want=want, images=images)
    st.close(); dense.close()


def test_the_device_equals_the_restatement_bit_for_bit(world):
    st, want = world["st"], world["want"]
    assert world["info"].lds_path and world["info"].n_points == sum(len(c) for c in world["clouds"])
    for k in range(Cs.STREET_FRAMES):
        th, te = st.read_votes(k)
        assert np.array_equal(th, want[k]["through"]) and np.array_equal(te, want[k]["tested"]), k
        kept = st.read_frame(k)
        assert kept.shape == want[k]["kept"].shape and np.array_equal(kept.view(np.uint32), want[k]["kept"].view(np.uint32)), k
        raw, fl = st.read_image(k)
        assert np.array_equal(raw.view(np.uint32), world["images"][k][0].view(np.uint32)) and np.array_equal(fl.view(np.uint32), world["images"][k][1].view(np.uint32)), k
    assert world["info"].n_dynamic == sum(int(w["dynamic"].sum()) for w in want) and world["info"].n_tested == sum(int((w["tested"] > 0).sum()) for w in want)


def test_the_scenes_conditions_hold_on_the_device(world):
    st, labels, off = world["st"], world["labels"], world["off"]
    lost = taken = 0
    for k in range(Cs.STREET_FRAMES):
        th, _ = st.read_votes(k)
        dyn = th >= 2
        lost += int((dyn & ~labels[k]).sum())
        if off[k + 1] - off[k] >= 4:
            taken += 1
            assert (dyn & labels[k]).sum() >= 0.5 * labels[k].sum(), k
    assert taken >= 4 and lost <= 0.001 * sum(int((~l).sum()) for l in labels)


def car_path_voxels(vox):
    """voxels of a map inside the corridor the box sweeps (18 m down the road, above the ground)"""
    return int(((np.abs(vox[:, 0] - 18.0) <= 1.0) & (vox[:, 2] > 0.15) & (np.abs(vox[:, 1]) < 9.5)).sum())


def test_the_map_over_the_static_store(world):
    from glio_amd import mapping
    st, dense, poses = world["st"], world["dense"], world["poses"]
    frames = list(range(Cs.STREET_FRAMES))
    opts = mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 16)
    gm = mapping.GlobalMap(st, opts)
    gi = gm.add(frames, poses)
    vox = gm.read()
    moved = np.vstack([move(world["want"][k]["kept"], poses[k]) for k in frames])
    want_vox, _ = restated_voxel_grid(moved, 0.2)
    assert gi.n_points_total == len(moved) and gi.n_voxels == len(want_vox)
    assert np.array_equal(vox.view(np.uint32), want_vox.view(np.uint32))
    full = mapping.GlobalMap(dense, opts)
    full.add(frames, poses)
    vox_full = full.read()
    n_clean, n_full = car_path_voxels(vox), car_path_voxels(vox_full)
    print("voxels along the car's path: %d uncleaned, %d cleaned; map %d -> %d voxels" % (n_full, n_clean, len(vox_full), len(vox)))
    assert n_full >= 100 and n_clean <= 0.5 * n_full and len(vox) > 0.9 * len(vox_full)
    # the next classification comes behind the map's read; a frame never classified reads as never set
    st.classify(frames, poses, world["off"], Cs.street_call(poses)[1])
    gm.clear()
    assert gm.add(frames, poses).n_voxels == len(want_vox)
    gm.close(); full.close()


def test_a_frame_never_classified_reads_as_never_set(world):
    from glio_amd import capi, mapping, static_map
    st2 = static_map.StaticClouds(world["dense"])
    gm = mapping.GlobalMap(st2, mapping.default_opts(max_voxels=1 << 12, max_points_per_add=1 << 12))
    with pytest.raises(capi.GlioError, match="never set"):
        gm.add([0], world["poses"][:1])
    gm.close(); st2.close()

"""GPU: glio_localmap_rebuild_from_frames -- the ring of the device-resident local map rebuilt from the keyframe clouds a batch association holds, at
caller-supplied (corrected) poses: buildLocalMapWithLandMark's rebuild branch (reference GLIO/src/Estimator.cpp:3545-3579) + downSampleCloud.  The call must
equal, bit for bit, a fresh ring that got the same clouds pushed at the same poses and was then built -- the map, the ring state later pushes see, both
accumulation modes -- and, in float mode, the oracle's restatement (transform_cloud + voxel_grid).  Every comparison of device output is exact equality."""
import numpy as np
import pytest

from glio_amd import synth

pytestmark = pytest.mark.gpu

WIDTH, LEAF, CAP, K = 4, 0.4, 8192, 8
CUT = {3: 1, 4: 1023, 5: 4097}            # ragged frames: off the 256- and 1024-point tile edges of the rebuild kernel


@pytest.fixture(scope="module")
def rig():
    """8 keyframes of 5000 points (the fixture of test_hip_localmap.py, one keyframe longer), some cut short; body clouds = scan - t_lb; the poses the clouds
    arrived with (ground truth) and the corrected ones (moved by ~0.3 m / 2 degrees); a batch association holding the clouds"""
    from glio_amd import batch
    win = synth.make_window(W=K, pts_per_scan=5000, seed=synth.SEED_BASE + 81, scan_radius=25.0)
    tlb = np.array(win.opts.t_lb, np.float32)
    clouds, scans = [], []
    for s in range(K):
        sc = np.ascontiguousarray(win.scans[s][:CUT.get(s, len(win.scans[s]))])
        c = sc.copy(); c[:, :3] -= tlb
        scans.append(sc); clouds.append(np.ascontiguousarray(c))
    rng = np.random.default_rng(11)
    old = np.zeros((K, 7)); new = np.zeros((K, 7))
    for s in range(K):
        old[s, :3], old[s, 3:] = win.gt.trans[s], win.gt.quat[s]
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        half = np.deg2rad(2.0) / 2
        q = synth.qmul(np.array([np.cos(half), *(np.sin(half) * ax)]), win.gt.quat[s])
        d = rng.normal(size=3); d *= 0.3 / np.linalg.norm(d)
        new[s, :3], new[s, 3:] = win.gt.trans[s] + d, q / np.linalg.norm(q)
    ba = batch.BatchAssociation(K, CAP, 16)
    for s in range(K):
        ba.set_frame(s, clouds[s])
    yield dict(win=win, tlb=tlb, clouds=clouds, scans=scans, old=old, new=new, ba=ba)
    ba.close()


def _opts(W=1):
    return synth.default_opts(W, pts=CAP, map_pts=1 << 17)


def _ctx(mode, W=1, opts=None):
    from glio_amd import capi
    ctx = capi.Context(opts if opts is not None else _opts(W))
    ctx.localmap_config(WIDTH, LEAF, CAP)
    if mode:
        ctx.localmap_set_accumulation(mode)
    return ctx


def _pushed(rig, frames, poses, mode):
    """the route the call replaces: a fresh ring, one push per frame, one build"""
    ctx = _ctx(mode)
    for f, p in zip(frames, poses):
        ctx.localmap_push(rig["clouds"][f], p[3:], p[:3])
    ctx.localmap_build()
    return ctx


def _oracle(rig, frames, poses):
    from oracle import pyoracle as po
    return po.voxel_grid(np.vstack([po.transform_cloud(rig["clouds"][f], p[3:], p[:3]) for f, p in zip(frames, poses)]), LEAF)[0]


def test_rebuild_equals_the_oracle_bit_for_bit_in_float_mode(rig):
    ctx = _ctx(1)
    for frames in ([2, 3, 4, 5], [5, 2, 4, 3]):                   # (concatenation order matters to the float sums)
        n = ctx.localmap_rebuild_from_frames(rig["ba"], frames, rig["new"][frames])
        ref = _oracle(rig, frames, rig["new"][frames])
        got = ctx.localmap_read()
        assert n == len(ref) == len(got) and np.array_equal(got, ref), frames
    # the corrected poses move voxels: a call that left the map as pushed at the old poses would not pass
    stale = _oracle(rig, [2, 3, 4, 5], rig["old"][[2, 3, 4, 5]])
    ctx.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4, 5], rig["new"][[2, 3, 4, 5]])
    got = ctx.localmap_read()
    assert len(got) != len(stale) or not np.array_equal(got, stale)
    ctx.close()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("frames", [[2], [2, 3, 4], [2, 3, 4, 5]], ids=["n1", "n3", "n4"])
def test_rebuild_equals_the_push_route(rig, mode, frames):
    ctx = _ctx(mode)
    # (something else in the ring first: the rebuild must leave nothing of it)
    ctx.localmap_push(rig["clouds"][0], rig["old"][0, 3:], rig["old"][0, :3]); ctx.localmap_build()
    n = ctx.localmap_rebuild_from_frames(rig["ba"], frames, rig["new"][frames])
    want = _pushed(rig, frames, rig["new"][frames], mode)
    a, b = ctx.localmap_read(), want.localmap_read()
    assert n == len(b) > 0 and np.array_equal(a, b)
    if len(frames) == WIDTH:
        old = _pushed(rig, frames, rig["old"][frames], mode)
        o = old.localmap_read()
        assert len(o) != len(a) or not np.array_equal(o, a)       # the rebuild moved voxels
        old.close()
    ctx.close(); want.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_the_ring_goes_on_after_a_rebuild(rig, mode):
    tlb, new = rig["tlb"], rig["new"]
    # four frames, then the resident scan of keyframe 6 is pushed: the oldest (2) is evicted -- the table must hold exactly what the rebuild added
    ctx = _ctx(mode)
    ctx.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4, 5], new[[2, 3, 4, 5]])
    ctx.set_scan(0, rig["scans"][6])
    ctx.localmap_push_scan(0, tlb, new[6, 3:], new[6, :3])
    n = ctx.localmap_build()
    want = _pushed(rig, [3, 4, 5, 6], new[[3, 4, 5, 6]], mode)
    assert n == len(want.localmap_read()) and np.array_equal(ctx.localmap_read(), want.localmap_read())
    # ... and once more (head has moved: the next eviction takes frame 3's points)
    ctx.localmap_push(rig["clouds"][7], new[7, 3:], new[7, :3]); ctx.localmap_build()
    want.localmap_push(rig["clouds"][7], new[7, 3:], new[7, :3]); want.localmap_build()
    assert np.array_equal(ctx.localmap_read(), want.localmap_read())
    want.close()
    # three frames, then a push: four, nothing evicted
    ctx.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4], new[[2, 3, 4]])
    ctx.localmap_push(rig["clouds"][5], new[5, 3:], new[5, :3]); ctx.localmap_build()
    want = _pushed(rig, [2, 3, 4, 5], new[[2, 3, 4, 5]], mode)
    assert np.array_equal(ctx.localmap_read(), want.localmap_read())
    want.close()
    # twice in a row at different poses = once, in a fresh context (no tombstones, no stale bits of the first)
    ctx.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4, 5], rig["old"][[2, 3, 4, 5]])
    ctx.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4, 5], new[[2, 3, 4, 5]])
    fresh = _ctx(mode)
    fresh.localmap_rebuild_from_frames(rig["ba"], [2, 3, 4, 5], new[[2, 3, 4, 5]])
    assert np.array_equal(ctx.localmap_read(), fresh.localmap_read())
    # a plain build afterwards reproduces it
    a = ctx.localmap_read().copy()
    ctx.localmap_build()
    assert np.array_equal(a, ctx.localmap_read())
    ctx.close(); fresh.close()


def test_association_on_the_rebuilt_map(rig):
    from glio_amd import capi
    o = _opts()
    o.t_lb[:] = [0, 0, 0]
    ctx = _ctx(0, opts=o)
    ctx.localmap_rebuild_from_frames(rig["ba"], [3, 4, 5, 6], rig["new"][[3, 4, 5, 6]])
    dev_map = ctx.localmap_read().copy()
    q, t = rig["win"].init.quat[7], rig["win"].init.trans[7]
    n_dev = ctx.associate(0, rig["clouds"][7], q, t)
    ctx2 = capi.Context(o)
    ctx2.set_map(dev_map)
    assert ctx2.associate(0, rig["clouds"][7], q, t) == n_dev > 1000
    assert all(np.array_equal(a, b) for a, b in zip(ctx.get_correspondences(0), ctx2.get_correspondences(0)))
    ctx.close(); ctx2.close()


@pytest.mark.parametrize("slide_first", [True, False], ids=["slide_then_rebuild", "rebuild_then_slide"])
def test_rebuild_supersedes_a_map_sent_ahead(rig, slide_first):
    from glio_amd import capi
    W, tlb, old, new = 3, rig["tlb"], rig["old"], rig["new"]
    frames = [2, 3, 4, 5]
    ctx = _ctx(0, W)
    ctx.set_scan(W - 1, rig["scans"][6])
    ctx.localmap_push_scan(W - 1, tlb, old[6, 3:], old[6, :3]); ctx.localmap_build()
    ctx.set_scan_ahead(rig["scans"][7])
    ctx.localmap_push_scan_ahead_and_build(tlb, old[7, 3:], old[7, :3])
    if slide_first:
        ctx.slide_window()
    n = ctx.localmap_rebuild_from_frames(rig["ba"], frames, new[frames])
    if not slide_first:
        ctx.slide_window()
    want = _pushed(rig, frames, new[frames], 0)
    the_map = want.localmap_read().copy()
    assert n == len(the_map) and np.array_equal(ctx.localmap_read(), the_map)
    # slot W - 1 holds the scan that was sent ahead: the same records as a context that was handed that scan and that map
    pose = capi.lidar_pose(rig["win"].opts, new[7, 3:], new[7, :3])
    other = capi.Context(_opts(W))
    other.set_map(the_map); other.set_scan(W - 1, rig["scans"][7])
    ca, cb = ctx.associate_resident(W - 1, *pose), other.associate_resident(W - 1, *pose)
    assert ca == cb > 100
    assert all(np.array_equal(x, y) for x, y in zip(ctx.get_correspondences(W - 1), other.get_correspondences(W - 1)))
    ctx.close(); want.close(); other.close()


def test_refusals_leave_the_map_as_it_was(rig):
    from glio_amd import batch, capi
    ba, new = rig["ba"], rig["new"]
    bare = capi.Context(_opts())
    with pytest.raises(capi.GlioError, match="error -3"):                     # GLIO_E_STATE: no glio_localmap_config
        bare.localmap_rebuild_from_frames(ba, [2], new[[2]])
    bare.close()
    ctx = _ctx(0)
    ctx.localmap_rebuild_from_frames(ba, [2, 3, 4], new[[2, 3, 4]])
    before = ctx.localmap_read().copy()
    small = batch.BatchAssociation(3, 2 * CAP, 16)                            # frame 0: more points than the ring takes; frame 2: never set
    big = np.tile(rig["clouds"][0], (2, 1))[:CAP + 1]
    small.set_frame(0, big); small.set_frame(1, rig["clouds"][1])
    bad_pose = new[[2]].copy(); bad_pose[0, 4] = np.nan
    inf_pose = new[[2]].copy(); inf_pose[0, 1] = np.inf
    cases = [
        ("no frames", ba, [], new[[]]),
        ("more frames than the ring is wide", ba, [1, 2, 3, 4, 5], new[[1, 2, 3, 4, 5]]),
        ("frame index below 0", ba, [2, -1], new[[2, 3]]),
        ("frame index K", ba, [K], new[[2]]),
        ("frame never set", small, [1, 2], new[[2, 3]]),
        ("frame larger than the ring's rows", small, [0], new[[2]]),
        ("NaN in a pose", ba, [2], bad_pose),
        ("infinity in a pose", ba, [2], inf_pose),
    ]
    other = None
    if capi.device_count() >= 2:                                              # (needs a second device to exist)
        other = batch.BatchAssociation(2, CAP, 16, device=1)
        other.set_frame(0, rig["clouds"][1])
        cases.append(("association on another device", other, [0], new[[2]]))
    for name, assoc, frames, poses in cases:
        with pytest.raises(capi.GlioError, match="error -1: .*glio_localmap_rebuild_from_frames"):      # GLIO_E_ARG with a message
            ctx.localmap_rebuild_from_frames(assoc, frames, poses)
        assert np.array_equal(ctx.localmap_read(), before), name
        ctx.localmap_build()                                                  # (the ring and the table too: a build gives the same map)
        assert np.array_equal(ctx.localmap_read(), before), name
    # and the context still works
    ctx.localmap_rebuild_from_frames(ba, [2, 3, 4, 5], new[[2, 3, 4, 5]])
    want = _pushed(rig, [2, 3, 4, 5], new[[2, 3, 4, 5]], 0)
    assert np.array_equal(ctx.localmap_read(), want.localmap_read())
    ctx.close(); want.close(); small.close()
    if other is not None:
        other.close()


def test_reference_map_schedule_in_both_hosts_equals_the_oracle(tmp_path):
    """A short stream (W = 3, local_map_width 4, 7 keyframes of 3000 points) with the reference's map schedule on and one loop closure after the fifth keyframe:
    sliding.ReferenceMapSchedule (Python) and glio::SlidingWindowBackend's schedule (C++, host_demo_map_schedule) must give equal maps at every keyframe call, and
    both the map of buildLocalMapWithLandMark (Estimator.cpp:3545-3616) + downSampleCloud restated here from the oracle's transform_cloud + voxel_grid -- the
    whole-map rebuilds of the warm-up, the pushes, and the 3-frame (= width - 1) rebuilds that follow the loop closure on every later call."""
    from collections import deque
    from glio_amd import batch, capi, loop, sliding
    from glio_amd.host import window_io
    from oracle import pyoracle as po
    W, width, NK, pts, cap, loop_after = 3, 4, 7, 3000, 4096, 4
    win = synth.make_window(W=NK, pts_per_scan=pts, seed=synth.SEED_BASE + 83, scan_radius=25.0)
    opts = synth.default_opts(W, pts=cap, map_pts=1 << 17)
    tlb = np.array(opts.t_lb, np.float32)
    scans = [np.ascontiguousarray(win.scans[j][:2500 if j == 2 else pts]) for j in range(NK)]
    q_bl, t_bl = synth.rotvec_q(np.array([0.02, -0.01, 0.03])), np.array([0.05, -0.1, 0.2])
    # pose_info_keyframe as every call finds it: the window's keyframes move with each solve (updatePose), everything moves with the loop closure
    rng = np.random.default_rng(83)
    pose_info = np.zeros((NK, NK, 7))
    cur = np.c_[win.gt.trans[:NK], win.gt.quat[:NK]].copy()
    for j in range(NK):
        for k in range(max(0, j - W + 1), j + 1):
            cur[k, :3] = win.gt.trans[k] + rng.normal(0, 0.05, 3)
            q = synth.qmul(synth.rotvec_q(rng.normal(0, 0.01, 3)), win.gt.quat[k]); cur[k, 3:] = q / np.linalg.norm(q)
        if j == loop_after + 1:                                                       # correctPoses ran between the calls
            cur[:j + 1, :3] += np.array([0.4, -0.3, 0.1])
        pose_info[j] = cur
    # C++
    path, out_path = str(tmp_path / "schedule.bin"), str(tmp_path / "maps.bin")
    window_io.write_map_schedule(path, opts, cap, width, LEAF, scans, pose_info, loop_after=loop_after, accumulation=1, q_bl=q_bl, t_bl=t_bl)
    cpp = window_io.run_demo_map_schedule(path, out_path)
    # Python
    ctx = capi.Context(opts)
    ctx.localmap_config(width, LEAF, cap); ctx.localmap_set_accumulation(1)
    ba = batch.BatchAssociation(NK, cap, 16)
    sched = sliding.ReferenceMapSchedule(ctx, ba, width, q_bl, t_bl)
    py = []
    for j in range(NK):
        if j > 0:
            ctx.slide_window()
        ctx.set_scan(W - 1, scans[j]); ba.set_frame_from_scan(j, ctx, W - 1, tlb)
        will = sched.will_rebuild(j + 1)
        n = sched.update(j + 1, pose_info[j], W - 1, tlb)
        assert will == (sched.last_action == sliding.MAP_REBUILD)
        py.append((sched.last_action, n, ctx.localmap_read().copy()))
        if j == loop_after:
            sched.loop_closed()
    ctx.close(); ba.close()
    # the reference, restated: surf_frames[k] = scan - t_lb (float), recent_surf_keyframes a deque of transformed clouds
    surf_frames = []
    for sc in scans:
        c = sc.copy(); c[:, :3] -= tlb
        surf_frames.append(c)

    def transformed(idx, info):
        p = loop.frame_poses(info[idx:idx + 1], q_bl, t_bl)[0]                        # q_po * q_bl, q_po * t_bl + t_po (:3562-3563)
        return po.transform_cloud(surf_frames[idx], p[3:], p[:3])
    recent, latest_frame_idx, want_actions = deque(), -1, []
    for j in range(NK):
        size, info = j + 1, pose_info[j]
        if len(recent) < width:                                                       # :3545
            recent.clear()
            for i in range(size - 1, -1, -1):
                if size > width and i <= size - width:                                # :3550
                    break
                recent.appendleft(transformed(i, info))
                if len(recent) >= width:
                    break
            want_actions.append(sliding.MAP_REBUILD)
        elif latest_frame_idx != size - 1:                                            # :3582
            recent.popleft(); latest_frame_idx = size - 1
            recent.append(transformed(latest_frame_idx, info))
            want_actions.append(sliding.MAP_PUSH)
        ref = po.voxel_grid(np.vstack(list(recent)), LEAF)[0]                         # :3612-3631
        assert py[j][0] == cpp[j][0] == want_actions[j], j
        assert py[j][1] == cpp[j][1] == len(ref) == len(py[j][2]) == len(cpp[j][2]), j
        assert np.array_equal(py[j][2], cpp[j][2]), f"keyframe {j}: the two hosts"
        assert np.array_equal(py[j][2], ref), f"keyframe {j}: the oracle"
        if j == loop_after:
            recent.clear()                                                            # correctPoses, :4660
    R, P = sliding.MAP_REBUILD, sliding.MAP_PUSH
    assert want_actions == [R, R, R, R, P, R, R]

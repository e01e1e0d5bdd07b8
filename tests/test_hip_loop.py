"""GPU tests of the loop closure (glio_loop_*, csrc/loop_kernels.hip): the submaps against the oracle's transformCloud + VoxelGrid bit for bit, the
1-NN search against brute force exactly, one round and the whole alignment against the numpy restatement (tests/loop_restated.py), the ends
that must not fault, repeatability, independence from a batch association in flight, and the C++ twin."""
import os
import re
import sys

import numpy as np
import pytest

from glio_amd import batch, capi, loop, synth, synth_lidar
from glio_amd import ctypes_types as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_restated as lr  # noqa: E402

pytestmark = pytest.mark.gpu

Q_BL = synth.rotvec_q(np.array([0.01, -0.02, 0.015]))
T_BL = np.array([0.05, -0.02, 0.1])
N_FRAMES = 57


@pytest.fixture(scope="module")
def drive():
    """57 keyframe clouds of a drive down the corridor (finite points, every third: ~4 k per frame as the released surf clouds) and their pose_info"""
    scans = synth_lidar.drive(n_frames=N_FRAMES, n_scans=16, n_az=900, step=(0.5, 0.02, 0.0), yaw_step=0.004)
    clouds, info = [], []
    for k, sc in enumerate(scans):
        sc = sc[np.isfinite(sc[:, :3]).all(axis=1)][::3]
        clouds.append(np.ascontiguousarray(sc, np.float32))
        yaw = 0.004 * k
        info.append(np.r_[np.array([40.0, 0.5, 1.8]) + k * np.array([0.5, 0.02, 0.0]), synth.rotvec_q(np.array([0.0, 0.0, yaw]))])
    return clouds, np.array(info)


@pytest.fixture(scope="module")
def assoc(drive):
    clouds, _ = drive
    ba = batch.BatchAssociation(N_FRAMES + 1, 8192, 200000)          # (frame N_FRAMES is never set)
    for k, c in enumerate(clouds):
        ba.set_frame(k, c)
    yield ba
    ba.close()


def _oracle_submap(clouds, poses, frames, leaf=0.4):
    from oracle import pyoracle as po
    cat = np.concatenate([po.transform_cloud(clouds[k], poses[f, 3:], poses[f, :3]) for f, k in enumerate(frames)])
    return po.voxel_grid(cat, leaf)[0]


def _rc(exc):
    return int(re.search(r"error (-?\d+)", str(exc.value)).group(1))


def _result_bytes(r):
    return (r.transform.tobytes(), np.float64(r.fitness).tobytes(), np.float64(r.last_mse).tobytes(), r.iterations, r.state, r.converged, r.last_n_corr, r.rank_deficient)


@pytest.mark.parametrize("frames", [list(range(56, 50, -1)), list(range(0, 51)), [3, 9, 10, 40], [7]], ids=["latest6", "history51", "gaps", "single"])
def test_submaps_equal_the_oracle_bit_for_bit(drive, assoc, frames):
    clouds, info = drive
    poses = loop.frame_poses(info[frames], Q_BL, T_BL)
    lp = loop.LoopClosure(assoc)
    for which in (loop.SOURCE, loop.TARGET):
        n = lp.build_submap(which, frames, poses)
        got = lp.read_submap(which)
        want = _oracle_submap(clouds, poses, frames)
        assert n == len(got) == len(want), (n, len(want))
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    lp.close()


@pytest.fixture(scope="module")
def known():
    return lr.known_answer_case()


@pytest.fixture(scope="module")
def small_assoc():
    ba = batch.BatchAssociation(2, 64, 16)
    yield ba
    ba.close()


def _check_search(lp, src, tgt, max_corr=30.0):
    idx, d2 = lp.read_correspondences(len(src))
    bi, bd = lr.nn_brute(src, tgt)
    want = np.where(bd.astype(np.float64) <= max_corr * max_corr, bi, -1)
    assert np.array_equal(idx, want)
    assert np.array_equal(d2.view(np.uint32), bd.view(np.uint32))
    return idx


def test_search_equals_brute_force_exactly(known, small_assoc):
    src, tgt, _ = known
    lp = loop.LoopClosure(small_assoc)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    st = lp.step()
    idx = _check_search(lp, src, tgt)
    assert st.n_corr == int((idx >= 0).sum()) == len(src)
    # the gate: an isolated target point, source points 29.9 and 30.1 m from it (and further from everything else)
    iso = np.array([[80.0, 0.0, 300.0, 1.0]], np.float32)
    tgt2 = np.ascontiguousarray(np.r_[tgt, iso], np.float32)
    far = np.array([[80.0, 0.0, 329.9, 0.0], [80.0, 0.0, 330.1, 0.0], [80.0, 0.0, 269.9, 0.0], [80.0, 29.9, 300.0, 0.0], [109.95, 0.0, 300.0, 0.0]], np.float32)
    src2 = np.ascontiguousarray(np.r_[src[:500], far], np.float32)
    lp.set_submap(loop.TARGET, tgt2); lp.set_submap(loop.SOURCE, src2)
    lp.reset_current()
    st = lp.step()
    idx = _check_search(lp, src2, tgt2)
    assert list(idx[500:]) == [len(tgt), -1, -1, len(tgt), len(tgt)]
    assert st.n_fallback >= 5                     # (far from every occupied cell: the brute-force scan answered them)
    lp.close()


def test_search_ties_and_duplicates(small_assoc):
    """duplicate target points, a source point equidistant to several targets (the lowest index wins), and lattice clouds full of exact ties"""
    lp = loop.LoopClosure(small_assoc)
    tgt = np.array([[2, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [1, 5, 0, 3], [1, 5, 0, 4], [1, -1, 0, 5], [1, 1, 0, 6], [1, 0, 1, 7]], np.float32)
    src = np.array([[1, 0, 0, 0], [1, 5, 0, 0], [0, 0, 0, 0], [1, 0, 0.5, 0], [50, 50, 50, 0]], np.float32)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    lp.step()
    idx = _check_search(lp, src, tgt)
    assert list(idx[:3]) == [0, 3, 1]
    rng = np.random.default_rng(5)
    tgt = np.c_[rng.integers(-12, 13, (6000, 3)), np.zeros(6000)].astype(np.float32)            # a lattice with many duplicates
    src = (np.c_[rng.integers(-14, 15, (3000, 3)), np.zeros(3000)] + np.array([0.5, 0.5, 0.5, 0.0])).astype(np.float32)      # cell centres: 8 equidistant corners
    src[::7, :3] *= 3.0                                                                          # and some far outside the target's box
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    lp.step()
    _check_search(lp, src, tgt)
    lp.close()


def _ulp_ok(got, want, n=2):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    tol = n * np.spacing(np.maximum(np.abs(want), np.float32(1.0)).astype(np.float32))
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol.astype(np.float64))


def test_step_equals_the_restated_round(known, small_assoc):
    src, tgt, _ = known
    lp = loop.LoopClosure(small_assoc)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    lp.reset_current()
    cur = lp.read_current()
    assert np.array_equal(cur.view(np.uint8), src.view(np.uint8))
    for rnd in range(4):
        st = lp.step()
        want = lr.round_of(cur, tgt, lr.DEFAULTS)
        print(f"round {rnd}: n_corr {st.n_corr} / {want['n_corr']}, mse {st.mse!r} / {want['mse']!r}, max |dT| {np.abs(st.transform - want['T']).max():.3e}, fallback {st.n_fallback}")
        assert st.n_corr == want["n_corr"]
        assert abs(st.mse - want["mse"]) <= 1e-12 * abs(want["mse"])
        assert _ulp_ok(st.transform, want["T"], 2), (st.transform, want["T"])
        nxt = lp.read_current()
        assert np.array_equal(nxt.view(np.uint8), lr.apply_T(st.transform, cur).view(np.uint8))      # rule 4, with the device's own transform
        cur = nxt
    lp.close()


def _check_align(lp, src, tgt, known_T=None):
    r = lp.align()
    want = lr.icp(src, tgt)
    dt, dr = lr.pose_error(r.transform, want["transform"])
    fit = lr.fitness(lp.read_current(), tgt, lr.make_tree(tgt))
    print(f"align: iterations {r.iterations} / {want['iterations']}, state {r.state_name}, |dt| {dt:.3e} m, |dR| {dr:.3e} rad vs the restatement, "
          f"fitness {r.fitness!r} (restated on the device's final cloud {fit!r}, the restatement's own {want['fitness']!r})")
    assert (r.iterations, r.state, r.converged) == (want["iterations"], want["state"], want["converged"])
    assert dt < 1e-4 and dr < 1e-5
    assert abs(r.fitness - fit) <= 1e-9 * fit
    assert r.last_n_corr == want["last_n_corr"]
    if known_T is not None:
        kt, kr = lr.pose_error(r.transform, known_T)
        print(f"       vs the known motion |dt| {kt:.3e} m, |dR| {kr:.3e} rad")
        assert kt < 1e-4 and kr < 1e-5
    return r, (dt, dr)


@pytest.mark.parametrize("seed", [20261017, 20261019, 20261020])
def test_align_known_answer(small_assoc, seed):
    """iterations / state / converged equal the restatement's; the transform within the project's pose gates (1e-4 m, 1e-5 rad) of the restatement's and
    of the known motion.  The fitness is the restatement's evaluated on the DEVICE's final cloud (the source moved by the device's own per-round
    transforms, rule 4: what getFitnessScore sees), to rel 1e-9: on this case the whole fitness (~1.7e-10 m^2) is float rounding of that cloud, so no
    other evaluation point -- the accumulated 4x4 applied to the source included -- can agree to that level."""
    src, tgt, known_T = lr.known_answer_case(seed)
    lp = loop.LoopClosure(small_assoc)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    r, _ = _check_align(lp, src, tgt, known_T)
    assert r.state == T.LOOP_TRANSFORM and r.converged
    lp.close()


def test_align_independently_sampled_pair(small_assoc):
    """~9 k source / ~33 k target points sampled independently from the same place (no known answer: point-to-point ICP slides along the corridor on such
    a pair); the reordering check of tests/test_loop_restated.py holds on it (the restatement: 18 rounds, TRANSFORM, fitness 0.025).  The differences
    between device and restatement are printed here and recorded by scripts/loop_timing.py ("align_independent_pair" / "vs_restatement"); NO figure from
    an MI355X is recorded yet -- the gates above are the project's pose gates and the issue's rel 1e-9, not figures seen."""
    src, tgt = lr.independent_pair()
    lp = loop.LoopClosure(small_assoc)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    _check_align(lp, src, tgt)
    fb = lp.fallbacks()
    assert len(fb) == lp.align().iterations + 1 and fb.min() >= 0
    lp.close()


def test_ends_without_fault(known, small_assoc):
    src, tgt, _ = known
    lp = loop.LoopClosure(small_assoc)
    # clouds 100 m apart: no pair inside 30 m
    lp.set_submap(loop.TARGET, tgt)
    away = src.copy(); away[:, 2] += 100.0
    lp.set_submap(loop.SOURCE, away)
    r, w = lp.align(), lr.icp(away, tgt)
    assert (r.converged, r.state, r.iterations) == (False, T.LOOP_NO_CORRESPONDENCES, 0) == (w["converged"], w["state"], w["iterations"])
    assert np.array_equal(r.transform, np.eye(4, dtype=np.float32)) and abs(r.fitness - w["fitness"]) <= 1e-9 * w["fitness"]
    # a 3-point source
    lp.set_submap(loop.SOURCE, src[[10, 700, 2500]])
    r, w = lp.align(), lr.icp(src[[10, 700, 2500]], tgt)
    assert np.isfinite(r.transform).all() and np.isfinite(r.fitness) and (r.iterations, r.state) == (w["iterations"], w["state"])
    # a coplanar source (rank 2: Umeyama still determines the rotation)
    flat = src[np.abs(src[:, 2] - np.median(src[:, 2])) < 0.5][:800].copy()
    flat[:, 2] = 0.25
    lp.set_submap(loop.SOURCE, flat)
    r, w = lp.align(), lr.icp(flat, tgt)
    assert np.isfinite(r.transform).all() and not r.rank_deficient and (r.iterations, r.state, r.converged) == (w["iterations"], w["state"], w["converged"])
    # a collinear source and a collinear target: no rotation is determined -- reported, nothing moves, no NaN
    line = np.zeros((50, 4), np.float32); line[:, 0] = np.arange(50)
    lp.set_submap(loop.SOURCE, line + np.array([0.25, 0, 0, 0], np.float32)); lp.set_submap(loop.TARGET, line)
    r = lp.align()
    assert r.rank_deficient and not r.converged and r.state == T.LOOP_NOT_CONVERGED and r.iterations == 0 and np.array_equal(r.transform, np.eye(4, dtype=np.float32))
    assert lr.icp(line + np.array([0.25, 0, 0, 0], np.float32), line)["rank_deficient"]
    lp.close()
    # max_iterations = 1 and 2
    for it in (1, 2):
        lp = loop.LoopClosure(small_assoc, loop.default_opts(max_iterations=it))
        lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
        r, w = lp.align(), lr.icp(src, tgt, max_iterations=it)
        assert (r.converged, r.state, r.iterations) == (True, T.LOOP_ITERATIONS, it) == (w["converged"], w["state"], w["iterations"])
        assert lr.pose_error(r.transform, w["transform"])[0] < 1e-4
        lp.close()


def test_error_returns(drive, assoc):
    clouds, info = drive
    lp = loop.LoopClosure(assoc, loop.default_opts(max_source_points=2000, max_frames_per_submap=8))
    poses = loop.frame_poses(info[:4], Q_BL, T_BL)
    with pytest.raises(capi.GlioError) as e:              # align before both submaps exist
        lp.align()
    assert _rc(e) == -3
    with pytest.raises(capi.GlioError) as e:
        lp.step()
    assert _rc(e) == -3
    for frames, what in (([0, 1, N_FRAMES + 1, 2], "outside"), ([0, -1, 1, 2], "outside"), ([0, 1, N_FRAMES, 2], "never set")):
        with pytest.raises(capi.GlioError) as e:
            lp.build_submap(loop.TARGET, frames, poses)
        assert _rc(e) == -1 and what in str(e.value)
    with pytest.raises(capi.GlioError) as e:              # more voxels than the source submap takes
        lp.build_submap(loop.SOURCE, [0, 1, 2, 3], poses)
    assert _rc(e) == -1 and "takes 2000" in str(e.value)
    with pytest.raises(capi.GlioError) as e:              # more frames than max_frames_per_submap
        lp.build_submap(loop.TARGET, list(range(9)), loop.frame_poses(info[:9], Q_BL, T_BL))
    assert _rc(e) == -1
    with pytest.raises(capi.GlioError) as e:              # an empty submap
        lp.set_submap(loop.SOURCE, np.zeros((0, 4), np.float32))
    assert _rc(e) == -1
    with pytest.raises(capi.GlioError) as e:              # a submap above capacity
        lp.set_submap(loop.SOURCE, np.zeros((2001, 4), np.float32))
    assert _rc(e) == -1
    lp.set_submap(loop.SOURCE, clouds[0][:100])
    with pytest.raises(capi.GlioError) as e:              # the target is still missing
        lp.align()
    assert _rc(e) == -3
    # and the object still works
    assert lp.build_submap(loop.TARGET, [0, 1, 2, 3], poses) > 0
    assert np.isfinite(lp.align().fitness)
    lp.close()
    with pytest.raises(capi.GlioError) as e:
        loop.LoopClosure(assoc, loop.default_opts(max_iterations=0))
    assert _rc(e) == -1


def test_two_aligns_give_identical_bytes(known, small_assoc):
    src, tgt, _ = known
    lp = loop.LoopClosure(small_assoc)
    lp.set_submap(loop.SOURCE, src); lp.set_submap(loop.TARGET, tgt)
    a = lp.align(); ca = lp.read_current()
    b = lp.align(); cb = lp.read_current()
    assert _result_bytes(a) == _result_bytes(b) and np.array_equal(ca.view(np.uint8), cb.view(np.uint8))
    other = loop.LoopClosure(small_assoc)                  # and a fresh object
    other.set_submap(loop.SOURCE, src); other.set_submap(loop.TARGET, tgt)
    assert _result_bytes(other.align()) == _result_bytes(a)
    other.close(); lp.close()


def test_align_beside_an_association_in_flight(drive, assoc):
    """an align issued while a glio_bassoc_run_append_async is on the association's stream: the same result as alone, the association's records unchanged"""
    clouds, info = drive
    poses_all = np.zeros((N_FRAMES + 1, 7)); poses_all[:, 3] = 1.0
    poses_all[:N_FRAMES] = loop.frame_poses(info, Q_BL, T_BL)
    ci, cj = batch.pair_list(12, 2)
    assoc.reset()
    cnt0, tot0 = assoc.run_append(poses_all, ci, cj)
    rec0 = [a.copy() for a in assoc.read()]
    lp = loop.LoopClosure(assoc)
    src_f, tgt_f = list(range(56, 50, -1)), list(range(0, 40))
    lp.build_submap(loop.SOURCE, src_f, loop.frame_poses(info[src_f], Q_BL, T_BL))
    lp.build_submap(loop.TARGET, tgt_f, loop.frame_poses(info[tgt_f], Q_BL, T_BL))
    alone = lp.align()
    assoc.reset()
    assoc.run_append(poses_all, ci, cj, wait=False)
    beside = lp.align()
    cnt1, tot1 = assoc.finish()
    rec1 = assoc.read()
    assert _result_bytes(alone) == _result_bytes(beside)
    assert tot0 == tot1 and tot0 > 0 and np.array_equal(cnt0, cnt1) and all(np.array_equal(a, b) for a, b in zip(rec0, rec1))
    # submaps built while a run is in flight, too
    assoc.reset()
    assoc.run_append(poses_all, ci, cj, wait=False)
    lp.build_submap(loop.SOURCE, src_f, loop.frame_poses(info[src_f], Q_BL, T_BL))
    again = lp.align()
    cnt2, tot2 = assoc.finish()
    assert _result_bytes(again) == _result_bytes(alone) and tot2 == tot0 and np.array_equal(cnt2, cnt0)
    assoc.reset()
    lp.close()


def test_host_demo_loop_equals_the_python_driver(drive, tmp_path):
    from glio_amd.host import window_io
    clouds, info = drive
    K = 30
    opts = loop.default_opts()
    closest = 8
    latest, src_f, tgt_f = loop.submap_frames(K + 4, 5, closest, 6)
    assert latest == K - 1
    path = str(tmp_path / "loop_case.bin")
    window_io.write_loop_case(path, opts, 8192, clouds[:K], src_f, info[src_f], tgt_f, info[tgt_f], Q_BL, T_BL, 0.3)
    got = window_io.run_demo_loop(path)
    ba = batch.BatchAssociation(K, 8192, 1)
    for k in range(K):
        ba.set_frame(k, clouds[k])
    lp = loop.LoopClosure(ba, opts)
    ns = lp.build_submap(loop.SOURCE, src_f, loop.frame_poses(info[src_f], Q_BL, T_BL))
    nt = lp.build_submap(loop.TARGET, tgt_f, loop.frame_poses(info[tgt_f], Q_BL, T_BL))
    assert (got["n_src"], got["n_tgt"]) == (ns, nt)
    assert got["src_sum"] == window_io.loop_checksum(lp.read_submap(loop.SOURCE)) and got["tgt_sum"] == window_io.loop_checksum(lp.read_submap(loop.TARGET))
    r = lp.align()
    assert (got["converged"], got["state"], got["iterations"], got["last_n_corr"], got["rank_deficient"]) == (r.converged, r.state, r.iterations, r.last_n_corr, r.rank_deficient)
    assert got["fitness"] == r.fitness and got["last_mse"] == r.last_mse
    assert np.array_equal(got["transform"].view(np.uint32), r.transform.view(np.uint32))
    con = loop.loop_constraint(r, info[src_f[0]], info[tgt_f[len(tgt_f) // 2]], 0.3)
    if con is None:
        assert got["constraint"] is None
    else:
        assert np.array_equal(got["constraint"][0], con[0]) and got["constraint"][1] == con[1][0]
    lp.close(); ba.close()

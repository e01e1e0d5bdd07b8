"""GPU: glio_batch_covariance (include/glio_batch_cov.h) -- the per-keyframe marginal covariance of the batch stage by selected inversion down the
block cyclic reduction's tree -- on the fixed cases of batch_covariance_restated.cases(), through the assertion the numpy restatement passes on the CPU:
against np.linalg.inv of the oracle's dense H with the anchor's rows and columns deleted.

Figures on the MI355X (scaled error / bound 8 n kappa_s eps): see DESIGN section 9."""
import ctypes as C

import numpy as np
import pytest

import batch_covariance_problems as problems
import batch_covariance_restated as restated
from glio_amd import batch, capi
from glio_amd import ctypes_types as T

pytestmark = pytest.mark.gpu
CASES = restated.cases()
BY_NAME = {c["name"]: c for c in CASES}


def _run(p, cross=True):
    st = problems.stage(p)
    try:
        return st.covariance(p["init"], p["sb0"], anchor=p["anchor"], cross=cross)
    finally:
        st.close()


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] in ("gate", "gate_gnss")], ids=lambda c: c["name"])
def test_blocks_against_the_dense_inverse(case):
    p = problems.build(case)
    st = problems.stage(p)
    diag, nxt, info = st.covariance(p["init"], p["sb0"], anchor=p["anchor"], cross=True)
    K, B, a = p["K"], p["B"], p["anchor"]
    assert (info.n, info.B, info.anchor, info.bad_keyframe) == (K * B, B, a, -1) and info.levels >= 1 and 0 < info.min_pivot <= info.max_pivot <= 1 + 1e-9
    restated.assert_blocks_within_bound(diag, nxt, p["H"], a, case["name"], restated.GUARD_GNSS if case["expect"] == "gate_gnss" else restated.GUARD)
    # the H used is the one linearize_full reports the diagonal of (the call scales by that very buffer): its diagonal against the diagonal of the
    # oracle's H, the matrix the blocks above were just held to the inverse of
    d_dev = st.linearize_full(p["init"], p["sb0"])[0]
    assert np.abs(d_dev - np.diag(p["H"])).max() <= 1e-10 * np.diag(p["H"]).max()
    if a >= 0:          # the anchor's pose rows and columns: exact zeros; its speed / bias block stays free
        assert not diag[a][:6, :].any() and not diag[a][:, :6].any()
        assert (a == 0 or not nxt[a - 1][:, :6].any()) and (a == K - 1 or not nxt[a][:6, :].any())
        if B == 15:
            assert np.all(np.diag(diag[a])[6:] > 0)
    assert all(np.array_equal(d, d.T) for d in diag)                      # symmetric to the bit
    assert all(np.all(np.diag(d)[(0 if k != a else 6):] > 0) for k, d in enumerate(diag))
    diag2, nxt2, _ = st.covariance(p["init"], p["sb0"], anchor=a, cross=True)          # bit-identical from run to run
    assert np.array_equal(diag2, diag) and np.array_equal(nxt2, nxt)
    diag3, _ = st.covariance(p["init"], p["sb0"], anchor=a, cross=False)               # next = NULL leaves diag's bits alone
    assert np.array_equal(diag3, diag)
    assert st.covariance_last_device_ms() > 0 and len(st.covariance_last_device_ms(stages=True)) == 5
    st.close()


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "floor"], ids=lambda c: c["name"])
def test_pose_only_with_gnss_follows_the_restatement(case):
    """kappa_s ~ 6e9: the bound against the inverse (3e-3) would say nothing.  GLIO_OK, symmetry, reproducibility, and agreement with the numpy
    restatement within 100 x the restatement's own scaled error against np.linalg.inv on this case (the floor convention)."""
    p = problems.build(case)
    st = problems.stage(p)
    diag, nxt, info = st.covariance(p["init"], anchor=-1, cross=True)
    assert info.bad_keyframe == -1
    rd, rn = restated.selected_inverse(p["H"], p["K"], p["B"], p["sbk"], -1)
    wd, wn, kappa, n = restated.reference_blocks(p["H"], p["K"], p["B"], -1)
    floor = restated.scaled_error(rd, rn, wd, wn, p["H"])
    agree = restated.scaled_error(diag, nxt, rd, rn, p["H"])
    print(f"{case['name']}: n {n}, kappa_s {kappa:.4e}, device vs restatement {agree:.2e}, restatement vs inverse {floor:.2e} (gate {restated.FLOOR_FACTOR} x), "
          f"device vs inverse {restated.scaled_error(diag, nxt, wd, wn, p['H']):.2e}, 8 n kappa_s eps {8 * n * kappa * restated.EPS:.2e}")
    assert agree <= restated.FLOOR_FACTOR * floor, (agree, floor)
    assert all(np.array_equal(d, d.T) for d in diag)
    diag2, nxt2, _ = st.covariance(p["init"], anchor=-1, cross=True)
    assert np.array_equal(diag2, diag) and np.array_equal(nxt2, nxt)
    st.close()


@pytest.mark.parametrize("case", [c for c in CASES if c["expect"] == "singular"], ids=lambda c: c["name"])
def test_a_free_gauge_ends_in_numeric_not_in_numbers(case):
    """planes (+ delta_q) only, and the same with the IMU chain, no GNSS, no anchor: data the Cholesky rejects"""
    p = problems.build(case)
    st = problems.stage(p)
    with pytest.raises(capi.GlioError) as e:
        st.covariance(p["init"], p["sb0"], anchor=-1, cross=True)
    assert e.value.code == capi.E_NUMERIC and 0 <= e.value.info.bad_keyframe < p["K"]
    assert not e.value.out[0].any() and not e.value.out[1].any()          # untouched
    # the same stage, anchored: the numbers of a fresh stage (a failed call leaves nothing behind)
    diag, info = st.covariance(p["init"], p["sb0"], anchor=0)
    st.close()
    st2 = problems.stage(p)
    want, _ = st2.covariance(p["init"], p["sb0"], anchor=0)
    st2.close()
    assert np.array_equal(diag, want) and info.bad_keyframe == -1


def test_every_refusal_leaves_diag_untouched():
    lib = capi.load()
    p = problems.build(BY_NAME["imu_K13_b6_nognss_a12"])
    K, B = p["K"], p["B"]
    poses = np.ascontiguousarray(p["init"], np.float64); sb = np.ascontiguousarray(p["sb0"], np.float64)
    diag = np.full((K, B, B), 7.0); nxt = np.full((K - 1, B, B), 7.0)
    info = T.GlioBatchCovInfo()
    st = problems.stage(p)
    call = lambda h, po, s, a, d: lib.glio_batch_covariance(h, po, s, a, d, T.dptr(nxt), C.byref(info))
    assert call(st._h, T.dptr(poses), T.dptr(sb), K, T.dptr(diag)) == capi.E_ARG           # anchor outside [-1, K)
    assert call(st._h, T.dptr(poses), T.dptr(sb), -2, T.dptr(diag)) == capi.E_ARG
    assert call(st._h, None, T.dptr(sb), 0, T.dptr(diag)) == capi.E_ARG                    # null poses
    assert call(st._h, T.dptr(poses), T.dptr(sb), 0, None) == capi.E_ARG                   # null diag
    assert call(None, T.dptr(poses), T.dptr(sb), 0, T.dptr(diag)) == capi.E_ARG
    assert call(st._h, T.dptr(poses), None, 0, T.dptr(diag)) == capi.E_ARG                 # the chain is set: speed_bias needed
    ms = C.c_float()
    assert lib.glio_batch_covariance_last_device_ms(st._h, C.byref(ms)) == capi.E_STATE      # nothing ran yet
    st.close()
    # a sharded stage
    from test_hip_batch_tr import _stage
    sh = _stage(K, p["band"], p["con"], p["dq"], p["dd"], p["frame"], imu=p["imu"], rank=0, world=2)
    assert call(sh._h, T.dptr(poses), T.dptr(sb), 0, T.dptr(diag)) == capi.E_STATE
    sh.close()
    # a band the block cyclic reduction does not cover
    wide = batch.BatchStage(30, 13, 16)
    pw = np.ascontiguousarray(batch.make_poses(30, seed=3)[1], np.float64)
    dw = np.full((30, 6, 6), 7.0)
    assert lib.glio_batch_covariance(wide._h, T.dptr(pw), None, 0, T.dptr(dw), None, C.byref(info)) == capi.E_ARG
    wide.close()
    assert np.all(diag == 7.0) and np.all(nxt == 7.0) and np.all(dw == 7.0)


@pytest.mark.parametrize("name", ["pose_K13_b6_nognss_a3", "imu_K13_b6_nognss_a12"])
def test_a_solve_after_the_call_returns_the_bits_it_returns_without_it(name):
    """with the moment records valid (a solve came before) and not (a fresh stage): solve_tr and linearize_full after covariance() == without it"""
    p = problems.build(BY_NAME[name])
    opts = T.batch_tr_opts(max_iterations=6)
    def solve(st):
        r = st.solve_tr(p["init"], opts, speed_bias=p["sb0"]) if p["imu"] is not None else st.solve_tr(p["init"], opts)
        return [np.asarray(x) for x in r[:-1]] + [np.array([r[-1].iterations, r[-1].final_cost])]
    plain = problems.stage(p)
    want1 = solve(plain); want2 = solve(plain); want_lin = plain.linearize_full(p["init"], p["sb0"])
    plain.close()
    st = problems.stage(p)
    st.covariance(p["init"], p["sb0"], anchor=p["anchor"], cross=True)          # records not valid yet
    got1 = solve(st)
    st.covariance(got1[0], got1[1] if p["imu"] is not None else None, anchor=p["anchor"])          # records valid, at another point
    got2 = solve(st)
    st.covariance(p["init"], p["sb0"], anchor=p["anchor"])
    got_lin = st.linearize_full(p["init"], p["sb0"])
    st.close()
    for a, b in zip(want1 + want2, got1 + got2):
        assert np.array_equal(a, b)
    assert np.array_equal(want_lin[0], got_lin[0]) and np.array_equal(want_lin[1], got_lin[1]) and want_lin[2] == got_lin[2]


def test_one_stage_through_two_problems():
    """the same stage handed another constraint set and then the IMU chain (B 6 -> 15: the workspaces are rebuilt) equals fresh stages"""
    pa = problems.build(BY_NAME["pose_K13_b6_nognss_a3"]); pb = problems.build(BY_NAME["imu_K13_b6_nognss_a12"]); pc = problems.build(BY_NAME["pose_K13_b6_gnss_a-1"])
    fresh = [_run(pa), _run(pb), _run(pc), _run(pa)]
    st = problems.stage(pa)
    got = [st.covariance(pa["init"], anchor=pa["anchor"], cross=True)]
    st.set_constraints(*pb["con"]); st.set_small_factors(pb["dq"], pb["dd"], pb["frame"]); st.set_imu(pb["imu"])
    got.append(st.covariance(pb["init"], pb["sb0"], anchor=pb["anchor"], cross=True))
    st.set_imu([]); st.set_constraints(*pc["con"]); st.set_small_factors(pc["dq"], pc["dd"], pc["frame"])
    got.append(st.covariance(pc["init"], anchor=-1, cross=True))
    st.set_constraints(*pa["con"]); st.set_small_factors(pa["dq"], pa["dd"], pa["frame"])
    got.append(st.covariance(pa["init"], anchor=pa["anchor"], cross=True))
    st.close()
    for (d, n, _), (wd, wn, _) in zip(got, fresh):
        assert np.array_equal(d, wd) and np.array_equal(n, wn)

"""IMU pre-integration from raw samples on the device (csrc/imu_kernels.hip, glio_imu_*): the integration against the recorded reference
(tests/golden/preint_cases.npz) and the numpy restatement at the project's pre-integration tolerances (tests/preint_cases.py), the
independence of an edge from the launch it rides in, and everything downstream of the digest -- window, moving window, batch stage --
against the host path fed with the same edges: H, g, cost to 1e-10 relative, poses inside the pose gate (1e-4 m, 1e-5 rad) with equal
iterations and termination, the marginalization's J0^T J0 to 1e-8, the batch solve to 1e-7 (poses) / 1e-6 (speed-bias)."""
import numpy as np
import pytest

import preint_cases
from glio_amd import ctypes_types as T
from glio_amd import synth

pytestmark = pytest.mark.gpu

CASES = preint_cases.load()


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


def rel_err(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def rot_angle(qa, qb):
    d = synth.qmul(synth.qconj(qa), qb)
    return 2 * np.arctan2(np.linalg.norm(d[1:]), abs(d[0]))


def assert_pose_gate(sa, sb):
    dt = np.linalg.norm(sa.trans - sb.trans, axis=1).max()
    dr = max(rot_angle(sa.quat[i], sb.quat[i]) for i in range(sa.W))
    print(f"pose gate: {dt:.3e} m {dr:.3e} rad")
    assert dt <= 1e-4 and dr <= 1e-5, (dt, dr)


def _case_edge(case):
    n = len(case["dt"])
    smp = np.zeros((n, 7))
    smp[:, 0], smp[:, 1:4], smp[:, 4:7] = case["dt"], case["acc"].reshape(-1, 3), case["gyr"].reshape(-1, 3)
    return smp, case["start"]


def test_fixture_cases_on_the_device(hip):
    """every recorded case, one store per noise setting, all its cases in ONE launch; read back with glio_imu_read"""
    from glio_amd import imu
    for noise in sorted({c["noise"] for c in CASES}):
        mine = [c for c in CASES if c["noise"] == noise]
        st = imu.ImuStore(len(mine), 1000, noise=noise)
        st.integrate(0, [_case_edge(c) for c in mine])
        got = st.read_structs(0, len(mine))
        for k, c in enumerate(mine):
            preint_cases.check(got[k], c["want"], c["name"])
            assert list(got[k].linearized_ba) == list(c["start"][6:9]) and list(got[k].linearized_bg) == list(c["start"][9:12])
            if len(c["dt"]) == 0:
                assert bytes(got[k]) == bytes(c["want"])          # the constructor's state, exactly
        assert st.last_device_ms() > 0
        st.close()


def _ragged_edges(n_edges, seed, max_len=400):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n_edges)
    lens[:3] = [0, 1, max_len]
    edges = []
    for n in lens:
        smp = np.zeros((n, 7))
        smp[:, 0] = rng.uniform(0.002, 0.012, n)
        smp[:, 1:4] = np.array([0, 0, 9.8]) + rng.normal(0, 0.5, (n, 3))
        smp[:, 4:7] = rng.normal(0, 0.2, (n, 3))
        start = np.concatenate([np.array([0, 0, 9.8]) + rng.normal(0, 0.5, 3), rng.normal(0, 0.2, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)])
        edges.append((smp, start))
    return edges


def test_an_edge_does_not_depend_on_the_launch_it_rides_in(hip):
    """1999 ragged edges (0 to 400 samples) in one launch: a seeded sample of 200 of them gives the same BYTES when integrated alone, and a
    seeded sample of 50 meets the tolerances against synth.preintegrate"""
    from glio_amd import imu
    N = 1999
    edges = _ragged_edges(N, seed=20261017)
    st = imu.ImuStore(N, 400)
    st.integrate(0, edges)
    got = st.read_structs(0, N)
    print(f"1999 ragged edges: {st.last_device_ms():.3f} ms on the device")
    rng = np.random.default_rng(5)
    alone = imu.ImuStore(1, 400)
    for e in sorted(set(rng.choice(N, 200, replace=False).tolist()) | {0, 1, 2}):
        alone.integrate(0, [edges[e]])
        one = alone.read_structs(0, 1)
        assert bytes(one[0]) == bytes(got[e]), e
    alone.close()
    for e in sorted(set(rng.choice(N, 50, replace=False).tolist()) | {0, 1, 2}):
        smp, start = edges[e]
        want = synth.preintegrate(np.vstack([start[0:3], smp[:, 1:4]]), np.vstack([start[3:6], smp[:, 4:7]]), smp[:, 0], start[6:9], start[9:12])
        preint_cases.check(got[e], want, f"edge {e} ({len(smp)} samples)")
    st.close()


def _window_store(win):
    from glio_amd import imu
    st = imu.ImuStore(len(win.imu_raw), max(len(r[2]) for r in win.imu_raw))
    st.integrate(0, [imu.edge_arrays(a, g, d, np.zeros(3), np.zeros(3)) for a, g, d in win.imu_raw])
    return st


def _associated_context(hip, win):
    ctx = hip.Context(win.opts)
    ctx.set_map(win.map_pts)
    for s in range(win.W):
        q2, t2 = hip.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s])
        assert ctx.associate(s, win.scans[s], q2, t2) > 0
    ctx.set_prior(win.prior)
    ctx.set_gnss(win.frame, win.dd, win.dop)
    return ctx


def _compare_contexts(ca, cb, state, marg=True):
    Ha, ga, costa = ca.linearize(state)
    Hb, gb, costb = cb.linearize(state)
    print(f"linearize: H {rel_err(Hb, Ha):.2e} g {rel_err(gb, ga):.2e} cost {abs(costb - costa) / abs(costa):.2e}")
    assert abs(costb - costa) <= 1e-10 * abs(costa) and rel_err(gb, ga) <= 1e-10 and rel_err(Hb, Ha) <= 1e-10
    sa, ma = ca.solve(state)
    sb, mb = cb.solve(state)
    assert ma.iterations == mb.iterations and ma.termination == mb.termination, (ma.as_dict(), mb.as_dict())
    assert_pose_gate(sb, sa)
    if marg:
        pa, pb = ca.marginalize(sa), cb.marginalize(sa)
        Sa, Sb = pa["lin_jac"].T @ pa["lin_jac"], pb["lin_jac"].T @ pb["lin_jac"]
        rel = np.linalg.norm(Sb - Sa) / np.linalg.norm(Sa)
        print(f"marginalization J0^T J0 rel {rel:.2e}")
        assert rel < 1e-8, rel
    return sa, sb


def test_window_from_store_equals_window_from_host(hip):
    """the same W = 5 window fed once by glio_set_imu with the edges read back from the store, once by glio_set_imu_from_store"""
    win = synth.make_window(W=5, with_gnss=True, with_prior=True)
    st = _window_store(win)
    back = st.read(0, win.W - 1)
    for k in range(win.W - 1):          # and the store's edges are the generator's, at the pre-integration tolerances
        preint_cases.check(back[k], win.preints[k], f"window edge {k}")
    ca, cb = _associated_context(hip, win), _associated_context(hip, win)
    ca.set_imu(back)
    cb.set_imu_from_store(st, np.arange(win.W - 1))
    _compare_contexts(ca, cb, win.init)
    ms, summ = cb.time_solve(win.init, reps=2)          # glio_time_solve runs on the same tables
    sa, ma = ca.solve(win.init)
    assert summ.iterations == ma.iterations and summ.termination == ma.termination
    ca.close(); cb.close(); st.close()


def test_moving_window_from_store_equals_host_path(hip):
    """sliding.py's moving window over 9 keyframes: the store takes one new edge per keyframe (a ring of W slots: the edge-to-slot mapping
    shifts at every slide) against the same stream fed with the host's pre-integrations"""
    from glio_amd import imu, sliding
    W, L = 4, 12
    long = synth.make_window(W=L, pts_per_scan=700, seed=synth.SEED_BASE + 41)
    opts = synth.default_opts(W, pts=1024, map_pts=max(len(long.map_pts), 64))
    first = T.WindowState(W)
    first.trans[:], first.quat[:], first.speed_bias[:] = long.init.trans[:W], long.init.quat[:W], long.init.speed_bias[:W]
    ca, cb = hip.Context(opts), hip.Context(opts)
    da, db = sliding.SlidingWindowDriver(ca, opts), sliding.SlidingWindowDriver(cb, opts)
    ra, rb = hip.Context(opts), hip.Context(opts)
    ea, eb = sliding.ResidentSlidingWindow(ra, opts), sliding.ResidentSlidingWindow(rb, opts)
    for d in (da, db, ea, eb):
        d.start(first)
    ring = W          # store slots: stream edge e lives in slot e % ring
    st = imu.ImuStore(ring, max(len(r[2]) for r in long.imu_raw))
    edge = lambda e: imu.edge_arrays(*long.imu_raw[e], np.zeros(3), np.zeros(3))
    for e in range(W - 2):
        st.integrate(e % ring, [edge(e)])
    for k in range(L - W + 1):
        e_new = k + W - 2          # the edge that entered with this keyframe
        st.integrate(e_new % ring, [edge(e_new)])
        idx = np.array([(k + s) % ring for s in range(W - 1)], np.int32)
        host = [st.read(int(i), 1)[0] for i in idx]
        for s in range(W - 1):
            preint_cases.check(host[s], long.preints[k + s], f"keyframe {k} slot {s}")
        scans = long.scans[k:k + W]
        sa, ma, na = da.step(long.map_pts, scans, host)
        sb, mb, nb = db.step(long.map_pts, scans, (st, idx))
        assert na == nb and ma.iterations == mb.iterations and ma.termination == mb.termination, (k, ma.as_dict(), mb.as_dict())
        assert_pose_gate(sb, sa)
        Sa, Sb = da.prior["lin_jac"].T @ da.prior["lin_jac"], db.prior["lin_jac"].T @ db.prior["lin_jac"]
        assert np.linalg.norm(Sb - Sa) / np.linalg.norm(Sa) < 1e-8, k
        # the same state through glio_linearize on both contexts (their tables still hold this keyframe's factors)
        Ha, ga, costa = ca.linearize(sa)
        Hb, gb, costb = cb.linearize(sa)
        assert abs(costb - costa) <= 1e-10 * abs(costa) and rel_err(gb, ga) <= 1e-10 and rel_err(Hb, Ha) <= 1e-10, k
        ta, xa, _ = ea.step(long.map_pts, scans, host)
        tb, xb, _ = eb.step(long.map_pts, scans, (st, idx))
        assert xa.iterations == xb.iterations and xa.termination == xb.termination, k
        assert_pose_gate(tb, ta)
        if k + W < L:
            for d in (da, db, ea, eb):
                d.slide(long.init.trans[k + W], long.init.quat[k + W], long.init.speed_bias[k + W])
    for c in (ca, cb, ra, rb):
        c.close()
    st.close()


def test_batch_chain_from_store_equals_chain_from_host(hip):
    """smoke()'s K = 24 batch problem: the IMU chain through glio_batch_set_imu_from_store against glio_batch_set_imu"""
    from glio_amd import batch, imu
    K, band = 24, 6
    gt, init = batch.make_poses(K, seed=5, perturb=(0.08, 0.004))
    ci, cj, cp, nc, score = batch.make_constraints(gt, 0, K, 60, band, seed=5)
    con = (ci, cj, cp.numpy(), nc.numpy(), score.numpy())
    dq = batch.delta_q_pairs(gt, 3)
    dd, frame = batch.make_batch_gnss(gt, seed=5)
    for f in dd:
        f.threshold = 10.0
    pre, _, sb0, raw = batch.make_batch_imu(K, seed=5, return_raw=True)
    store = imu.ImuStore(K + 3, max(len(r[2]) for r in raw))
    first = 2          # the chain need not start at the store's edge 0
    store.integrate(first, [imu.edge_arrays(a, g, d, np.zeros(3), np.zeros(3)) for a, g, d in raw])
    back = store.read(first, K - 1)
    for k in range(K - 1):
        preint_cases.check(back[k], pre[k], f"batch edge {k}")
    opts = T.batch_tr_opts(max_iterations=10)
    res = []
    for use_store in (False, True):
        st = batch.BatchStage(K, band, len(ci))
        st.set_constraints(*con); st.set_small_factors(dq, dd, frame)
        if use_store:
            st.set_imu_from_store(store, first)
        else:
            st.set_imu(back)
        res.append(st.solve_tr(init, opts, speed_bias=sb0))
        st.close()
    (pa, sba, ma), (pb, sbb, mb) = res
    print(f"batch: {ma.iterations} iterations, dpose {np.abs(pb - pa).max():.2e}, dsb {np.abs(sbb - sba).max():.2e}")
    assert ma.iterations == mb.iterations and ma.termination == mb.termination, (ma.as_dict(), mb.as_dict())
    assert np.abs(pb - pa).max() < 1e-7 and np.abs(sbb - sba).max() < 1e-6
    store.close()


def test_refusals_launch_nothing(hip):
    from glio_amd import imu
    st = imu.ImuStore(4, 8)
    good = (np.c_[np.full(5, 0.01), np.tile([0, 0, 9.8], (5, 1)), np.zeros((5, 3))], np.r_[0, 0, 9.8, np.zeros(9)])
    st.integrate(0, [good, good, good, good])
    before = bytes(st.read_structs(0, 4))
    long = (np.c_[np.full(9, 0.01), np.tile([0, 0, 9.8], (9, 1)), np.zeros((9, 3))], good[1])
    for first, edges in ((4, [good]), (3, [good, good]), (-1, [good]), (1, [long])):          # past max_edges, negative, longer than max_samples_per_edge
        with pytest.raises(hip.GlioError, match="error -1"):
            st.integrate(first, edges)
    with pytest.raises(hip.GlioError, match="error -1"):
        st.read_structs(3, 2)
    assert bytes(st.read_structs(0, 4)) == before          # nothing ran
    win = synth.make_window(W=3, pts_per_scan=64)
    ctx = hip.Context(win.opts)
    for edges, slots in (([0, 4], [0, 1]), ([0, 1], [0, 2]), ([0, 1, 2], [0, 1, 2])):          # edge past the store, slot past the window, too many edges
        with pytest.raises(hip.GlioError, match="error -1"):
            ctx.set_imu_from_store(st, edges, slots)
    if hip.device_count() > 1:
        other = imu.ImuStore(2, 8, device=1)
        with pytest.raises(hip.GlioError, match="error -1"):
            ctx.set_imu_from_store(other, [0, 1])
        other.close()
    ctx.close()
    from glio_amd import batch
    bs = batch.BatchStage(24, 6, 16)
    with pytest.raises(hip.GlioError, match="error -1"):
        bs.set_imu_from_store(st, 0)          # K - 1 = 23 edges of a store of 4
    bs.close()
    st.close()


def test_a_nan_sample_flags_its_edge_and_no_other(hip):
    """bad DATA, handled by a flag: the edge with the NaN is named by glio_imu_read (GLIO_E_NUMERIC), the other edges of the same launch are intact"""
    from glio_amd import imu
    edges = _ragged_edges(6, seed=11, max_len=40)
    clean = imu.ImuStore(6, 40)
    clean.integrate(0, edges)
    want = clean.read_structs(0, 6)
    bad = [(e[0].copy(), e[1].copy()) for e in edges]
    assert len(bad[2][0]) == 40
    bad[2][0][17, 2] = np.nan
    st = imu.ImuStore(6, 40)
    st.integrate(0, bad)
    with pytest.raises(hip.GlioError, match=r"error -4: IMU edge 2\b"):
        st.read_structs(0, 6)
    with pytest.raises(hip.GlioError, match=r"error -4: IMU edge 2\b"):
        st.read_structs(2, 1)
    assert bytes(st.read_structs(0, 2)) == bytes(want)[:2 * 3736]
    assert bytes(st.read_structs(3, 3)) == bytes(want)[3 * 3736:]
    win = synth.make_window(W=3, pts_per_scan=64)
    ctx = hip.Context(win.opts)
    with pytest.raises(hip.GlioError, match="error -4"):
        ctx.set_imu_from_store(st, [1, 2])          # the flag is known to the host since the read
    ctx.set_imu_from_store(st, [0, 1])
    ctx.close()
    st.integrate(2, [edges[2]])          # integrating the edge again with good samples clears its flag
    assert bytes(st.read_structs(0, 6)) == bytes(want)
    clean.close(); st.close()

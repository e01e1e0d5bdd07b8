"""GPU: the marginal covariance of the window (include/glio_cov.h, covariance_kernels.hip).

1. Matrix families through glio_debug_covariance_of against the family's exact inverse, at every size where the kernels change what they do: the 16-wide
   MFMA / Gram tile, the 32-column panel, the 64-row workgroup tile and forward-substitution round (t - 1, t, t + 1 each, below the one-workgroup limit and
   above it, where panel and tile edges fall at multiples of 32 and at 32 + 64 k), the one-workgroup limit 88 | 89, and 928.  The numpy restatement goes
   through the same assertion first.  "Well conditioned" is the family at kappa = 10, so that one closed-form inverse serves every case.
2. Not positive definite, and every refusal of the header.
3. Real windows against np.linalg.inv of the matrix glio_linearize returns at the same state.
4. Free columns: a front-end context and an epoch no Doppler row touches.
5. No side effect on solve / marginalize_keep / linearize, also with an asynchronous marginalization pending."""
import ctypes as C

import numpy as np
import pytest

import covariance_cases as cases
import covariance_restated as restated
from glio_amd import synth

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
GLIO_OK, GLIO_E_ARG, GLIO_E_NUMERIC = 0, -1, -4
N_MAX = 928
SIZES = [1, 15, 16, 17, 30, 31, 32, 33, 47, 63, 64, 65, 75, 87, 88, 89, 95, 96, 97, 120, 121, 127, 128, 129, 159, 160, 161, 928]
FAMILY = [(n, kappa) for n in SIZES for kappa in (10.0, 1e8)] + [(75, 1e12), (928, 1e12)]


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def big_ctx(hip):
    ctx = hip.Context(synth.default_opts(W=61, pts=64, map_pts=64, n_ddt=13))
    yield ctx
    ctx.close()


def _spd_family(n, kappa, seed):
    """A = D Q diag(lam) Q^T D with log-spaced lam (condition number kappa) and a graded diagonal D (10^-3 .. 10^3, shuffled), the spread of
    the diagonal of a window's H.  Returns A, D, Q and lam (the exact inverse is D^-1 Q diag(1 / lam) Q^T D^-1)."""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.normal(0, 1, (n, n)))
    Q *= np.sign(np.diag(R))
    lam = np.logspace(0, -np.log10(kappa), n)
    A0 = (Q * lam) @ Q.T
    A0 = 0.5 * (A0 + A0.T)
    d = 10.0 ** rng.uniform(-3, 3, n)
    A = d[:, None] * A0 * d[None, :]
    return 0.5 * (A + A.T), d, Q, lam


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("n,kappa", FAMILY, ids=[f"n{n}-k{kappa:.0e}" for n, kappa in FAMILY])
def test_matrix_families(hip, big_ctx, n, kappa):
    """|| D (Sigma - Sigma*) D ||_F <= 4 n kappa eps || D Sigma* D ||_F (the form and constant of test_dense_cholesky_up_to_the_limit), D Sigma* D formed in
    long double; symmetric to the bit; two runs equal to the bit; a request for the last 15 columns and a scattered, shuffled request return the bits the
    all-columns request returns for the same entries."""
    A, d, Q, lam = _spd_family(n, kappa, seed=n + int(np.log10(kappa)))
    want = restated.family_scaled_inverse(Q, lam)
    bound = 4 * n * kappa * EPS
    all_cols = np.arange(n)
    ref, ref_info = restated.covariance_columns(A, all_cols)
    err_ref = restated.scaled_error(ref, want, d)
    assert err_ref <= bound, ("the numpy restatement", n, kappa, err_ref, bound)
    got, info = big_ctx.covariance_of(np.tril(A), all_cols)
    err = restated.scaled_error(got, want, d)
    print(f"n {n} kappa {kappa:.0e}: scaled error device {err:.2e}, numpy {err_ref:.2e}, bound {bound:.2e}; pivots {info.min_pivot:.2e} .. {info.max_pivot:.2e}")
    assert err <= bound, (n, kappa, err, bound)
    assert (info.n, info.n_free, info.n_free_asked, info.bad_pivot) == (n, 0, 0, -1)
    assert info.min_pivot > 0 and info.max_pivot >= info.min_pivot
    # a pivot is 1 / (the last diagonal entry of the leading block's inverse): its relative perturbation is bounded like the inverse's
    assert abs(info.min_pivot - ref_info["min_pivot"]) <= bound * ref_info["min_pivot"] and abs(info.max_pivot - ref_info["max_pivot"]) <= bound * ref_info["max_pivot"]
    assert _same_bits(got, got.T)
    again, _ = big_ctx.covariance_of(np.tril(A), all_cols)
    assert _same_bits(got, again)
    rng = np.random.default_rng(n)
    last = np.arange(max(0, n - 15), n)
    scattered = rng.permutation(n)[:max(1, n // 3)]
    for cols in (last, scattered):
        sub, sub_info = big_ctx.covariance_of(np.tril(A), cols)
        assert sub_info.bad_pivot == -1 and sub.shape == (len(cols), len(cols))
        assert _same_bits(sub, got[np.ix_(cols, cols)]), (n, kappa, cols[:4])


def _not_pd(n, k, seed):
    """B B^T / n + I with the pivot of column k made -1 (relative to the unit diagonal): a_kk = a^T A11^-1 a - 1"""
    rng = np.random.default_rng(seed)
    B = rng.normal(0, 1, (n, n))
    A = B @ B.T / n + np.eye(n)
    if k > 0:
        a = A[:k, k]
        A[k, k] = a @ np.linalg.solve(A[:k, :k], a) - 1.0
    else:
        A[0, 0] = -1.0
    return A


@pytest.mark.parametrize("n", [75, 200])
def test_not_positive_definite(hip, big_ctx, n):
    for k in (n - 1, n // 2):
        A = _not_pd(n, k, seed=n + k)
        none, ref_info = restated.covariance_columns(A, np.arange(n))
        assert none is None and ref_info["bad_pivot"] == k
        for cols in (np.arange(n), np.arange(n - 15, n)):
            with pytest.raises(hip.GlioError) as e:
                big_ctx.covariance_of(np.tril(A), cols)
            assert e.value.code == GLIO_E_NUMERIC and e.value.info.bad_pivot == k, (n, k, e.value.code, e.value.info.as_dict())
            assert np.all(np.isnan(e.value.out))
    # a NaN on the diagonal is a bad pivot, not a free column
    A = _not_pd(n, 0, seed=n)
    A[0, 0] = 1.0 + n
    A[3, 3] = np.nan
    with pytest.raises(hip.GlioError) as e:
        big_ctx.covariance_of(np.tril(A), [0, 1])
    assert e.value.code == GLIO_E_NUMERIC and e.value.info.bad_pivot == 3


def test_refusals(hip):
    win, corr, kw, st = cases.build("w3_gnss")
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, **kw)
    lib, n, W = hip.load(), 15 * win.W + st.n_ddt, win.W
    H0, g0, c0 = ctx.linearize(st)
    out = np.full((n, n), np.nan)
    info = hip.GlioCovInfo()
    cs = st.c()
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    refused = [
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 0, ip([0]), dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), n + 1, ip(list(range(n)) + [0]), dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 2, ip([0, n]), dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 2, ip([-1, 0]), dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 3, ip([4, 7, 4]), dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 1, None, dp, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, C.byref(cs), 1, ip([0]), None, C.byref(info)),
        lib.glio_covariance_columns(ctx._h, None, 1, ip([0]), dp, C.byref(info)),
        lib.glio_covariance_columns(None, C.byref(cs), 1, ip([0]), dp, C.byref(info)),
        lib.glio_covariance_slots(ctx._h, C.byref(cs), 1, ip([W]), dp, C.byref(info)),
        lib.glio_covariance_slots(ctx._h, C.byref(cs), 1, ip([-1]), dp, C.byref(info)),
        lib.glio_covariance_slots(ctx._h, C.byref(cs), 2, ip([1, 1]), dp, C.byref(info)),
        lib.glio_covariance_slots(ctx._h, C.byref(cs), 0, ip([0]), dp, C.byref(info)),
        lib.glio_covariance_slots(ctx._h, C.byref(cs), 1, None, dp, C.byref(info)),
        lib.glio_debug_covariance_of(ctx._h, 0, dp, 1, ip([0]), dp, C.byref(info)),
        lib.glio_debug_covariance_of(ctx._h, n + 1, dp, 1, ip([0]), dp, C.byref(info)),
        lib.glio_debug_covariance_of(ctx._h, 4, None, 1, ip([0]), dp, C.byref(info)),
    ]
    assert refused == [GLIO_E_ARG] * len(refused), refused
    assert np.all(np.isnan(out))
    ms = C.c_float()
    assert lib.glio_covariance_last_device_ms(ctx._h, C.byref(ms)) == -3          # GLIO_E_STATE: no call has completed, nothing was allocated
    H1, g1, c1 = ctx.linearize(st)
    assert _same_bits(H0, H1) and _same_bits(g0, g1) and c0 == c1
    # info may be null; the timing call answers after a completed call
    one = np.full((1, 1), np.nan)
    assert lib.glio_covariance_columns(ctx._h, C.byref(cs), 1, ip([5]), one.ctypes.data_as(C.POINTER(C.c_double)), None) == GLIO_OK
    assert one[0, 0] > 0 and ctx.covariance_last_device_ms() > 0
    ctx.close()


def _ctx_for(hip, name):
    win, corr, kw, st = cases.build(name)
    ctx = hip.Context(win.opts)
    ctx.load_window(win, corr, **kw)
    return ctx, win, st


def _check_golden(name, kappa):
    """tests/golden/covariance_cases.json records kappa_s of the ORACLE's H per case; the device's H differs from it in the last digits (and, where a solve
    precedes it, by the solves' 1e-4 m), which moves a condition number of a few hundred by far less than 2 %"""
    assert abs(kappa - cases.golden()[name]["kappa_s"]) <= 0.02 * kappa, (name, kappa)


def test_window_w2_lidar_imu(hip):
    ctx, win, st = _ctx_for(hip, "w2_lidar_imu")
    H = ctx.linearize(st)[0]
    cov, info = ctx.covariance(st, columns=np.arange(30))
    assert (info.n, info.n_free, info.n_free_asked, info.bad_pivot) == (30, 0, 0, -1) and _same_bits(cov, cov.T)
    _check_golden("w2_lidar_imu", cases.assert_within_bound(cov, H, "w2_lidar_imu")[2])
    ctx.close()


def test_window_w3_gnss(hip):
    ctx, win, st = _ctx_for(hip, "w3_gnss")
    n = 45 + st.n_ddt
    assert st.n_ddt > 0
    H = ctx.linearize(st)[0]
    cov, info = ctx.covariance(st, columns=np.arange(n))
    assert (info.n, info.n_free, info.bad_pivot) == (n, 0, -1) and _same_bits(cov, cov.T)
    _check_golden("w3_gnss", cases.assert_within_bound(cov, H, "w3_gnss")[2])
    ctx.close()


def test_window_w5_prior_from_marginalize_keep(hip):
    w0, c0, w1, c1 = cases.marg_pair()
    ctx = hip.Context(w0.opts)
    ctx.load_window(w0, c0, use_gnss=False, use_prior=False)
    s0 = w0.init.copy(); s0.n_ddt = 0
    sol, _ = ctx.solve(s0)
    ctx.marginalize_keep(sol)
    for s in range(5):
        ctx.set_correspondences(s, *c1[s])
    ctx.set_imu(w1.preints)
    st = w1.init.copy(); st.n_ddt = 0
    H = ctx.linearize(st)[0]
    one, info = ctx.covariance(st, slots=[4])
    assert one.shape == (15, 15) and info.n == 75 and info.n_free == 0
    kappa = cases.assert_within_bound(one, H, "w5_marg {4}", cols=np.arange(60, 75))[2]
    _check_golden("w5_marg", kappa)
    two, _ = ctx.covariance(st, slots=[0, 4])
    cases.assert_within_bound(two, H, "w5_marg {0, 4}", cols=np.r_[np.arange(15), np.arange(60, 75)])
    assert _same_bits(two[15:, 15:], one) and _same_bits(two, two.T)
    default, _ = ctx.covariance(st)                     # neither slots nor columns: the newest keyframe
    assert _same_bits(default, one)
    ctx.close()


def test_window_w20_gnss_prior(hip):
    ctx, win, st = _ctx_for(hip, "w20_gnss_prior")
    n = 300 + st.n_ddt
    H = ctx.linearize(st)[0]
    full, info = ctx.covariance(st, columns=np.arange(n))
    assert (info.n, info.n_free, info.bad_pivot) == (n, 0, -1) and _same_bits(full, full.T)
    _check_golden("w20_gnss_prior", cases.assert_within_bound(full, H, "w20 all")[2])
    newest, _ = ctx.covariance(st, slots=[19])
    cases.assert_within_bound(newest, H, "w20 newest", cols=np.arange(285, 300))
    assert _same_bits(newest, full[285:300, 285:300])
    ctx.close()


def test_window_w61_at_the_limit(hip):
    ctx, win, st = _ctx_for(hip, "w61_gnss")
    assert 15 * 61 + st.n_ddt == N_MAX
    H = ctx.linearize(st)[0]
    cols = np.r_[np.arange(900, 915), np.arange(915, 928)]
    cov, info = ctx.covariance(st, columns=cols)
    assert (info.n, info.n_free, info.bad_pivot) == (N_MAX, 0, -1) and _same_bits(cov, cov.T)
    _check_golden("w61_gnss", cases.assert_within_bound(cov, H, "w61 newest + epochs", cols=cols)[2])
    ctx.close()


def test_free_columns_front_end(hip):
    """window = 1, LiDAR factors only: speed and biases are touched by nothing"""
    ctx, win, st = _ctx_for(hip, "w1_front_end")
    H = ctx.linearize(st)[0]
    assert np.all(np.diag(H)[6:] == 0) and np.all(np.diag(H)[:6] > 0)
    cov, info = ctx.covariance(st, slots=[0])
    assert (info.n, info.n_free, info.n_free_asked, info.bad_pivot) == (15, 9, 9, -1)
    _check_golden("w1_front_end", cases.assert_within_bound(cov, H, "w1 front end")[2])
    assert np.all(np.diag(cov)[6:] == np.inf)
    off = cov.copy()
    off[np.arange(6, 15), np.arange(6, 15)] = 0.0
    assert np.all(off[6:, :] == 0) and np.all(off[:, 6:] == 0)
    pose, info = ctx.covariance(st, columns=[5, 0, 3])
    assert info.n_free == 9 and info.n_free_asked == 0 and _same_bits(pose, cov[np.ix_([5, 0, 3], [5, 0, 3])])
    ctx.close()


def test_free_columns_untouched_epoch(hip):
    """the state carries one clock-drift epoch more than the Doppler rows reference"""
    win, corr, kw, st0 = cases.build("w3_gnss")
    opts = synth.default_opts(3, pts=win.opts.max_points_per_scan, map_pts=win.opts.max_map_points, n_ddt=st0.n_ddt + 1)
    ctx = hip.Context(opts)
    ctx.load_window(win, corr, **kw)
    st = st0.copy()
    st.n_ddt = st0.n_ddt + 1
    st.rcv_ddt = np.r_[st0.rcv_ddt[:st0.n_ddt], 0.0]
    n = 45 + st.n_ddt
    H = ctx.linearize(st)[0]
    assert H[n - 1, n - 1] == 0 and not H[n - 1].any() and not H[:, n - 1].any()
    cov, info = ctx.covariance(st, columns=np.arange(n))
    assert (info.n, info.n_free, info.n_free_asked, info.bad_pivot) == (n, 1, 1, -1)
    cases.assert_within_bound(cov, H, "w3 + untouched epoch")
    assert cov[n - 1, n - 1] == np.inf and not cov[n - 1, :n - 1].any() and not cov[:n - 1, n - 1].any()
    # the columns kept: the bits the same kernels give for the matrix without the free column
    cov0, _ = ctx.covariance_of(np.tril(H[:n - 1, :n - 1]), np.arange(n - 1))
    assert _same_bits(cov0, cov[:n - 1, :n - 1])
    ctx.close()


def _sequence(hip, with_cov, pending):
    """solve, [covariance], marginalize_keep, slide, solve, linearize (which reads the installed prior)"""
    w0, c0, w1, c1 = cases.marg_pair()
    ctx = hip.Context(w0.opts)
    ctx.load_window(w0, c0, use_gnss=False, use_prior=False)
    s0 = w0.init.copy(); s0.n_ddt = 0
    sol, summ = ctx.solve(s0)
    cov = None
    if with_cov and not pending:
        cov = ctx.covariance(sol, slots=[4])[0]
    if pending:
        ctx.marginalize_keep_async(sol)
        if with_cov:
            cov = ctx.covariance(sol, slots=[4])[0]           # finishes the marginalization first, as glio_linearize would, and sees the NEW prior
        ctx.marginalize_keep_finish()
    else:
        ctx.marginalize_keep(sol)
    for s in range(5):
        ctx.set_correspondences(s, *c1[s])
    ctx.set_imu(w1.preints)
    nxt = sol.copy()
    nxt.trans[:-1], nxt.quat[:-1], nxt.speed_bias[:-1] = sol.trans[1:].copy(), sol.quat[1:].copy(), sol.speed_bias[1:].copy()
    nxt.trans[-1], nxt.quat[-1], nxt.speed_bias[-1] = w1.init.trans[-1], w1.init.quat[-1], w1.init.speed_bias[-1]
    if with_cov:
        ctx.covariance(nxt, slots=[4])                        # once more, before the second solve
    sol2, summ2 = ctx.solve(nxt)
    lin = ctx.linearize(sol2)
    ctx.close()
    return sol, summ.as_dict(), sol2, summ2.as_dict(), lin, cov


@pytest.mark.parametrize("pending", [False, True], ids=["synchronous", "marginalization-pending"])
def test_no_side_effect(hip, pending):
    a = _sequence(hip, False, pending)
    b = _sequence(hip, True, pending)
    for sa, sb in ((a[0], b[0]), (a[2], b[2])):
        assert _same_bits(sa.trans, sb.trans) and _same_bits(sa.quat, sb.quat) and _same_bits(sa.speed_bias, sb.speed_bias)
    assert a[1] == b[1] and a[3] == b[3]
    assert _same_bits(a[4][0], b[4][0]) and _same_bits(a[4][1], b[4][1]) and a[4][2] == b[4][2]
    assert b[5] is not None and np.all(np.isfinite(b[5])) and np.all(np.diag(b[5]) > 0)

"""The window's own GNSS and prior kernels (gnss_block, prior_dx_M / prior_rg_block / prior_H_block of factor_kernels.hip, the a.marg form in
k_marg_assemble of solver_kernels.hip), glio_set_gnss's structure branches and the batch stage's k_small_eval / k_small_add / k_small_cost,
against the oracle at the reference's branch inputs (tests/factor_branch_cases.py: a non-zero yaw, lever arms, per-row matrices, masters at
both ends, 2..20 satellites side by side, non-symmetric weights, rows on both sides of the threshold, ratios 0 and 1, unsorted / reversed /
skipping / one-sided pairs, more than GN_MAX_RUNS epochs per pair, (x0^-1 q).w < 0).  tests/test_factor_branch_cases_cpu.py shows that the
cases take those branches and that the oracle's linearisation on them is the sum of its pinned per-factor evaluators.

Gates are those of tests/test_hip_parity.py (cost 1e-10 relative, rel_err(g), rel_err(H) <= 1e-10, assert_pose_parity at its defaults,
rcv_ddt 1e-6), tests/test_hip_marg.py (check_root, 1e-8 on the chained prior) and tests/test_hip_batch_tr.py (1e-11 on H and g, 1e-12 on
the cost, the trust-region gates).  Every test prints the figures it asserts."""
import numpy as np
import pytest

import factor_branch_cases as fc
from glio_amd import ctypes_types as T
from glio_amd import synth
from parity_checks import assert_pose_parity, check_root, rel_err

pytestmark = pytest.mark.gpu

GNSS_NAMES = ["yaw_lever", "masters_sizes", "thresholds", "ratios", "structure_sorted", "structure_shuffled", "structure_reversed", "structure_skip",
              "structure_split", "many_epochs"]
PRIOR_NAMES = [(k, v) for k in ("dense", "steady") for v in fc.PRIOR_VARIANTS]
LAUNCH_FORMS = [0, 1, 2]          # the modes test_linearize_launch_forms parametrises


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


class _Ref:
    """a window, its correspondences and the oracle's linearisation and solve on it -- computed once, shared, never modified"""

    def __init__(self, po, win):
        self.win, self.corr = win, synth.analytic_correspondences(win)
        self.prob = po.Problem(win, self.corr)
        self.H, self.g, self.cost = self.prob.linearize(win.init)
        self.sol, self.summ = self.prob.solve(win.init)
        for a in (self.H, self.g, self.sol.trans, self.sol.quat, self.sol.speed_bias, self.sol.rcv_ddt):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def refs(po):
    out = {name: _Ref(po, win) for name, win in fc.gnss_cases().items()}
    assert sorted(out) == sorted(GNSS_NAMES)
    bases = dict(dense=fc.dense_prior_window(), steady=fc.steady_window(po))
    for kind, base in bases.items():
        out[("base", kind)] = _Ref(po, base)
        for v in fc.PRIOR_VARIANTS:
            out[(kind, v)] = _Ref(po, fc.prior_signs(base, v))
    return out


def _context(hip, ref, mode=None, **use):
    ctx = hip.Context(ref.win.opts)
    ctx.load_window(ref.win, ref.corr, **use)
    if mode is not None:
        assert hip.load().glio_debug_set_merged_linearize(ctx._h, mode) == 0
    return ctx


def _check_linearize(hip, ref, mode, label):
    ctx = _context(hip, ref, mode)
    H, g, c = ctx.linearize(ref.win.init)
    H2, g2, c2 = ctx.linearize(ref.win.init)
    ctx.close()
    ec, eg, eH = abs(c - ref.cost) / abs(ref.cost), rel_err(g, ref.g), rel_err(H, ref.H)
    print(f"{label} launch form {mode}: cost {ec:.2e} rel_err(g) {eg:.2e} rel_err(H) {eH:.2e}")
    assert ec <= 1e-10
    assert eg <= 1e-10
    assert eH <= 1e-10
    assert np.array_equal(H2, H) and np.array_equal(g2, g) and c2 == c, "a second linearisation is bit-identical"


def _check_solve(hip, ref, label):
    ctx = _context(hip, ref)
    sh, mh = ctx.solve(ref.win.init)
    path = hip.load().glio_debug_solver_path(ctx._h)
    ctx.close()
    so, mo = ref.sol, ref.summ
    print(f"{label}: solver path {path}, {mh.iterations} iterations (oracle {mo.iterations}), termination {mh.termination} (oracle {mo.termination}), "
          f"cost {mh.initial_cost:.1f} -> {mh.final_cost:.1f}, max |dt| {np.linalg.norm(sh.trans - so.trans, axis=1).max():.2e} m, "
          f"max |d rcv_ddt| {np.abs(sh.rcv_ddt - so.rcv_ddt).max():.2e}")
    assert mh.iterations == mo.iterations and mh.termination == mo.termination
    assert_pose_parity(sh, so)
    if so.n_ddt:
        assert np.abs(sh.rcv_ddt - so.rcv_ddt).max() <= 1e-6
    return path


# ------------------------------------------------------------------------------------------------ GNSS cases
@pytest.mark.parametrize("mode", LAUNCH_FORMS)
@pytest.mark.parametrize("name", GNSS_NAMES)
def test_gnss_case_linearisation(hip, refs, name, mode):
    _check_linearize(hip, refs[name], mode, name)


@pytest.mark.parametrize("name", GNSS_NAMES)
def test_gnss_case_solve(hip, refs, name):
    _check_solve(hip, refs[name], name)


def test_shuffled_handover_is_the_sorted_one_bit_for_bit(hip, refs):
    """glio_set_gnss sorts stably by (pair, epoch); the shuffle keeps the order inside a pair / an epoch (fc.group_preserving_shuffle), so the
    kernels must see the same arrays"""
    out = []
    for name in ("structure_sorted", "structure_shuffled"):
        ctx = _context(hip, refs[name])
        out.append(ctx.linearize(refs[name].win.init))
        ctx.close()
    (Ha, ga, ca), (Hb, gb, cb) = out
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and ca == cb


def test_many_epochs_reads_runs_beyond_the_lds_table(hip, refs):
    win = refs["many_epochs"].win
    per = fc.epochs_per_pair(win)
    assert max(per.values()) > 32, "the case must keep more epochs per pair than GN_MAX_RUNS"
    # the clock-drift blocks of the epochs behind the table, on their own: rows / columns 15 W + e of the runs 32.. of each pair
    ctx = _context(hip, refs["many_epochs"])
    H, g, _ = ctx.linearize(win.init)
    ctx.close()
    late = []
    for pair in per:
        ep = sorted({f.epoch for f in win.dop if (f.slot_i, f.slot_j) == pair})
        late += [15 * win.W + e for e in ep[32:]]
    assert len(late) == sum(max(0, v - 32) for v in per.values()) > 0
    eH, eg = rel_err(H[late, :], refs["many_epochs"].H[late, :]), rel_err(g[late], refs["many_epochs"].g[late])
    print(f"many_epochs, {len(late)} epochs behind the table: rel_err(g) {eg:.2e} rel_err(H rows) {eH:.2e}")
    assert eH <= 1e-10 and eg <= 1e-10


# ------------------------------------------------------------------------------------------------ the prior's w < 0 branch
@pytest.mark.parametrize("mode", LAUNCH_FORMS)
@pytest.mark.parametrize("kind,variant", PRIOR_NAMES)
def test_prior_sign_linearisation(hip, refs, kind, variant, mode):
    ref = refs[(kind, variant)]
    assert fc.negative_w_blocks(ref.win.prior, ref.win.init) > 0
    _check_linearize(hip, ref, mode, f"prior_{kind}_{variant}")


@pytest.mark.parametrize("kind,variant", PRIOR_NAMES)
def test_prior_sign_solve(hip, refs, kind, variant):
    _check_solve(hip, refs[(kind, variant)], f"prior_{kind}_{variant}")


@pytest.mark.parametrize("kind,variant", PRIOR_NAMES)
def test_prior_sign_is_the_same_problem(hip, refs, kind, variant):
    """-q is the rotation q: the device's H, g, cost with the negated quaternions equal its own with the positive ones.  Prior, LiDAR and GNSS
    factors only: the reference's ImuFactor is NOT invariant (its attitude residual 2 vec(dq^-1 q_i^-1 q_j) changes sign with q_i and the full
    15 x 15 information matrix couples it to the other rows; tests/test_factor_branch_cases_cpu.py shows both on the oracle)."""
    out = []
    for key in ((kind, variant), ("base", kind)):
        ctx = _context(hip, refs[key], use_imu=False)
        out.append(ctx.linearize(refs[key].win.init))
        ctx.close()
    (Hn, gn, cn), (Hp, gp, cp) = out
    print(f"prior_{kind}_{variant} against +q: cost {abs(cn - cp) / abs(cp):.2e} rel_err(g) {rel_err(gn, gp):.2e} rel_err(H) {rel_err(Hn, Hp):.2e}")
    assert abs(cn - cp) <= 1e-12 * abs(cp)
    assert rel_err(gn, gp) <= 1e-10 and rel_err(Hn, Hp) <= 1e-10


@pytest.mark.parametrize("kind,variant", PRIOR_NAMES)
def test_prior_sign_marginalisation_and_the_chained_prior(hip, refs, kind, variant):
    ref = refs[(kind, variant)]
    sol = ref.sol.copy()
    ctx = _context(hip, ref)
    out_o = ref.prob.marginalize(sol)
    assert fc.negative_w_blocks(ref.win.prior, sol) > 0, "k_marg_assemble itself must meet the prior on the w < 0 side"
    check_root(ctx.marginalize(sol), out_o)            # k_marg_assemble takes the prior through the a.marg form of M
    # the chained path: the prior the device keeps drives the next linearisation like the oracle's output does
    nxt = sol.copy()
    nxt.trans += 0.03
    nxt.speed_bias[:, :3] += 0.02
    nxt.quat[1] *= -1.0
    assert fc.negative_w_blocks(out_o, nxt) > 0, "the chained prior must be entered on the w < 0 side too"
    ctx.marginalize_keep(sol)
    Hh, gh, ch = ctx.linearize(nxt)
    ctx.set_prior(out_o)
    Ho, go, co = ctx.linearize(nxt)
    ctx.close()
    print(f"prior_{kind}_{variant} chained: cost {abs(ch - co) / abs(co):.2e} rel_err(g) {rel_err(gh, go):.2e} rel_err(H) {rel_err(Hh, Ho):.2e}")
    assert rel_err(Hh, Ho) <= 1e-8 and rel_err(gh, go) <= 1e-8 and abs(ch - co) <= 1e-8 * abs(co)


# ------------------------------------------------------------------------------------------------ the batch stage's small factors
@pytest.fixture(scope="module")
def batch_case():
    return fc.batch_problem()


def test_batch_small_factors_at_the_branch_inputs(po, batch_case):
    from glio_amd import batch
    P = batch_case
    K, band, con = P["K"], P["band"], P["con"]
    st = batch.BatchStage(K, band, len(con[0]))
    st.set_constraints(*con)
    st.set_small_factors(P["dq"], P["dd"], P["frame"])
    Hg = st.new_hg()
    st.linearize(P["init"], Hg)
    lidar_only = Hg.cpu().numpy().copy()
    st.add_small(P["init"], Hg)
    got = Hg.cpu().numpy()
    Hg2 = st.new_hg(); st.linearize(P["init"], Hg2); st.add_small(P["init"], Hg2)
    again = Hg2.cpu().numpy()
    st.close()
    H, g, cost = po.BatchProblem(K, band, *con, dq=P["dq"], dd=P["dd"], frame=P["frame"]).linearize(P["init"])
    want = np.concatenate([H.ravel(), g.ravel(), [cost]])
    nH = K * (band + 1) * 36
    eH = np.abs(got[:nH] - want[:nH]).max() / np.abs(want[:nH]).max()
    eg = np.abs(got[nH:-1] - want[nH:-1]).max() / np.abs(want[nH:-1]).max()
    ec = abs(got[-1] - want[-1]) / want[-1]
    print(f"batch small factors: H {eH:.2e} g {eg:.2e} cost {ec:.2e}")
    assert np.abs(got - lidar_only).max() > 1.0, "the small factors must contribute"
    assert eH <= 1e-11
    assert eg <= 1e-11
    assert ec <= 1e-12
    assert np.array_equal(again, got)


def test_batch_trust_region_solve_at_the_branch_inputs(po, batch_case):
    from glio_amd import batch
    P = batch_case
    K, band, con = P["K"], P["band"], P["con"]
    st = batch.BatchStage(K, band, len(con[0]))
    st.set_constraints(*con)
    st.set_small_factors(P["dq"], P["dd"], P["frame"])
    opts = T.batch_tr_opts(max_iterations=30)
    poses, summ = st.solve_tr(P["init"], opts)
    st.close()
    want, wsum = po.BatchProblem(K, band, *con, dq=P["dq"], dd=P["dd"], frame=P["frame"]).solve(P["init"], opts)
    print(f"batch solve: {summ.iterations} iterations (oracle {wsum.iterations}), cost {summ.initial_cost:.1f} -> {summ.final_cost:.1f}, max |dpose| {np.abs(poses - want).max():.2e}")
    assert summ.iterations == wsum.iterations and summ.successful_steps == wsum.successful_steps and summ.termination == wsum.termination, (summ.as_dict(), wsum.as_dict())
    assert np.isclose(summ.initial_cost, wsum.initial_cost, rtol=1e-12)
    assert np.isclose(summ.final_cost, wsum.final_cost, rtol=1e-9)
    assert np.abs(poses - want).max() < 1e-8

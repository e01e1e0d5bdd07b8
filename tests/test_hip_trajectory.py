"""The every-frame trajectory on the device (csrc/trajectory_kernels.hip, glio_traj_*) against the numpy restatement (tests/trajectory_restated.py): dead
reckoning and measurements to 1e-12 relative to max(1, |value|), the local graph with equal termination, iteration count and accept / reject sequence and
poses within 1e-9 (the figure tests/test_hip_odometry.py uses) on every case of the shared builder, the batch form bit for bit against one gap at a time,
and the refusals.

Largest deviations seen on an MI355X (also in DESIGN.md section 9): dead-reckoned rows and measurements 0 (bit-equal) against the bound 1e-12; solved poses
1.1e-15 and costs 1.1e-16 against the bound 1e-9, on the builder's six cases (1, 2, 3, 11 and 32 frames, and the far anchor: NO_CONVERGENCE after 15 iterations,
3 steps accepted, 12 rejected); the resolve of six gaps against the restatement 2.8e-17.

Every trust-region branch, end and pass boundary (tr.branch_cases(), tr.limit_cases(), tr.resolve_cases(); one function, tr.assert_same_solve, holds the device
and -- in tests/test_trajectory_restated.py -- deliberately wrong restatements to them).
Reached on the device: the dogleg's gn, cauchy and interp (c > 0) branches in each pass-count class of evaluate() (N <= 9, 10-18, 19-27, 28-32); the radius
rules grow, keep, shrink-on-accept and reject on gaps of more than one pass; the ends FUNCTION_TOLERANCE, PARAMETER_TOLERANCE (poses at 1e5 and 1e7 m, at
iteration 2 and 1), GRADIENT_TOLERANCE (through a push and through a resolve), NO_CONVERGENCE and FAILURE at entry; nominal gaps of 9, 10, 18, 19, 27 and 28
frames; max_iterations 0, 1 and 32 (bit 31 of accepted_mask); resolves of 0 to 32 frames with consistent, disturbed and loop-closure-sized right rows.
Declared unreachable through the public API (the reasons in tr.branch_cases()): interp with c <= 0 (Cauchy-Schwarz), the mu escalation and five invalid
steps (the model is J'J plus a positive diagonal), MIN_RADIUS (about 120 rejections, max_iterations <= 32), a non-finite candidate cost.
The gate of a case is max(1e-9, 100 x its floor), relative to max(1, |value|); the floor is the restatement against itself with every input one ulp up.
Floors and the largest deviations seen on an MI355X (poses / costs; every case not named: floor <= 3e-15, gate 1e-9, deviation <= 3.3e-16):
  cauchy_1 floor 1.1e-9: 1.3e-9 / 2.2e-16    cauchy_2 6.0e-10: 1.3e-9 / 5.2e-14     cauchy_10 1.2e-8: 1.2e-8 / 1.0e-9     cauchy_19 6.7e-9: 4.5e-9 / 9.4e-10
  cauchy_32 4.8e-8: 2.1e-8 / 1.8e-9          interp_9 1.3e-11: 7.7e-12 / 3.4e-14    interp_10 1.8e-11: 1.6e-11 / 5.0e-15  interp_18 2.1e-13: 9.5e-14 / 6.9e-15
  interp_18_far 2.5e-11: 5.0e-11 / 3.6e-14   interp_19 6.4e-12: 1.4e-12 / 3.8e-16   interp_27 3.6e-11: 6.4e-11 / 2.7e-15  interp_28 3.6e-9: 2.5e-9 / 1.6e-11
  interp_32 2.1e-13: 2.7e-13 / 4.0e-16       interp_18_far at 32 iterations 1.6e-11: 2.0e-11 / 5.9e-16
  resolve: closures of tens of metres floors 1.4e-14 .. 4.1e-13, deviations up to 2.9e-13; the two far closures (1e4 m and more, the Cauchy branch) floors
  1.0e-8 and 6.6e-9, deviations 4.6e-9 and 1.6e-8 / 8.0e-10.
The device stays within a few times the restatement's own floor everywhere: the far-jump cases are ill conditioned, not wrongly computed."""
import numpy as np
import pytest

import trajectory_restated as tr
from glio_amd import trajectory

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from glio_amd import capi
    assert capi.device_count() >= 1, "no HIP device: the product path has no fallback"
    return capi


def rel_dev(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a, np.float64).tobytes() for a in arrays)


def summary_key(s):
    return (s["termination"], s["iterations"], s["successful_steps"], s["n_frames"], s["accepted_mask"], s["flag"],
            np.float64(s["initial_cost"]).tobytes(), np.float64(s["final_cost"]).tobytes())


HEADINGS = {"trace": (0.0, 0.0, 1.0, 0.2), "diag_x": (1.0, 0.0, 0.0, 3.1), "diag_y": (0.0, 1.0, 0.0, 3.1), "diag_z": (0.0, 0.0, 1.0, 3.1)}


def test_dead_reckoning_and_measurements(hip):
    """gap sizes 0, 1, 2, 3 and the maximum; 0 whole samples (start row + closing row), 1, and the configured maximum of rows; all four
    Quaterniond(Matrix3d) branches"""
    max_rows = 2 * (trajectory.MAX_FRAMES + 1)
    st = trajectory.TrajectoryStore(max_gaps=16, max_samples_per_gap=max_rows)
    shapes = [("n0_full", dict(n_frames=0, samples_per_segment=max_rows - 2, heading=HEADINGS["trace"])),
              ("n1_none", dict(n_frames=1, samples_per_segment=0, heading=HEADINGS["diag_x"])),
              ("n2_one", dict(n_frames=2, samples_per_segment=1, heading=HEADINGS["diag_y"])),
              ("n3", dict(n_frames=3, samples_per_segment=[0, 1, 5, 2], heading=HEADINGS["diag_z"])),
              ("n32", dict(n_frames=trajectory.MAX_FRAMES, samples_per_segment=0, heading=HEADINGS["trace"]))]
    seen, worst = set(), 0.0
    for k, (name, kw) in enumerate(shapes):
        c = tr.make_gap(seed=100 + k, gyr_scale=0.05, **kw)
        if name == "n0_full":
            assert len(c["samples"]) == max_rows
        rows, meas, sol, summ, branches = tr.restate(c)
        seen.update(branches)
        st.push(k, c)
        got = st.read(k)
        d = max(rel_dev(got.dead_reckoned, rows), rel_dev(got.measurements, meas))
        print(f"{name}: dead reckoning / measurements deviate by {d:.3e}, branches {sorted(set(branches))}")
        worst = max(worst, d)
        assert d <= 1e-12, (name, d)
        assert got.summary["n_frames"] == c["n_frames"] and got.summary["flag"] == 0
        if c["n_frames"] == 0:
            assert got.summary["termination"] == trajectory.NOT_SOLVED and got.summary["iterations"] == 0 and got.solved.shape == (0, 7)
    assert seen == {0, 1, 2, 3}, seen
    print(f"largest deviation {worst:.3e}")
    st.close()


def test_clamped_sample_and_unclamped_start_row(hip):
    """from a raw IMU buffer through trajectory.frame_samples, against the reference's loop read straight off the buffer"""
    rng = np.random.default_rng(9)
    stamps = 100.0 + np.cumsum(rng.uniform(0.004, 0.006, 80))
    acc = np.array([0.0, 0.0, 9.8]) + rng.normal(0, 0.5, (80, 3))
    gyr = rng.normal(0, 0.2, (80, 3))
    acc[5] = [30.0, 0.0, 9.8]; acc[6] = [30.0, 0.0, 9.8]          # around the first frame stamp: the unclamped start row
    acc[12] = [-40.0, 22.0, 31.0]                                  # a whole sample beyond every clamp
    fs = [stamps[5] + 0.002, stamps[20] + 0.001, stamps[33], stamps[50] + 0.003]
    P, V, R, g = rng.normal(size=3), rng.normal(size=3), tr.q2R_np(tr.rot_q([0.2, 0.1, 1.0], 0.7)), np.array([0, 0, 9.805])
    rows, _, _ = tr.fill_in_direct(stamps, acc, gyr, fs, 5, P, V, R, g)
    offs, smp, _ = trajectory.frame_samples(stamps, acc, gyr, fs, 5)
    assert smp[0, 1] > 29.0 and list(smp[7, 1:4]) == [-15.0, 15.0, 18.0]
    prev = np.concatenate([P, tr.quat_from_matrix(R)[0]])
    st = trajectory.TrajectoryStore(max_gaps=1)
    st.push_gap(0, 2, offs, smp, np.concatenate([P, V, R.reshape(-1)]), g, prev, prev, rows[-1])
    got = st.read(0)
    d = max(rel_dev(got.dead_reckoned, rows), rel_dev(got.measurements, tr.measurements(prev, rows)))
    print(f"deviation {d:.3e}")
    assert d <= 1e-12
    st.close()


def test_solve_against_the_restatement(hip):
    """every case of the shared builder (its margins are asserted there): the decisions are equal, the poses within 1e-9"""
    cases = tr.cases()
    st = trajectory.TrajectoryStore(max_gaps=len(cases))
    for k, (name, c, _) in enumerate(cases):
        st.push(k, c)
    worst = 0.0
    for k, (name, c, (rows, meas, sol, summ, _)) in enumerate(cases):
        got = st.read(k)
        s = got.summary
        d = float(np.abs(got.solved - sol).max())
        print(f"{name}: {got.termination_name} after {s['iterations']} iterations, {s['successful_steps']} accepted (mask {s['accepted_mask']:#x}), "
              f"cost {s['initial_cost']:.6e} -> {s['final_cost']:.6e}; poses deviate by {d:.3e}, costs by "
              f"{abs(s['initial_cost'] - summ['initial_cost']):.3e} / {abs(s['final_cost'] - summ['final_cost']):.3e}")
        assert (s["termination"], s["iterations"], s["successful_steps"], s["accepted_mask"]) == \
            (summ["termination"], summ["iterations"], summ["successful_steps"], summ["accepted_mask"]), (name, s, summ)
        assert d <= 1e-9, (name, d)
        assert abs(s["initial_cost"] - summ["initial_cost"]) <= 1e-9 * max(1.0, summ["initial_cost"])
        assert abs(s["final_cost"] - summ["final_cost"]) <= 1e-9 * max(1.0, summ["final_cost"])
        worst = max(worst, d)
    print(f"largest pose deviation {worst:.3e}")
    st.close()


def _drive(n_gaps):
    """n_gaps different gaps and keyframe rows [n_gaps + 1] that give every gap its own anchors up to a rigid motion (row k + 1 = row k (+) the gap's own
    left-to-right relative pose, slightly disturbed)"""
    rng = np.random.default_rng(77)
    gaps = [tr.make_gap(seed=300 + k, n_frames=k % 6, samples_per_segment=1 + k % 3) for k in range(n_gaps)]
    kf = [np.concatenate([rng.normal(size=3), tr.rot_q(rng.normal(size=3), 0.4)])]
    for c in gaps:
        rel = tr.measurements(c["anchor_left"], [c["anchor_right"]])[0]
        rel[4:7] += 0.01 * rng.normal(size=3)
        kf.append(tr.compose(kf[-1], rel))
    return gaps, np.array(kf)


def _batch_against_single(gaps, kf, max_samples):
    """the gaps resolved in one launch (twice) and one launch per gap: (solved bits, summary keys) of the batch, after asserting all three equal"""
    n = len(gaps)
    runs = []
    for mode in ("batch", "batch", "single"):
        st = trajectory.TrajectoryStore(max_gaps=n, max_samples_per_gap=max_samples)
        for k, c in enumerate(gaps):
            st.push(k, c)
        before = [st.read(k) for k in range(n)]
        if mode == "batch":
            summ = st.resolve(0, kf)
        else:
            summ = [st.resolve(k, kf[k:k + 2])[0] for k in range(n)]
        after = [st.read(k) for k in range(n)]
        for k in range(n):          # a resolve keeps the dead-reckoned rows and the measurements
            assert bits(before[k].dead_reckoned, before[k].measurements) == bits(after[k].dead_reckoned, after[k].measurements)
            assert summary_key(after[k].summary) == summary_key(summ[k])
        runs.append(([bits(r.solved) for r in after], [summary_key(s) for s in summ]))
        st.close()
    assert runs[0] == runs[1], "two identical runs differ"
    assert runs[0] == runs[2], "a gap in the batch differs from the gap alone"
    return runs[0]


def test_batch_resolve_is_the_gaps_one_at_a_time(hip):
    gaps, kf = _drive(64)
    run = _batch_against_single(gaps, kf, 64)
    terms = [k[0] for k in run[1]]
    print("terminations of the batch:", {trajectory.TERMINATION_NAMES[t]: terms.count(t) for t in sorted(set(terms))})


def test_batch_resolve_of_the_mixed_set_is_the_gaps_one_at_a_time(hip):
    """the gaps of tr.resolve_cases() -- 0 to 32 frames, consistent, disturbed and loop-closure-sized, every dogleg branch -- in one launch and one at a time:
    equal bits, solved rows and summaries"""
    gaps, kf = tr.resolve_cases()
    run = _batch_against_single([g["case"] for g in gaps], kf, 128)
    terms = [k[0] for k in run[1]]
    assert len(set(terms)) >= 4, terms
    print("terminations of the batch:", {trajectory.TERMINATION_NAMES[t]: terms.count(t) for t in sorted(set(terms))})


def test_resolve_against_the_restatement(hip):
    gaps, kf = _drive(6)
    st = trajectory.TrajectoryStore(max_gaps=6, max_samples_per_gap=64)
    for k, c in enumerate(gaps):
        st.push(k, c)
    summ = st.resolve(0, kf)
    for k, c in enumerate(gaps):
        rows, meas, _, _, _ = tr.restate(c)
        N = c["n_frames"]
        want, ws, _ = tr.local_graph(meas, kf[k], kf[k + 1], tr.resolve_init(meas, kf[k], N))
        if N:
            tr.assert_margins(f"resolve {k}", ws)
        got = st.read(k)
        d = float(np.abs(got.solved - want).max()) if N else 0.0
        print(f"gap {k} ({N} frames): {trajectory.TERMINATION_NAMES[summ[k]['termination']]} after {summ[k]['iterations']}, poses deviate by {d:.3e}")
        assert (summ[k]["termination"], summ[k]["iterations"], summ[k]["accepted_mask"]) == (ws["termination"], ws["iterations"], ws["accepted_mask"])
        assert d <= 1e-9
    st.close()


def _refused(fn, code):
    from glio_amd import capi
    with pytest.raises(capi.GlioError) as e:
        fn()
    assert f"error {code}:" in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_leave_the_store_as_it_was(hip):
    F, rows = 4, 24
    st = trajectory.TrajectoryStore(max_gaps=4, max_frames_per_gap=F, max_samples_per_gap=rows)
    good = [tr.make_gap(seed=400 + k, n_frames=k + 1, samples_per_segment=1) for k in range(3)]
    for k, c in enumerate(good):
        st.push(k, c)

    def snapshot():
        out = []
        for k in range(3):
            r = st.read(k)
            out.append((bits(r.dead_reckoned, r.measurements, r.solved), summary_key(r.summary)))
        return out
    before = snapshot()
    ok = good[1]

    def push(gap=1, **kw):
        c = dict(ok, **kw)
        return lambda: st.push(gap, c)
    _refused(push(gap=4), -1)
    _refused(push(gap=-1), -1)
    too_many = tr.make_gap(seed=1, n_frames=F + 1, samples_per_segment=0)
    _refused(lambda: st.push(1, too_many), -1)                                   # max_frames_per_gap + 1
    at_limit = tr.make_gap(seed=2, n_frames=F, samples_per_segment=0)
    too_long = tr.make_gap(seed=3, n_frames=0, samples_per_segment=rows - 1)     # rows + 1 sample rows
    _refused(lambda: st.push(1, too_long), -1)
    bad = ok["samples"].copy(); bad[2, 5] = np.nan
    _refused(push(samples=bad), -1)
    bad = ok["samples"].copy(); bad[1, 0] = -1e-3
    _refused(push(samples=bad), -1)
    _refused(push(start_state=np.r_[np.inf, ok["start_state"][1:]]), -1)
    _refused(push(anchor_right=np.r_[ok["anchor_right"][0:3], 0, 0, 0, 0]), -1)
    _refused(push(prev_row=np.r_[ok["prev_row"][0:3], 0, 0, 0, 0]), -1)
    kf = np.array([ok["anchor_left"]] * 5)
    _refused(lambda: st.resolve(0, kf), -3)                                      # gap 3 was never pushed
    _refused(lambda: st.resolve(0, np.r_[kf[:2], [np.r_[kf[0][0:3], 0, 0, 0, 0]]]), -1)
    _refused(lambda: st.read(3), -3)
    assert snapshot() == before
    st.push(3, at_limit)                                                         # the maximum itself is taken
    assert st.read(3).summary["n_frames"] == F
    assert snapshot() == before

    # a non-finite value arising on the device flags the gap; reading names it; pushing it again clears the flag
    wild = ok["samples"].copy(); wild[1:, 4:7] = 1e200
    st.push(1, dict(ok, samples=wild))
    msg = _refused(lambda: st.read(1), -4)
    assert "gap 1" in msg
    assert st.read(1, check=False).summary["flag"] == 1
    assert snapshot_one(st, 0) == before[0] and snapshot_one(st, 2) == before[2]
    st.push(1, ok)
    assert snapshot() == before
    st.close()


def snapshot_one(st, k):
    r = st.read(k)
    return (bits(r.dead_reckoned, r.measurements, r.solved), summary_key(r.summary))


# ------------------------------------------------------------------ every trust-region branch, end and pass boundary (tr.branch_cases())
def _taken(summ):
    br = [b for b, _ in summ["census"]]
    ru = [r for _, r in summ["census"]]
    return ("/".join(f"{b} {br.count(b)}" for b in tr.DOGLEG_BRANCHES if b in br) or "-") + "; " + ("/".join(f"{r} {ru.count(r)}" for r in tr.RADIUS_RULES if r in ru) or "-")


def _hold_to_restatement(st, k, b, flag=0):
    """gap k of the store against the case's restatement: inputs to 1e-12, the solve by tr.assert_same_solve with the case's own gate; prints the table row"""
    rows, meas, sol, summ, _ = b["restated"]
    got = st.read(k, check=False)
    d_in = max(rel_dev(got.dead_reckoned, rows), rel_dev(got.measurements, meas))
    s = got.summary
    print(f"{b['name']:>24}: N {s['n_frames']:2d}, {_taken(summ)}; {got.termination_name} after {s['iterations']} ({s['successful_steps']} accepted, mask {s['accepted_mask']:#x}); "
          f"floor {b['floor']:.1e} gate {b['gate']:.1e}", end="")
    assert d_in <= 1e-12, (b["name"], d_in)
    assert s["n_frames"] == b["gap"]["n_frames"] and s["flag"] == flag, (b["name"], s)
    d_pose, d_cost = tr.assert_same_solve(b["name"], got.solved, s, sol, summ, b["gate"])
    print(f"; inputs deviate by {d_in:.1e}, poses {d_pose:.1e}, costs {d_cost:.1e}")
    return got, d_pose, d_cost


def test_solve_on_every_branch_case(hip):
    """all of tr.branch_cases() in one store: gn, cauchy and interp in every pass-count class, the four radius rules over more than one pass, the ends
    FUNCTION / PARAMETER / GRADIENT tolerance, NO_CONVERGENCE and FAILURE at entry, a nominal gap on both sides of every pass boundary"""
    cases = tr.branch_cases()
    st = trajectory.TrajectoryStore(max_gaps=len(cases), max_samples_per_gap=128)
    for k, b in enumerate(cases):
        st.push(k, b["gap"])
    worst = (0.0, 0.0)
    for k, b in enumerate(cases):
        _, d_pose, d_cost = _hold_to_restatement(st, k, b, flag=1 if b["restated"][3]["termination"] == trajectory.FAILURE else 0)
        worst = (max(worst[0], d_pose), max(worst[1], d_cost))
    print(f"largest deviation: poses {worst[0]:.3e}, costs {worst[1]:.3e}")
    st.close()


def test_failure_at_entry(hip):
    by_name = {b["name"]: b for b in tr.branch_cases()}
    bad, good = by_name["failure_at_entry_3"], [by_name["nominal_9"], by_name["interp_10"]]
    st = trajectory.TrajectoryStore(max_gaps=3, max_samples_per_gap=128)
    st.push(0, good[0]["gap"]); st.push(2, good[1]["gap"])
    before = [snapshot_one(st, 0), snapshot_one(st, 2)]
    st.push(1, good[0]["gap"])
    st.push(1, bad["gap"])
    got = st.read(1, check=False)
    s = got.summary
    assert (s["termination"], s["iterations"], s["successful_steps"], s["accepted_mask"], s["flag"]) == (trajectory.FAILURE, 0, 0, 0, 1), s
    assert bits(got.solved) == bits(got.dead_reckoned[:3])
    assert rel_dev(got.dead_reckoned, bad["restated"][0]) <= 1e-12
    assert [snapshot_one(st, 0), snapshot_one(st, 2)] == before
    msg = _refused(lambda: st.read(1), -4)
    assert "gap 1" in msg
    st.push(1, good[0]["gap"])
    assert snapshot_one(st, 1) == before[0]
    assert [snapshot_one(st, 0), snapshot_one(st, 2)] == before
    st.close()


def test_max_iterations_ends(hip):
    """stores created with max_iterations 0, 1 and 32 (glio_traj_create takes 0 .. 32)"""
    for b in tr.limit_cases():
        m = b["max_iterations"]
        st = trajectory.TrajectoryStore(max_gaps=1, max_samples_per_gap=128, max_iterations=m)
        st.push(0, b["gap"])
        got, _, _ = _hold_to_restatement(st, 0, b)
        s = got.summary
        assert s["termination"] == trajectory.NO_CONVERGENCE and s["iterations"] == m
        if m == 0:
            assert bits(got.solved) == bits(got.dead_reckoned[:b["gap"]["n_frames"]])
            assert np.float64(s["final_cost"]).tobytes() == np.float64(s["initial_cost"]).tobytes() and s["accepted_mask"] == 0
        if m == 32:
            assert s["accepted_mask"] >> 31 == 1 and bin(s["accepted_mask"]).count("1") == s["successful_steps"]
        st.close()


def test_resolve_across_pass_boundaries_and_branches(hip):
    """tr.resolve_cases(): gaps of 0, 1, 9, 10, 18, 19, 27, 28 and 32 frames solved again in one launch between keyframe rows that leave some consistent
    (GRADIENT_TOLERANCE before the first iteration, the composed chain delivered), disturb some by a centimetre and move others by a loop-closure-sized
    correction chosen on the CPU so that cauchy and interp arise; against tr.local_graph from tr.resolve_init by tr.assert_same_solve"""
    gaps, kf = tr.resolve_cases()
    st = trajectory.TrajectoryStore(max_gaps=len(gaps), max_samples_per_gap=128)
    for k, g in enumerate(gaps):
        st.push(k, g["case"])
    summ = st.resolve(0, kf)
    worst = 0.0
    for k, g in enumerate(gaps):
        N, ws = g["spec"]["n_frames"], g["summary"]
        got = st.read(k)
        assert summary_key(got.summary) == summary_key(summ[k]) and got.summary["n_frames"] == N and got.summary["flag"] == 0
        assert rel_dev(got.measurements, g["meas"]) <= 1e-12
        print(f"{g['name']:>36}: {_taken(ws)}; {got.termination_name} after {summ[k]['iterations']} (mask {summ[k]['accepted_mask']:#x}); floor {g['floor']:.1e} gate {g['gate']:.1e}", end="")
        d_pose, d_cost = tr.assert_same_solve(g["name"], got.solved, summ[k], g["poses"], ws, g["gate"])
        print(f"; poses deviate by {d_pose:.1e}, costs {d_cost:.1e}")
        worst = max(worst, d_pose, d_cost)
        if g["spec"]["kind"] == "consistent" and N:
            assert (summ[k]["termination"], summ[k]["iterations"]) == (trajectory.GRADIENT_TOLERANCE, 0)
            assert rel_dev(got.solved, tr.resolve_init(g["meas"], kf[k], N)) <= 1e-12
    print(f"largest deviation {worst:.3e}")
    st.close()

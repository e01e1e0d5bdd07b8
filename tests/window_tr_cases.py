"""Windows on which the sliding-window solve's trust-region loop takes every branch it has, and a classifier that says which branch each
iteration took.  tests/test_window_tr_cases_cpu.py shows that the cases do what the table claims and that the oracle and the numpy
restatement of the Ceres loop (tests/np_ceres.py) agree on them; tests/test_hip_window_tr_branches.py holds every factorisation path of the
device to the oracle on them, whole solves and every prefix.

A case is a dict:
  window    arguments of synth.make_window (256 points per keyframe unless the case says otherwise: the loop does not depend on the count)
  opts      overrides of the window's glio_opts
  far       None or (sigma, seed): the start is the window's own initial state moved as tests/test_hip_solve_ends.py's _far does
  use       the use_gnss / use_prior / use_imu flags of po.Problem and Context.load_window
  corrupt   None or the IMU edge whose bias Jacobian overflows (tests/test_oracle_tr_pins.py: every factorisation fails)
  marg      True: keyframes 1..W of a W+1 stream with the prior the ORACLE's marginalization of keyframe 0 leaves (block diagonal by keyframe)
  expect    the labels the case is in the table for: step kinds, outcomes, termination (test_window_tr_cases_cpu.py asserts them)

classify(name) runs both CPU witnesses and returns, per iteration, step kind, ratio, outcome, the radius before and after, the state after
it (both witnesses'), and every quantity the loop compares with a threshold.  The step kind is computed here from np_ceres.Dogleg's grad,
gn, alpha and radius by a recording subclass; nothing np_ceres computes is changed.

Branches no case reaches, after a bounded search (the probes are described where they apply):
  * dogleg interpolation with c = b.a - |a|^2 <= 0.  With a = -alpha g the Cauchy point and b the Gauss-Newton point of a positive definite
    model, a.(b - a) >= 0 (the norm grows along the dogleg path), so c >= 0 up to rounding.  classify records c / (|a| |b|) of every
    interpolated step ("interp_c"): over all cases it lies between 0.010 and 0.22, and test_window_tr_cases_cpu.py asserts that it is
    positive.  The branch is dead for a solve.
  * a finite window whose first Cholesky fails, mu rises and the solve goes on.  Tried: windows of 2 and 3 keyframes whose only factors
    are the IMU edges -- the global translation and yaw are unobservable, every diagonal entry of H is >= 1e3 and its smallest eigenvalue is
    -4e-11 (zero to rounding).  Both witnesses factor S H S + mu D^2 at the first mu = 1e-8 and solve on to PARAMETER_TOLERANCE: after Jacobi
    scaling the diagonal is of order one, so mu D^2 lifts a zero pivot to ~1e-8, eight orders above the rounding of the factorisation.  Only a
    non-finite H fails the first factorisation, and then every retry fails: that is `failure`.  The retry loop also runs in the `breakdown`
    form of the GPU file, where the chain kernel reports a bad pivot at every step.

No GPU in here; the oracle is imported inside the functions that need it.  `PYTHONPATH=. python tests/window_tr_cases.py` rewrites
tests/golden/window_tr_spread.json, the spread between the two witnesses' iterates that the GPU file's prefix tolerances come from."""
import copy
import functools

import numpy as np

import np_ceres as nc
from glio_amd import ctypes_types as T
from glio_amd import synth

BASE = synth.SEED_BASE
PTS = 256
MARGIN = 1e-4                       # relative distance every decision of the loop keeps from its threshold
FAR_PERTURB = (8.0, 50.0, 2.0)
KINDS = ("gn", "cauchy", "interp", "lm")
OUTCOMES = ("accept_hi", "accept_mid", "accept_lo", "rejected", "invalid")      # ratio > 0.75, 0.25 .. 0.75, < 0.25
TERMINATIONS = dict(NO_CONVERGENCE=0, FUNCTION_TOL=1, PARAMETER_TOL=2, GRADIENT_TOL=3, MIN_RADIUS=4, FAILURE=5)

_W12 = dict(W=12, with_gnss=True, with_prior=False, seed=BASE + 321)
_W12_FAR = dict(W=12, with_gnss=True, with_prior=False, seed=BASE + 322, perturb=FAR_PERTURB)
_W5_FAR = dict(W=5, with_gnss=False, with_prior=False, seed=BASE + 302, perturb=FAR_PERTURB)


def _case(window, opts=None, far=None, use=None, corrupt=None, marg=False, pts=PTS, **expect):
    return dict(window=window, opts=opts or {}, far=far, use=dict(dict(use_gnss=True, use_prior=True, use_imu=True), **(use or {})), corrupt=corrupt, marg=marg,
                pts=pts, expect=expect)


CASES = {
    "small_radius": _case(_W12, dict(initial_trust_region_radius=0.01, max_iterations=30), kinds={"cauchy", "gn"}, outcomes={"accept_hi"}, termination=1),
    "radius_20": _case(_W12, dict(initial_trust_region_radius=20.0, max_iterations=30), kinds={"cauchy", "gn"}, outcomes={"accept_hi"}, termination=1),
    "far_w5": _case(_W5_FAR, dict(max_iterations=40), kinds={"interp", "gn", "cauchy"}, outcomes={"rejected", "accept_lo", "accept_hi"}),
    "far_w5_prior": _case(dict(_W5_FAR, with_prior=True), dict(max_iterations=40), kinds={"interp", "cauchy"}, outcomes={"rejected"}),
    "far_w12_prior": _case(dict(_W12_FAR, with_prior=True), dict(max_iterations=40), kinds={"interp"}, outcomes={"rejected"}),
    "mid_ratios": _case(_W12_FAR, dict(max_iterations=40), kinds={"gn"}, outcomes={"accept_mid"}),
    "forced_rejects": _case(_W12, dict(min_relative_decrease=1.05, max_iterations=30), far=(0.4, 5), kinds={"gn", "interp", "cauchy"}, outcomes={"rejected"}),
    "min_radius": _case(_W12, dict(min_relative_decrease=1.05, min_trust_region_radius=1.0, max_iterations=60), far=(0.4, 5), outcomes={"rejected"}, termination=4),
    "grad_tol_first": _case(_W12, dict(gradient_tolerance=1e3), termination=3),
    "grad_tol_late": _case(_W12, dict(gradient_tolerance=0.5, function_tolerance=0.0), termination=3),
    "param_tol": _case(_W12, dict(parameter_tolerance=1e-3, function_tolerance=0.0), termination=2),
    "failure": _case(_W12, corrupt=3, outcomes={"invalid"}, termination=5),
    # 24 iterations when left alone; capped at 18 (a quarter cut): from iteration 19 on the cost changes by a few 1e-3 per step, a difference of 1e-11 m
    # in the iterate moves the ratio by 1e-8, and Levenberg-Marquardt's radius is a smooth function of the ratio -- the two CPU witnesses then
    # differ by 1.6e-9 .. 1.1e-7 in the radius, more than the 1e-9 they are held to.  Up to iteration 18 they agree to 4.4e-11.
    "lm_accept": _case(_W12_FAR, dict(trust_region_strategy=1, max_iterations=18), kinds={"lm"}, outcomes={"accept_hi", "accept_mid"}, termination=0),
    "lm_reject": _case(_W12_FAR, dict(trust_region_strategy=1, max_iterations=30, initial_trust_region_radius=1e-2, min_relative_decrease=1.05), kinds={"lm"},
                       outcomes={"rejected"}, termination=2),
    "lm_min_radius": _case(_W12_FAR, dict(trust_region_strategy=1, max_iterations=60, min_relative_decrease=1.05, min_trust_region_radius=1e-6), kinds={"lm"},
                           outcomes={"rejected"}, termination=4),
    "lm_w1": _case(dict(W=1, with_gnss=False, with_prior=False, seed=BASE + 303, perturb=(0.3, 2.0, 0.0)),
                   dict(trust_region_strategy=1, max_iterations=12, initial_trust_region_radius=1e-3), use=dict(use_imu=False), pts=600, kinds={"lm"},
                   outcomes={"accept_hi"}, termination=0),
    # a prior with the structure the running estimator has (block diagonal by keyframe: the keyframe chain takes it), from a far start at a small radius
    "marg_prior": _case(dict(W=12, with_gnss=True, seed=BASE + 312), dict(initial_trust_region_radius=0.5, max_iterations=30), far=(0.4, 5), marg=True,
                        kinds={"cauchy", "gn"}, outcomes={"accept_hi"}, termination=1),
}


def far_state(st, sigma, seed):
    far = st.copy()
    far.trans = far.trans + np.random.default_rng(seed).normal(0, sigma, far.trans.shape)
    far.speed_bias = far.speed_bias + np.random.default_rng(seed + 1).normal(0, sigma / 2, far.speed_bias.shape)
    return far


@functools.lru_cache(maxsize=None)
def build(name):
    """(window, correspondences, start state, use flags) of a case; shared, not to be modified"""
    c = CASES[name]
    if c["marg"]:
        from oracle import pyoracle as po
        W = c["window"]["W"]
        stream = synth.make_window(pts_per_scan=c["pts"], **dict(c["window"], W=W + 1))
        first = synth.sub_window(stream, 0, W)
        p0 = po.Problem(first, synth.analytic_correspondences(first))
        s0, _ = p0.solve(first.init)
        win = synth.sub_window(stream, 1, W)
        win.prior = p0.marginalize(s0)
    else:
        win = synth.make_window(pts_per_scan=c["pts"], **c["window"])
    for k, v in c["opts"].items():
        assert hasattr(win.opts, k), k
        setattr(win.opts, k, v)
    corr = synth.analytic_correspondences(win)
    if c["corrupt"] is not None:
        win.preints[c["corrupt"]]["jacobian"][0, 9] = 1e200
    start = win.init.copy()
    if not c["use"]["use_gnss"]:
        start.n_ddt = 0
    if c["far"]:
        start = far_state(start, *c["far"])
    return win, corr, start, c["use"]


def with_max_iterations(win, k):
    w = copy.copy(win)
    w.opts = T.GlioOpts.from_buffer_copy(win.opts)
    w.opts.max_iterations = k
    return w


# ------------------------------------------------------------------ the numpy witness: callbacks of np_ceres.minimize for a window problem
def quat_plus(q, d):
    n = np.linalg.norm(d)
    if n == 0.0:
        return q.copy()
    dq = np.r_[np.cos(n), np.sin(n) / n * d]
    w1, v1, w2, v2 = dq[0], dq[1:], q[0], q[1:]
    return np.r_[w1 * w2 - v1 @ v2, w1 * v2 + w2 * v1 + np.cross(v1, v2)]


def window_callbacks(prob):
    W = prob.win.W

    def plus(x, d):
        y = x.copy()
        for s in range(W):
            y.trans[s] = x.trans[s] + d[15 * s:15 * s + 3]
            y.quat[s] = quat_plus(x.quat[s], d[15 * s + 3:15 * s + 6])
            y.speed_bias[s] = x.speed_bias[s] + d[15 * s + 6:15 * s + 15]
        if x.n_ddt:
            y.rcv_ddt[:x.n_ddt] = x.rcv_ddt[:x.n_ddt] + d[15 * W:]
        return y

    def flat(x):
        return np.concatenate([x.trans.ravel(), x.quat.ravel(), x.speed_bias.ravel(), x.rcv_ddt[:x.n_ddt]])

    def evaluate(x):
        H, g, c = prob.linearize(x)          # the oracle does not treat non-finite values as an evaluation failure either
        return c, H, g

    return evaluate, plus, flat


def np_opts_from(o, **kw):
    return nc.Options(max_iterations=o.max_iterations, strategy="lm" if o.trust_region_strategy == 1 else "dogleg", dogleg="traditional",
                      jacobi_scaling=bool(o.jacobi_scaling), initial_radius=o.initial_trust_region_radius, max_radius=o.max_trust_region_radius,
                      min_radius=o.min_trust_region_radius, min_relative_decrease=o.min_relative_decrease, function_tolerance=o.function_tolerance,
                      gradient_tolerance=o.gradient_tolerance, parameter_tolerance=o.parameter_tolerance, **kw)


def _recording_strategies(log):
    """subclasses of np_ceres' two strategies that note, per call of compute(), what the loop is about to decide on"""

    class Dogleg(nc.Dogleg):
        def compute(self, Hs, gs):
            rec = dict(radius_before=self.radius, kind=None, outcome=None, ratio=None)
            log.append(rec)
            step = super().compute(Hs, gs)
            if step is not None:
                gn, cauchy, r = float(np.linalg.norm(self.gn)), float(np.linalg.norm(self.grad) * self.alpha), self.radius
                rec.update(kind="gn" if gn <= r else "cauchy" if cauchy >= r else "interp", gn_norm=gn, cauchy_norm=cauchy, mu=self.mu)
                if rec["kind"] == "interp":
                    a, b = -self.alpha * self.grad, self.gn
                    rec["interp_c"] = float((a @ b - a @ a) / (np.linalg.norm(a) * np.linalg.norm(b)))
            return step

        def accepted(self, q):
            log[-1].update(outcome="accept_hi" if q > 0.75 else "accept_lo" if q < 0.25 else "accept_mid", ratio=float(q))
            super().accepted(q)

        def rejected(self):
            log[-1]["outcome"] = "rejected"
            super().rejected()

        def invalid(self):
            log[-1]["outcome"] = "invalid"
            super().invalid()

    class LevenbergMarquardt(nc.LevenbergMarquardt):
        def compute(self, Hs, gs):
            rec = dict(radius_before=self.radius, kind=None, outcome=None, ratio=None, decrease=self.decrease)
            log.append(rec)
            step = super().compute(Hs, gs)
            if step is not None:
                rec["kind"] = "lm"
            return step

        def accepted(self, q):
            log[-1].update(outcome="accept_hi" if q > 0.75 else "accept_lo" if q < 0.25 else "accept_mid", ratio=float(q))
            super().accepted(q)

        def rejected(self):
            log[-1]["outcome"] = "rejected" if log[-1]["kind"] else "invalid"
            super().rejected()

        invalid = rejected

    return Dogleg, LevenbergMarquardt


def np_witness(prob, start, opts):
    """np_ceres.minimize on a window problem with the recording strategies: (state, summary dict, history rows, per-iteration records)"""
    evaluate, plus, flat = window_callbacks(prob)
    log, trace = [], []
    saved = nc.Dogleg, nc.LevenbergMarquardt
    nc.Dogleg, nc.LevenbergMarquardt = _recording_strategies(log)
    try:
        with np.errstate(all="ignore"):
            x, info, hist = nc.minimize(start.copy(), evaluate, plus, flat, np_opts_from(opts), trace=trace)
    finally:
        nc.Dogleg, nc.LevenbergMarquardt = saved
    assert len(log) == info["iterations"]
    o = np_opts_from(opts)
    c0, _, g0 = evaluate(start)
    cost, xflat, gmax = c0, flat(start), float(np.abs(flat(start) - flat(plus(start, -g0))).max())
    hist = [tuple(h) for h in hist]
    rows = iter(trace)
    for k, rec in enumerate(log):
        rec.update(cost_before=cost, gradient_before=gmax, x_norm=float(np.linalg.norm(xflat)))
        if rec["kind"] is None:                       # the factorisation failed (or the model did not decrease): no candidate
            rec["outcome"] = "invalid"
        elif k < len(hist):
            rec.update(candidate_cost=hist[k][0], step_norm=hist[k][2])
        if rec["outcome"] in ("accept_hi", "accept_mid", "accept_lo", "rejected") and rec["kind"] is not None:
            row = next(rows)
            rec["ratio"] = float(row["ratio"])
            if rec["outcome"] != "rejected":
                cost, xflat, gmax = row["cost"], row["x"], row["gradient"]
        elif rec["outcome"] is None:
            rec["outcome"] = "end"                    # a tolerance test ended the solve with this candidate evaluated, not taken
        rec["x_after"] = np.array(xflat, float)
        rec["radius_after"] = log[k + 1]["radius_before"] if k + 1 < len(log) else info["final_radius"]
    info["gradient_max_norm"] = gmax
    return x, info, np.array(hist).reshape(-1, 3), log


def flat_state(s):
    return np.concatenate([s.trans.ravel(), s.quat.ravel(), s.speed_bias.ravel(), s.rcv_ddt[:s.n_ddt]])


def state_parts(W, v):
    """translations, quaternions, speed-bias and clock drifts of a flat state"""
    return dict(trans=v[:3 * W], quat=v[3 * W:7 * W], speed_bias=v[7 * W:16 * W], ddt=v[16 * W:])


@functools.lru_cache(maxsize=None)
def oracle_prefixes(name):
    """[(state, summary)] of the oracle's solve with max_iterations = 0 .. n, n the iteration count of the case's own solve (the last entry is that
    solve).  The oracle keeps no history of its iterates; capping the run makes each observable, on the device as well."""
    from oracle import pyoracle as po
    win, corr, start, use = build(name)
    full = po.Problem(win, corr, **use).solve(start)
    out = []
    for k in range(full[1].iterations):
        out.append(po.Problem(with_max_iterations(win, k), corr, **use).solve(start))
    out.append(full)
    for s, _ in out:
        for a in (s.trans, s.quat, s.speed_bias, s.rcv_ddt):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def classify(name):
    """dict(summary=oracle's GlioSummary, np_summary=..., hist=oracle's history rows, np_hist=..., iterations=[records], oracle=[(state, summary)] prefixes).
    Each record: kind, ratio, outcome, radius_before, radius_after, x_after (numpy witness), the compared quantities."""
    from oracle import pyoracle as po
    win, corr, start, use = build(name)
    prob = po.Problem(win, corr, **use)
    sol, summ, hist = prob.solve_history(start)
    x, info, nhist, log = np_witness(prob, start, win.opts)
    return dict(summary=summ, solution=sol, hist=hist, np_solution=x, np_summary=info, np_hist=nhist, iterations=log, strategy=int(win.opts.trust_region_strategy))


def labels(name):
    c = classify(name)
    its = c["iterations"]
    return dict(kinds={r["kind"] for r in its if r["kind"]}, outcomes={r["outcome"] for r in its if r["outcome"] != "end"},
                termination=int(c["summary"].termination), strategy=c["strategy"])


def margins(name):
    """[(iteration, what, value, threshold)] for every comparison the loop decides on: |value - threshold| must exceed MARGIN * max(|value|, |threshold|)"""
    win, _, _, _ = build(name)
    o = win.opts
    out = []
    its = classify(name)["iterations"]
    for k, r in enumerate(its):
        out.append((k, "gradient_tolerance", r["gradient_before"], o.gradient_tolerance))
        out.append((k, "min_radius", r["radius_before"], o.min_trust_region_radius))
        if r["kind"] in ("gn", "cauchy", "interp"):
            out.append((k, "gn_norm vs radius", r["gn_norm"], r["radius_before"]))
            if r["gn_norm"] > r["radius_before"]:
                out.append((k, "cauchy_norm vs radius", r["cauchy_norm"], r["radius_before"]))
        if "candidate_cost" in r and r["kind"]:
            out.append((k, "parameter_tolerance", r["step_norm"], o.parameter_tolerance * (r["x_norm"] + o.parameter_tolerance)))
            if r["outcome"] != "end" or classify(name)["summary"].termination == TERMINATIONS["FUNCTION_TOL"]:
                out.append((k, "function_tolerance", abs(r["cost_before"] - r["candidate_cost"]), o.function_tolerance * r["cost_before"]))
        if r["ratio"] is not None:
            out.append((k, "min_relative_decrease", r["ratio"], o.min_relative_decrease))
            if r["kind"] != "lm" and r["outcome"] != "rejected":          # Levenberg-Marquardt's radius is a continuous function of the ratio
                out.append((k, "ratio vs 0.25", r["ratio"], 0.25))
                out.append((k, "ratio vs 0.75", r["ratio"], 0.75))
    last = its[-1] if its else None
    if last is not None:                                                   # the tests the loop makes before an iteration that did not start
        out.append((len(its), "min_radius", last["radius_after"], o.min_trust_region_radius))
        out.append((len(its), "gradient_tolerance", classify(name)["np_summary"]["gradient_max_norm"], o.gradient_tolerance))
    return out


def spread(name):
    """S_k, k = 0 .. n: max |x_oracle,k - x_np,k| per part of the state after k iterations, between the two CPU witnesses"""
    win, _, start, _ = build(name)
    pre = oracle_prefixes(name)
    its = classify(name)["iterations"]
    assert len(pre) == len(its) + 1, (name, len(pre), len(its))
    xs = [flat_state(start)] + [r["x_after"] for r in its]
    rows = []
    for (so, _), xn in zip(pre, xs):
        a, b = state_parts(win.W, flat_state(so)), state_parts(win.W, xn)
        rows.append({p: float(np.abs(a[p] - b[p]).max()) if len(a[p]) else 0.0 for p in a})
    return rows


def exact_radius_prefix(name):
    """The largest K such that the radius after k <= K iterations is the initial radius times exact factors only (powers of two, and 3 x radius
    for an accepted step on the boundary, whose norm IS the radius): every implementation must then return the same bits.  A Gauss-Newton
    step accepted with ratio > 0.75 keeps the radius when 3 |step| is below it (required here with the margin); an interpolated step's norm
    and Levenberg-Marquardt's accepted steps are rounded quantities."""
    K = 0
    for r in classify(name)["iterations"]:
        if r["outcome"] in ("rejected", "invalid", "end"):
            exact = True
        elif r["kind"] == "lm":
            exact = False
        elif r["outcome"] in ("accept_mid", "accept_lo") or r["kind"] == "cauchy":
            exact = True
        else:
            exact = r["kind"] == "gn" and 3.0 * r["gn_norm"] < (1.0 - MARGIN) * r["radius_before"]
        if not exact:
            break
        K += 1
    return K


# ------------------------------------------------------------------ device (or any third solver) against the oracle
STATE_GATES = dict(trans=1e-9, quat=1e-10, speed_bias=1e-6, ddt=1e-6)      # tests/test_hip_solver_limits.py (poses), tests/test_hip_solve_ends.py (the rest)
SUMMARY_GATES = dict(initial_cost=1e-9, final_cost=1e-9, final_radius=1e-9, gradient_max_norm=1e-6)


def compare_with_oracle(s, m, so, mo, state_tol=None, exact_radius=False, label=""):
    """A solve (state s, summary m) against the oracle's (so, mo): the integer fields equal, the real ones to SUMMARY_GATES (relative), the state to
    `state_tol` per part (default STATE_GATES).  Returns every figure as a ratio to its tolerance; prints them first."""
    from parity_checks import assert_pose_parity
    tol = dict(STATE_GATES, **(state_tol or {}))
    ratios = {}
    for k, gate in SUMMARY_GATES.items():
        a, b = getattr(m, k), getattr(mo, k)
        ratios[k] = 0.0 if a == b else abs(a - b) / max(abs(b), 1e-300) / gate
    W = so.W
    a, b = state_parts(W, flat_state(s)), state_parts(W, flat_state(so))
    for p in a:
        ratios[p] = float(np.abs(a[p] - b[p]).max()) / tol[p] if len(a[p]) else 0.0
    print(f"{label}: iterations {m.iterations}/{mo.iterations} successful {m.successful_steps}/{mo.successful_steps} termination {m.termination}/{mo.termination} "
          f"radius {m.final_radius!r}/{mo.final_radius!r}; figure / tolerance: " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    assert (m.iterations, m.successful_steps, m.termination) == (mo.iterations, mo.successful_steps, mo.termination), (label, m.as_dict(), mo.as_dict())
    if exact_radius:
        assert m.final_radius == mo.final_radius, (label, m.final_radius, mo.final_radius)
    for k, v in ratios.items():
        assert v <= 1.0, (label, k, v, m.as_dict(), mo.as_dict())
    assert_pose_parity(s, so)
    return ratios


GOLDEN = "window_tr_spread.json"


def prefix_tolerances(name, golden):
    """per k: the final-state gate or 100 x S_k of the golden file (two decimal digits over the spread between the CPU witnesses), whichever is larger"""
    g = golden[name]
    n = len(g["trans"])
    return [{p: max(STATE_GATES[p], 100.0 * g[p][k]) for p in STATE_GATES} for k in range(n)]


def load_golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as f:
        return json.load(f)


def write_golden(path):
    import json
    doc = {name: {p: [row[p] for row in spread(name)] for p in ("trans", "quat", "speed_bias", "ddt")} for name in CASES}
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    import os
    write_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN))

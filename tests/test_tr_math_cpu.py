"""glio_amd/csrc/tr_math.h -- the one definition of Ceres 1.14's scalar trust-region rule that the window, batch, trajectory and pose-graph kernels call --
compiled by a plain host compiler (glio_amd/host/host_tr_math_test.cpp, no HIP header) and compared EXACTLY (== on the doubles, NaN matching NaN) with the
same formulas restated here in Python floats and, where tests/np_ceres.py has them as scalar formulas, with np_ceres.  The program is built like the other
host_*_test.cpp programs plus -ffp-contract=off, so every operation rounds once, as Python's do.  A second test reads the sources: the three kernel files
include the header and call it, and the formulas are written out nowhere else under glio_amd/csrc."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ceres as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glio_amd", "csrc")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def call(tmp_path_factory):
    """call(lines) -> one list of floats per line, all in one run of the program"""
    exe = str(tmp_path_factory.mktemp("trmath") / "host_tr_math_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-ffp-contract=off", os.path.join(ROOT, "glio_amd", "host", "host_tr_math_test.cpp"), "-o", exe])

    def run(lines):
        text = "".join(name + " " + " ".join(float(v).hex() for v in args) + "\n" for name, *args in lines)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[float.fromhex(t) if "x" in t else float(t) for t in ln.split()] for ln in out]
    return run


def same(got, want):
    """bit equality, NaN = NaN (0.0 and -0.0 differ)"""
    got, want = list(got), list(want)
    return len(got) == len(want) and all((math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1.0, g) == math.copysign(1.0, w)) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------- the restatement (C's fmax / fmin: a NaN loses)
def fmax(a, b):
    return b if math.isnan(a) else (a if math.isnan(b) else max(a, b))


def fmin(a, b):
    return b if math.isnan(a) else (a if math.isnan(b) else min(a, b))


def r_dogleg(lm, gg, nn, gd, gnorm, gnn, radius, alpha):
    if lm or gnn <= radius:
        return 0.0, 1.0, gnn
    if gnorm * alpha >= radius:
        return -(radius / gnorm), 0.0, radius
    b_dot_a = -alpha * gd
    a_sq = alpha * alpha * gg
    b_minus_a_sq = nn - 2 * b_dot_a + a_sq
    c = b_dot_a - a_sq
    d = math.sqrt(c * c + b_minus_a_sq * (radius * radius - a_sq))
    beta = (d - c) / b_minus_a_sq if c <= 0 else (radius * radius - a_sq) / (d + c)
    return -alpha * (1.0 - beta), beta, -1.0


def r_step(*args):
    ca, cb, grad, gn, diag, scale, g, t, y, mu = (np.float64(v) for v in args)          # (numpy's doubles: a division by zero gives the infinity C gives)
    with np.errstate(all="ignore"):
        sv = ca * grad + cb * gn
        step_s = sv / diag
        gs = scale * g
        hs_step = ca * (scale * t) - cb * (gs - mu * diag * diag * y)
        return [float(v) for v in (sv, step_s, scale * step_s, gs * step_s, step_s * hs_step)]


def r_accept(q, step_norm, radius, mu):
    if q < 0.25:
        radius *= 0.5
    if q > 0.75:
        radius = fmax(radius, 3.0 * step_norm)
    return radius, fmax(1e-8, 2.0 * mu / 10.0)


def r_lm_accept(gain, radius, max_radius, cube):
    return fmin(max_radius, radius / fmax(1.0 / 3.0, 1.0 - cube(2.0 * gain - 1.0)))


def r_gate(it, max_it, out_of_time, gmax, gtol, radius, min_radius):
    if it >= max_it or out_of_time:
        return nc.NO_CONVERGENCE
    if gmax <= gtol:
        return nc.GRADIENT_TOL
    if radius <= min_radius:
        return nc.MIN_RADIUS
    return -1


def from_vectors(grad, gn, alpha):
    """the scalars the kernels hand over: the sums and their roots"""
    grad, gn = np.asarray(grad, float), np.asarray(gn, float)
    gg, nn, gd = float(grad @ grad), float(gn @ gn), float(grad @ gn)
    return gg, nn, gd, math.sqrt(gg), math.sqrt(nn), alpha


# ---------------------------------------------------------------------------------------------------------------- dogleg
# Cauchy point a = -alpha grad = (1, 0); Gauss-Newton points b with a . (b - a) <= 0 and > 0 (the two branches of beta)
DOGLEG_CASES = {
    "gauss_newton_inside": (from_vectors([-1.0, 0.0], [0.5, 2.0], 1.0), 2.5),
    "gauss_newton_on_the_boundary": (from_vectors([-1.0, 0.0], [0.0, 2.0], 1.0), 2.0),
    "cauchy_outside": (from_vectors([-1.0, 0.0], [0.5, 2.0], 1.0), 0.75),
    "cauchy_on_the_boundary": (from_vectors([-1.0, 0.0], [0.5, 2.0], 1.0), 1.0),
    "interpolation_c_negative": (from_vectors([-1.0, 0.0], [0.5, 2.0], 1.0), 1.5),
    "interpolation_c_zero": (from_vectors([-1.0, 0.0], [1.0, 2.0], 1.0), 1.5),
    "interpolation_c_positive": (from_vectors([-1.0, 0.0], [2.0, 1.0], 1.0), 1.5),
    "interpolation_odd_numbers": (from_vectors([-0.3, 0.7, 0.11], [1.9, -2.3, 0.4], 0.37), 1.234),
}


@pytest.mark.parametrize("name", sorted(DOGLEG_CASES))
def test_dogleg_coefficients(call, name):
    (gg, nn, gd, gnorm, gnn, alpha), radius = DOGLEG_CASES[name]
    want = r_dogleg(False, gg, nn, gd, gnorm, gnn, radius, alpha)
    got, got_lm = call([("dogleg", 0.0, gg, nn, gd, gnorm, gnn, radius, alpha), ("dogleg", 1.0, gg, nn, gd, gnorm, gnn, radius, alpha)])
    assert same(got, want), (got, want)
    assert same(got_lm, (0.0, 1.0, gnn))                       # Levenberg-Marquardt: the damped step itself, whatever the radius
    # the trajectory's form: the squares of the rounded roots stand for the sums (the sums handed over are not read)
    got_roots, = call([("dogleg_roots", gd, gnorm, gnn, radius, alpha)])
    assert same(got_roots, r_dogleg(False, gnorm * gnorm, gnn * gnn, gd, gnorm, gnn, radius, alpha)), (got_roots, name)
    branch = {"gauss": (0.0, 1.0), "cauchy": (None, 0.0)}.get(name.split("_")[0])
    if branch:
        assert got[1] == branch[1] and got[2] == (gnn if name.startswith("gauss") else radius)
    else:
        c = -alpha * gd - alpha * alpha * gg
        assert got[2] == -1.0 and 0.0 < got[1] < 1.0 and {"negative": c < 0, "zero": c == 0, "positive": c > 0, "numbers": True}[name.split("_")[-1]]


# the hand-made problem of tests/test_dogleg_hand_kat.py: unit diagonal, so Jacobi scale 1/2 and D = 1/2 cancel: grad = g, gn = p_gn, alpha = 17/26
HAND_H = np.array([[1.0, 0.6, 0.0], [0.6, 1.0, 0.0], [0.0, 0.0, 1.0]])
HAND_G = np.array([-2.0, -1.2, 0.0])
HAND_GN = np.array([2.0, 0.0, 0.0])
HAND_PC = np.array([17.0 / 13.0, 51.0 / 65.0, 0.0])


def hand_step(radius):
    if radius >= 2.0:
        return HAND_GN.copy()
    if radius <= np.linalg.norm(HAND_PC):
        return np.array([2.0, 1.2, 0.0]) / np.sqrt(5.44) * radius
    d = HAND_GN - HAND_PC
    pd, dd = HAND_PC @ d, d @ d
    return HAND_PC + (-pd + np.sqrt(pd * pd + dd * (radius * radius - HAND_PC @ HAND_PC))) / dd * d


@pytest.mark.parametrize("radius", [1.0, 1.8, 3.0])
def test_dogleg_takes_the_hand_steps(call, radius):
    alpha = float(HAND_G @ HAND_G / (HAND_G @ HAND_H @ HAND_G))
    gg, nn, gd, gnorm, gnn, _ = from_vectors(HAND_G, HAND_GN, alpha)
    (ca, cb, snorm), = call([("dogleg", 0.0, gg, nn, gd, gnorm, gnn, radius, alpha)])
    assert same((ca, cb, snorm), r_dogleg(False, gg, nn, gd, gnorm, gnn, radius, alpha))
    step = ca * HAND_G + cb * HAND_GN
    assert np.abs(step - hand_step(radius)).max() < 1e-14
    assert {1.0: (cb == 0.0 and snorm == radius), 1.8: (snorm == -1.0 and abs(np.linalg.norm(step) - 1.8) < 1e-14), 3.0: ((ca, cb, snorm) == (0.0, 1.0, 2.0))}[radius]
    # and np_ceres' vector form of the same rule takes the same step (np.linalg.norm against the root of the sum: a rounding apart at the most)
    d = nc.Dogleg(nc.Options(initial_radius=radius))
    d.grad, d.gn, d.alpha = HAND_G, HAND_GN, alpha
    assert np.abs(d._traditional_step() - step).max() < 1e-14


def test_step_element(call):
    rng = np.random.RandomState(7)
    rows = [tuple(rng.uniform(-3, 3, 10)) for _ in range(6)] + [(0.0, 1.0, 0.3, -0.2, 0.5, 0.5, 1.5, 0.7, 0.4, 1e-8), (-0.8, 0.0, 0.3, -0.2, 1e-3, 0.25, 1.5, 0.7, 0.4, 1.0),
                                                                (0.5, 0.5, NAN, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0), (0.5, 0.5, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0)]
    for got, row in zip(call([("step",) + r for r in rows]), rows):
        assert same(got, r_step(*row)), row


# ---------------------------------------------------------------------------------------------------------------- the candidate's verdict
def test_convergence_tests_and_quality(call):
    up, dn = lambda v: math.nextafter(v, INF), lambda v: math.nextafter(v, -INF)
    ptol, ftol, xn, cost = 1e-8, 1e-6, 3.7, 12.5
    edge_p, edge_f = ptol * (xn + ptol), ftol * cost
    lines = [("pconv", edge_p, xn, ptol), ("pconv", up(edge_p), xn, ptol), ("pconv", 0.0, 0.0, ptol), ("pconv", NAN, xn, ptol),
             ("fconv", cost, cost - edge_f, ftol), ("fconv", cost, cost + edge_f, ftol), ("fconv", cost, cost - 2 * edge_f, ftol), ("fconv", cost, NAN, ftol), ("fconv", 0.0, 0.0, ftol),
             ("quality", 5.0, 3.0, 4.0), ("quality", 5.0, 7.0, 4.0), ("quality", 5.0, INF, 4.0), ("quality", 5.0, NAN, 4.0), ("quality", 1.0, 0.1, 0.3)]
    got = [g[0] for g in call(lines)]
    want = [1.0, 0.0, 1.0, 0.0,
            float(abs(cost - (cost - edge_f)) <= edge_f), float(abs(cost - (cost + edge_f)) <= edge_f), 0.0, 0.0, 1.0,
            0.5, -0.5, -INF, NAN, (1.0 - 0.1) / 0.3]
    assert same(got, want), (got, want)


def test_accept_rule_at_its_boundaries(call):
    up, dn = lambda v: math.nextafter(v, INF), lambda v: math.nextafter(v, -INF)
    radius, step_norm, mu = 2.0, 5.0, 1e-3
    qs = [0.25, dn(0.25), up(0.25), 0.75, dn(0.75), up(0.75), 1e-3, 1.0, 0.5, NAN, -INF]
    got = call([("accept", q, step_norm, radius, mu) for q in qs])
    for q, g in zip(qs, got):
        assert same(g, r_accept(q, step_norm, radius, mu)), q
    by_q = dict(zip(qs[:9], (g[0] for g in got)))
    assert by_q[0.25] == radius and by_q[0.75] == radius                              # exactly on the thresholds: no shrink, no growth
    assert by_q[dn(0.25)] == 1.0 and by_q[up(0.25)] == radius and by_q[dn(0.75)] == radius and by_q[up(0.75)] == 15.0
    assert by_q[1e-3] == 1.0 and by_q[1.0] == 15.0 and by_q[0.5] == radius
    # growth never shrinks: max(radius, 3 |step|)
    assert call([("accept", 1.0, 0.1, radius, mu)])[0][0] == radius
    # np_ceres' DoglegStrategy::StepAccepted says the same on finite numbers
    for q, g in zip(qs[:9], got):
        d = nc.Dogleg(nc.Options(initial_radius=radius))
        d.mu, d.step_norm = mu, step_norm
        d.accepted(q)
        assert same(g, (d.radius, d.mu)), q
    # the acceptance itself: quality > min_relative_decrease, so the threshold and a NaN are rejected
    acc = [g[0] for g in call([("accepted", 1e-3, 1e-3), ("accepted", up(1e-3), 1e-3), ("accepted", NAN, 1e-3), ("accepted", -INF, 1e-3), ("accepted", INF, 1e-3)])]
    assert acc == [0.0, 1.0, 0.0, 0.0, 1.0]
    assert [g[0] for g in call([("reject", radius), ("reject", 1e-32)])] == [radius * 0.5, 1e-32 * 0.5]


def test_mu_at_its_floor(call):
    mus = [1e-8, 5e-8, 4.9e-8, 1e-7, 1e-3, 1.0, 10.0, 0.0, NAN]
    got = [g[1] for g in call([("accept", 0.5, 1.0, 1.0, m) for m in mus])]
    assert same(got, [fmax(1e-8, 2.0 * m / 10.0) for m in mus])
    assert got[0] == 1e-8 and got[2] == 1e-8 and got[3] == 2.0 * 1e-7 / 10.0 and got[5] == 0.2 and got[7] == 1e-8 and got[8] == 1e-8


@pytest.mark.parametrize("variant", ["pow", "mul"])
def test_levenberg_marquardt_rule(call, variant):
    cube = (lambda c: c ** 3) if variant == "pow" else (lambda c: c * c * c)
    gains = [0.5, 1.0, 0.9, 0.95, 1e-3, 0.25, 0.75, 2.0, 0.3123, -0.5, INF]
    rows = [(g, 10.0, 1e16) for g in gains] + [(1.0, 1e16, 1e16), (1.0, 5e15, 1e16), (0.5, 2e16, 1e16)]
    got = [g[0] for g in call([("lm_accept_" + variant,) + r for r in rows])]
    assert same(got, [r_lm_accept(g, r, m, cube) for g, r, m in rows]), got
    assert got[0] == 10.0                                            # gain 0.5: the radius stays
    assert got[1] == got[3] == got[7] == got[10] == 10.0 / (1.0 / 3.0) == 30.0       # the 1/3 cap, from (2 gain - 1)^3 >= 2/3 on: the radius at most triples
    assert 10.0 < got[2] < 30.0 and got[4] < 10.0 and got[9] < 10.0                  # gain 0.9 is still below the cap; a poor gain shrinks
    assert got[11] == 1e16 and got[12] == 1e16 and got[13] == 1e16                                               # the max_radius cap
    if variant == "pow":                                             # np_ceres' LevenbergMarquardtStrategy::StepAccepted spells the cube as a power
        for (g, r, m), v in zip(rows[:10] + rows[11:], got[:10] + got[11:]):
            lm = nc.LevenbergMarquardt(nc.Options(initial_radius=r, max_radius=m))
            lm.accepted(g)
            assert lm.radius == v and lm.decrease == 2.0
    # StepRejected: radius / factor, the factor doubles
    assert call([("lm_reject", 10.0, 2.0), ("lm_reject", 5.0, 4.0), ("lm_reject", 1e-32, 8.0)]) == [[5.0, 4.0], [1.25, 8.0], [1e-32 / 8.0, 16.0]]
    lm = nc.LevenbergMarquardt(nc.Options(initial_radius=10.0))
    lm.rejected(); lm.rejected()
    assert (lm.radius, lm.decrease) == (1.25, 8.0)


def test_iteration_gate_order(call):
    # it, max_iterations, out_of_time, gradient max norm, gradient tolerance, radius, min radius
    rows = [(3, 15, 0, 1.0, 1e-10, 1.0, 1e-32),            # nothing holds
            (15, 15, 0, 1e-11, 1e-10, 1e-33, 1e-32),       # all three: max_iterations first
            (3, 15, 0, 1e-11, 1e-10, 1e-33, 1e-32),        # gradient and radius: the gradient first
            (3, 15, 0, 1.0, 1e-10, 1e-33, 1e-32),          # the radius alone
            (3, 15, 1, 1e-11, 1e-10, 1.0, 1e-32),          # out of time and the gradient: no convergence
            (16, 15, 0, 1.0, 1e-10, 1.0, 1e-32), (14, 15, 0, 1.0, 1e-10, 1.0, 1e-32), (0, 0, 0, 1.0, 1e-10, 1.0, 1e-32),
            (3, 15, 0, 1e-10, 1e-10, 1.0, 1e-32), (3, 15, 0, 1.0, 1e-10, 1e-32, 1e-32),          # both tests are "<="
            (3, 15, 0, NAN, 1e-10, 1.0, 1e-32), (3, 15, 0, 1.0, 1e-10, NAN, 1e-32)]              # a NaN passes
    got = [int(g[0]) for g in call([("gate",) + r for r in rows])]
    assert got == [r_gate(*r) for r in rows]
    assert got == [-1, nc.NO_CONVERGENCE, nc.GRADIENT_TOL, nc.MIN_RADIUS, nc.NO_CONVERGENCE, nc.NO_CONVERGENCE, -1, nc.NO_CONVERGENCE, nc.GRADIENT_TOL, nc.MIN_RADIUS, -1, -1]


def test_five_invalid_steps(call):
    assert [g[0] for g in call([("invalid", k) for k in (1, 2, 3, 4, 5, 6, 0)])] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0]          # four go on, the fifth ends the solve


def test_scale_and_clip(call):
    up, dn = lambda v: math.nextafter(v, INF), lambda v: math.nextafter(v, -INF)
    hs = [0.0, 1.0, 4.0, 2.0, 1e-300, 1e300, INF, NAN, -1.0]
    got = [g[0] for g in call([("scale", h) for h in hs])]
    assert same(got, [1.0 / (1.0 + (math.sqrt(h) if h >= 0 else NAN)) for h in hs]) and got[:3] == [1.0, 0.5, 1.0 / 3.0]
    ds = [1e-6, dn(1e-6), up(1e-6), 1e32, dn(1e32), up(1e32), 0.0, -5.0, 1.0, INF, -INF, NAN]
    tern = [g[0] for g in call([("clip", d) for d in ds])]
    mm = [g[0] for g in call([("clip_minmax", d) for d in ds])]
    assert same(tern, [1e-6 if d < 1e-6 else (1e32 if d > 1e32 else d) for d in ds])
    assert same(mm, [fmin(fmax(d, 1e-6), 1e32) for d in ds])
    assert same(tern[:-1], mm[:-1]) and same(tern[:-1], [1e-6, 1e-6, up(1e-6), 1e32, dn(1e32), 1e32, 1e-6, 1e-6, 1.0, 1e32, 1e-6])
    assert math.isnan(tern[-1]) and mm[-1] == 1e-6                   # the one difference: the ternary lets a NaN through, min/max makes it the lower bound
    # the same clip with a caller's own bounds (the pose graph's options)
    own = [g[0] for g in call([("clip", d, 0.5, 8.0) for d in (0.5, 0.4, 8.0, 9.0, 3.0, NAN)])]
    assert same(own, [0.5, 0.5, 8.0, 8.0, 3.0, NAN])
    assert same(tern, [float(np.clip(d, 1e-6, 1e32)) for d in ds])   # np_ceres clips with np.clip, which keeps a NaN too


# ---------------------------------------------------------------------------------------------------------------- constants
CONSTANTS = dict(initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, function_tolerance=1e-6, gradient_tolerance=1e-10,
                 parameter_tolerance=1e-8, min_mu=1e-8, max_mu=1.0, mu_increase=10.0, mu_decrease_num=2.0, mu_decrease_den=10.0, shrink_below=0.25, shrink=0.5,
                 grow_above=0.75, grow=3.0, min_diagonal=1e-6, max_diagonal=1e32, lm_decrease_factor=2.0, lm_decrease_growth=2.0, max_invalid_steps=5.0, go_on=-1.0,
                 no_convergence=0.0, function_tol=1.0, parameter_tol=2.0, gradient_tol=3.0, min_radius_reached=4.0, failure=5.0)


def test_named_constants(call):
    got, = call([("consts",)])
    assert got == list(CONSTANTS.values())
    o = nc.Options()                                                  # the restatement's defaults are the same numbers
    assert (o.initial_radius, o.max_radius, o.min_radius, o.min_relative_decrease, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == tuple(got[:7])
    assert [nc.NO_CONVERGENCE, nc.FUNCTION_TOL, nc.PARAMETER_TOL, nc.GRADIENT_TOL, nc.MIN_RADIUS, nc.FAILURE] == got[22:]


def test_the_library_defaults_are_the_named_constants(call):
    """glio_opts_default and the pose graph's LM defaults, read back through the ctypes mirrors"""
    from glio_amd import build, capi
    from glio_amd import ctypes_types as T
    build.build()
    lib = capi.load()
    c = dict(zip(CONSTANTS, call([("consts",)])[0]))
    o = T.GlioOpts()
    lib.glio_opts_default.restype = None
    lib.glio_opts_default(C.byref(o))
    assert (o.initial_trust_region_radius, o.max_trust_region_radius, o.min_trust_region_radius, o.min_relative_decrease, o.function_tolerance, o.gradient_tolerance,
            o.parameter_tolerance) == (c["initial_radius"], c["max_radius"], c["min_radius"], c["min_relative_decrease"], c["function_tolerance"], c["gradient_tolerance"],
                                       c["parameter_tolerance"])
    lm = T.GlioPgraphLmOpts()
    lib.glio_pgraph_lm_opts_default.restype = None
    lib.glio_pgraph_lm_opts_default(C.byref(lm))
    assert (lm.initial_radius, lm.max_radius, lm.min_radius, lm.min_relative_decrease, lm.min_diagonal, lm.max_diagonal) == (
        c["initial_radius"], c["max_radius"], c["min_radius"], c["min_relative_decrease"], c["min_diagonal"], c["max_diagonal"])
    b = T.batch_tr_opts()                                             # the Python mirror of the batch options states the same defaults
    assert (b.initial_trust_region_radius, b.max_trust_region_radius, b.min_trust_region_radius, b.min_relative_decrease, b.function_tolerance, b.gradient_tolerance,
            b.parameter_tolerance) == tuple(call([("consts",)])[0][:7])


# ---------------------------------------------------------------------------------------------------------------- the sources
def _code(path):
    """a source file without its // comments"""
    return re.sub(r"//[^\n]*", "", open(path).read())


def test_the_rule_has_one_definition():
    """the three kernel files (and the pose graph) include tr_math.h and call it; the interpolation formula (b_dot_a) and the 0.75 / 3.0 radius rule are written
    out in tr_math.h and nowhere else under glio_amd/csrc; the checkers do not know the header"""
    hdr = _code(os.path.join(CSRC, "tr_math.h"))
    assert "b_dot_a" in hdr and re.search(r"TR_GROW_ABOVE = 0\.75, TR_GROW = 3\.0", hdr) and "radius = fmax(radius, TR_GROW * step_norm)" in hdr
    assert "#include" not in hdr.replace("#include <math.h>", "") and "__host__ __device__ __forceinline__" in hdr          # no HIP header on any path
    assert "tr_grad_max_rot(" in _code(os.path.join(CSRC, "tr_math_device.h"))
    calls = {
        "solver_kernels.hip": ["tr_dogleg_coeffs(", "tr_step_element(", "tr_parameter_converged(", "tr_function_converged(", "tr_step_quality(", "tr_step_accepted(",
                               "tr_dogleg_accepted_radius(", "tr_mu_accepted(", "tr_dogleg_rejected_radius(", "tr_lm_accepted_radius(", "tr_cube_pow(", "tr_lm_rejected(",
                               "tr_iteration_gate(", "tr_invalid_limit(", "tr_jacobi_scale(", "tr_clip_diagonal(", "tr_grad_max_rot("],
        "batch_tr_kernels.hip": ["tr_dogleg_coeffs(", "tr_parameter_converged(", "tr_function_converged(", "tr_step_quality(", "tr_step_accepted(", "tr_dogleg_accepted_radius(",
                                 "tr_mu_accepted(", "tr_dogleg_rejected_radius(", "tr_invalid_limit(", "tr_jacobi_scale(", "tr_clip_diagonal(", "tr_grad_max_rot("],
        "trajectory_kernels.hip": ["tr_dogleg_coeffs(", "tr_parameter_converged(", "tr_function_converged(", "tr_step_quality(", "tr_step_accepted(", "tr_dogleg_accepted_radius(",
                                   "tr_mu_accepted(", "tr_dogleg_rejected_radius(", "tr_invalid_limit(", "tr_jacobi_scale(", "tr_clip_diagonal_minmax("],
        "posegraph_kernels.hip": ["tr_step_quality(", "tr_step_accepted(", "tr_lm_accepted_radius(", "tr_cube_mul(", "tr_lm_rejected(", "tr_clip_diagonal("],
    }
    for name, fns in calls.items():
        src = _code(os.path.join(CSRC, name))
        assert '#include "tr_math.h"' in src, name
        for fn in fns:
            assert fn in src, (name, fn)
    # the two step tails of the window call the per-element function: the fused tail of k_chain_step and tr_dogleg_body
    assert _code(os.path.join(CSRC, "solver_kernels.hip")).count("tr_step_element(") == 2 and _code(os.path.join(CSRC, "solver_kernels.hip")).count("tr_dogleg_coeffs(") == 2
    for name in sorted(os.listdir(CSRC)):
        if name in ("tr_math.h", "tr_math_device.h"):
            continue
        src = _code(os.path.join(CSRC, name))
        assert "b_dot_a" not in src and "b_minus_a_sq" not in src, name
        assert not re.search(r"[<>] 0\.75\b", src) and not re.search(r"fmax\([a-z_.]*radius, 3\.0 \*", src), name
        assert not re.search(r"fmax\(1e-8, 2\.0 \*", src) and not re.search(r"\? 1e-6 : \(", src) and "fmin(fmax(hs, 1e-6), 1e32)" not in src, name
        assert "1.0 / (1.0 + sqrt(" not in src, name
    # Ceres' defaults are no longer bare literals in the trajectory's loop
    traj = _code(os.path.join(CSRC, "trajectory_kernels.hip"))
    loop = traj[traj.index("int term = GLIO_TRAJ_NOT_SOLVED"):traj.index("size_t round64")]
    for lit in ("1e4", "1e-8", "1e-10", "1e-32", "1e-6", "1e-3", "1e32", ">= 5", "10.0", "0.25", "0.75", "3.0"):
        assert not re.search(r"(?<![\w.])" + re.escape(lit) + r"(?![\w.])", loop), lit
    # the oracle and the restatements stay independent
    for rel in ("oracle/orc_solver.c", "oracle/orc_batch2.c", "tests/np_ceres.py", "tests/trajectory_restated.py"):
        assert "tr_math" not in open(os.path.join(ROOT, rel)).read(), rel
    assert "tr_math.h" in open(os.path.join(ROOT, "glio_amd", "build.py")).read()

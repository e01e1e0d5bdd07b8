"""The damped solve of the pose graph (glio_pgraph_solve_damped, include/glio_pgraph_lm.h) restated in numpy on top of pose_graph_restated: Ceres 1.14's
LevenbergMarquardtStrategy in the monotonic trust-region loop, on the graph's own normal equations, retraction and error E = 1/2 |r|^2, without Jacobi
scaling, with the same three interchangeable linear solvers.  It never imports the product and the product never imports it.  Ceres is restated from its
published behaviour (UNPINNED), as GTSAM is in pose_graph_restated.

A history row is [E tried (E itself for an invalid trial), the radius used, the model decrease m, 1 accepted / 0 rejected / -1 invalid]."""
import numpy as np

import pose_graph_restated as W

CONVERGED, ITERATION_LIMIT, MIN_RADIUS = 1, 2, 4
DEFAULTS = dict(initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_diagonal=1e-6, max_diagonal=1e32)


def radius_accepted(radius, gain, max_radius=DEFAULTS["max_radius"]):
    """StepAccepted: the new radius; the decrease factor goes back to 2"""
    c = 2.0 * gain - 1.0
    return min(max_radius, radius / max(1.0 / 3.0, 1.0 - c * c * c))


def radius_rejected(radius, decrease_factor):
    """StepRejected (and an invalid step): (the new radius, the new decrease factor)"""
    return radius / decrease_factor, decrease_factor * 2.0


def radius_update(radius, decrease_factor, accepted, gain, max_radius=DEFAULTS["max_radius"]):
    """the loop's whole radius state after a trial: (radius, decrease factor)"""
    if accepted:
        return radius_accepted(radius, gain, max_radius), 2.0
    return radius_rejected(radius, decrease_factor)


def normal_diagonal(J):
    """diag(J^T J), dense or scipy.sparse"""
    if isinstance(J, np.ndarray):
        return np.einsum("ij,ij->j", J, J)
    return np.asarray(J.multiply(J).sum(axis=0)).ravel()


def damping(J, min_diagonal=DEFAULTS["min_diagonal"], max_diagonal=DEFAULTS["max_diagonal"]):
    """d_i = clamp(H_ii, min_diagonal, max_diagonal)"""
    return np.clip(normal_diagonal(J), min_diagonal, max_diagonal)


def damped_step(J, r, d, radius, solver):
    """(H + diag(d) / radius) delta = -g; raises numpy.linalg.LinAlgError on a matrix that is not positive definite"""
    add = d / radius
    if solver == "lstsq":
        A = np.vstack([J, np.diag(np.sqrt(add))])
        return np.linalg.lstsq(A, -np.r_[r, np.zeros(len(add))], rcond=None)[0]
    if solver == "cholesky":
        import scipy.linalg as sl
        H = J.T @ J
        H[np.diag_indices_from(H)] += add
        return sl.cho_solve(sl.cho_factor(H, lower=True), -(J.T @ r))
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    H = ((J.T @ J) + sp.diags(add)).tocsc()
    return spl.splu(H, permc_spec="COLAMD", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(-(J.T @ r))


def model_decrease(delta, g, d, radius):
    """m = -(g^T delta + 1/2 delta^T H delta); by the step equation H delta = -g - (d / radius) delta this is 1/2 sum_i delta_i (d_i delta_i / radius - g_i)"""
    return 0.5 * float(np.sum(delta * (d * delta / radius - g)))


def model_decrease_from_jacobian(J, r, delta):
    Jd = J @ delta
    return -(float((J.T @ r) @ delta) + 0.5 * float(Jd @ Jd))


def levenberg_marquardt(g, x0, solver="cholesky", max_trials=100, rel_tol=1e-5, abs_tol=1e-5, **kw):
    """Returns the poses (the last accepted estimate) and a dict: trials, accepted, rejected (invalid ones included), invalid, initial_error, final_error,
    final_radius, termination, history [trials][4], steps (delta per trial, None for an invalid one)."""
    o = dict(DEFAULTS, **kw)
    sparse = solver == "sparse"
    x = np.array(x0, float)
    r, J = g.linearize(x, sparse=sparse)
    e0 = cur = 0.5 * float(r @ r)
    radius, factor = o["initial_radius"], 2.0
    hist, steps = [], []
    acc = rej = inv = 0
    reason = ITERATION_LIMIT
    while len(hist) < max_trials:
        d = damping(J, o["min_diagonal"], o["max_diagonal"])
        grad = np.asarray(J.T @ r).ravel()
        try:
            delta = np.asarray(damped_step(J, r, d, radius, solver), float).ravel()
            m = model_decrease(delta, grad, d, radius) if np.isfinite(delta).all() else np.nan
        except (np.linalg.LinAlgError, RuntimeError):
            delta, m = None, np.nan
        valid = bool(m > 0.0) and bool(np.isfinite(m))
        accepted = False
        if valid:
            xc = np.array([W.retract(x[i], delta[6 * i:6 * i + 6]) for i in range(len(x))])
            rc, Jc = g.linearize(xc, sparse=sparse)
            ec = 0.5 * float(rc @ rc)
            gain = (cur - ec) / m
            accepted = bool(gain > o["min_relative_decrease"])
            hist.append([ec, radius, m, 1.0 if accepted else 0.0])
            steps.append(delta)
        else:
            hist.append([cur, radius, 0.0 if delta is None else m, -1.0])
            steps.append(None)
            inv += 1
        stop = False
        radius, factor = radius_update(radius, factor, accepted, gain if accepted else None, o["max_radius"])
        if accepted:
            acc += 1
            dec = cur - ec
            stop = ec <= 0.0 or (rel_tol != 0.0 and dec / cur <= rel_tol) or dec <= abs_tol
            x, r, J, cur = xc, rc, Jc, ec
            if stop:
                reason = CONVERGED
        else:
            rej += 1
            if radius <= o["min_radius"]:
                stop, reason = True, MIN_RADIUS
        if stop:
            break
    return x, dict(trials=len(hist), accepted=acc, rejected=rej, invalid=inv, initial_error=e0, final_error=cur, final_radius=radius, termination=reason,
                   history=np.array(hist, float).reshape(-1, 4), steps=steps)


# (n, rot, trans, seed): circle_truth(n) through noisy_odometry, the reference's prior and odometry variances, one loop n - 1 -> 2 with variance 0.09: drives whose
# drift makes the first undamped Gauss-Newton step RAISE the error
DRIFT_SCENES = ((150, 5e-2, 3e-2, 1), (150, 5e-2, 3e-2, 2), (120, 0.1, 0.1, 2), (200, 3e-2, 3e-2, 1))


def drift_scene(n, rot, trans, seed, loop_var=0.09):
    """Returns (initial poses, loop (i, j, rel, var), Graph)"""
    truth = W.circle_truth(n)
    x0 = W.noisy_odometry(truth, np.random.default_rng(seed), rot, trans)
    loop = (n - 1, 2, W.between(truth[n - 1], truth[2]), np.full(6, loop_var))
    g = W.Graph()
    g.add_prior(0, x0[0])
    g.add_chain(x0)
    g.add_between(*loop)
    return x0, loop, g

"""The pose graph of include/glio_hip.h (glio_pgraph_*) restated in numpy: the three factors with analytic Jacobians, the retraction (rotation first),
Gauss-Newton with gtsam::GaussNewtonParams' termination on the total error, and three interchangeable linear solvers -- numpy.linalg.lstsq on the stacked
Jacobian, a dense Cholesky of J^T J, and scipy.sparse + splu of J^T J for long graphs.  It never imports the product and the product never imports it.
GTSAM is not part of the reference tree: like the header, this file restates published behaviour (UNPINNED).

Poses are rows t[3], q[4] (w first)."""
import numpy as np

PRIOR_VAR = np.array([1e-2, 1e-2, np.pi ** 2, 1e8, 1e8, 1e8])          # Estimator.cpp:864
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])             # Estimator.cpp:865
LOG_SERIES_BELOW = 1e-3          # |v| of the quaternion
JRINV_SERIES_BELOW = 1e-2        # theta
CONVERGED, ITERATION_LIMIT = 1, 2


def q_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def q_conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


def q_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def so3_log(q):
    """Log of a unit quaternion as a rotation vector in (-pi, pi]"""
    q = np.asarray(q, float)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    if s < LOG_SERIES_BELOW:
        u = s / q[0]
        k = 2.0 / q[0] * (1.0 - u * u / 3.0 + u ** 4 / 5.0)
    else:
        k = 2.0 * np.arctan2(s, q[0]) / s
    return k * q[1:]


def so3_exp(d):
    d = np.asarray(d, float)
    t = np.linalg.norm(d)
    k = 0.5 - t * t / 48.0 + t ** 4 / 3840.0 if t < 1e-3 else np.sin(0.5 * t) / t
    return np.r_[np.cos(0.5 * t), k * d]


def jr_inv(phi):
    """inverse right Jacobian of SO(3): I + 1/2 [phi]x + (1/theta^2 - (1 + cos theta) / (2 theta sin theta)) [phi]x^2"""
    t = np.linalg.norm(phi)
    c = 1.0 / 12.0 + t * t / 720.0 + t ** 4 / 30240.0 if t < JRINV_SERIES_BELOW else 1.0 / (t * t) - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    K = skew(phi)
    return np.eye(3) + 0.5 * K + c * (K @ K)


def between(a, b):
    """a^-1 b as t, q"""
    Ra = q_mat(a[3:])
    return np.r_[Ra.T @ (b[:3] - a[:3]), q_mul(q_conj(a[3:]), b[3:])]


def compose(a, rel):
    return np.r_[a[:3] + q_mat(a[3:]) @ rel[:3], q_mul(a[3:], rel[3:])]


def retract(x, d):
    """x [+] d, d = (d_r, d_t); unit quaternion with w >= 0"""
    q = q_mul(x[3:], so3_exp(d[:3]))
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    return np.r_[x[:3] + q_mat(x[3:]) @ d[3:], q]


def between_factor(xi, xj, m, var):
    w = 1.0 / np.sqrt(var)
    Ri, Rm = q_mat(xi[3:]), q_mat(m[3:])
    qij = q_mul(q_conj(xi[3:]), xj[3:])
    qe = q_mul(q_conj(m[3:]), qij)
    phi = so3_log(qe)
    u = Ri.T @ (xj[:3] - xi[:3])
    r = np.r_[phi, Rm.T @ (u - m[:3])] * w
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Jr = jr_inv(phi)
    Ji[:3, :3] = -Jr @ q_mat(qij).T
    Ji[3:, :3] = Rm.T @ skew(u)
    Ji[3:, 3:] = -Rm.T
    Jj[:3, :3] = Jr
    Jj[3:, 3:] = q_mat(qe)
    return r, Ji * w[:, None], Jj * w[:, None]


def prior_factor(x, m, var):
    w = 1.0 / np.sqrt(var)
    Rm = q_mat(m[3:])
    qe = q_mul(q_conj(m[3:]), x[3:])
    phi = so3_log(qe)
    r = np.r_[phi, Rm.T @ (x[:3] - m[:3])] * w
    J = np.zeros((6, 6))
    J[:3, :3] = jr_inv(phi)
    J[3:, 3:] = q_mat(qe)
    return r, J * w[:, None]


def gps_factor(x, p, var):
    w = 1.0 / np.sqrt(var)
    J = np.zeros((3, 6))
    J[:, 3:] = q_mat(x[3:])
    return (x[:3] - p) * w, J * w[:, None]


class Graph:
    """factors: ("between", i, j, meas[7], var[6]) | ("prior", i, meas[7], var[6]) | ("gps", i, p[3], var[3])"""

    def __init__(self):
        self.factors = []

    def add_between(self, i, j, meas, var):
        self.factors.append(("between", int(i), int(j), np.asarray(meas, float), np.asarray(var, float)))

    def add_prior(self, i, meas, var=PRIOR_VAR):
        self.factors.append(("prior", int(i), np.asarray(meas, float), np.asarray(var, float)))

    def add_gps(self, i, p, var, floor=1.0):
        self.factors.append(("gps", int(i), np.asarray(p, float), np.maximum(np.asarray(var, float), floor)))

    def add_chain(self, poses, var=ODOM_VAR, first=0):
        """what glio_pgraph_append adds: between(previous given pose, this given pose) per new node"""
        for k in range(1, len(poses)):
            self.add_between(first + k - 1, first + k, between(poses[k - 1], poses[k]), var)

    def blocks(self, x):
        """per factor: (row count, [(node, J block)], r)"""
        out = []
        for f in self.factors:
            if f[0] == "between":
                r, Ji, Jj = between_factor(x[f[1]], x[f[2]], f[3], f[4])
                out.append((r, [(f[1], Ji), (f[2], Jj)]))
            elif f[0] == "prior":
                r, J = prior_factor(x[f[1]], f[2], f[3])
                out.append((r, [(f[1], J)]))
            else:
                r, J = gps_factor(x[f[1]], f[2], f[3])
                out.append((r, [(f[1], J)]))
        return out

    def error(self, x):
        return 0.5 * sum(float(r @ r) for r, _ in self.blocks(x))

    def linearize(self, x, sparse=False):
        bl = self.blocks(x)
        r = np.concatenate([b[0] for b in bl])
        n = 6 * len(x)
        if not sparse:
            J = np.zeros((len(r), n))
            at = 0
            for rr, parts in bl:
                for node, Jb in parts:
                    J[at:at + len(rr), 6 * node:6 * node + 6] = Jb
                at += len(rr)
            return r, J
        import scipy.sparse as sp
        by_rows, at = {}, 0                       # blocks grouped by their row count: the indices of a group come from one broadcast
        for rr, parts in bl:
            for node, Jb in parts:
                ats, nodes, Js = by_rows.setdefault(len(rr), ([], [], []))
                ats.append(at); nodes.append(node); Js.append(Jb)
            at += len(rr)
        rows, cols, vals = [], [], []
        for m, (ats, nodes, Js) in by_rows.items():
            shape = (len(ats), m, 6)
            rows.append(np.broadcast_to(np.array(ats)[:, None, None] + np.arange(m)[None, :, None], shape).ravel())
            cols.append(np.broadcast_to(6 * np.array(nodes)[:, None, None] + np.arange(6)[None, None, :], shape).ravel())
            vals.append(np.array(Js).ravel())
        return r, sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(r), n))


def step_lstsq(J, r):
    return np.linalg.lstsq(J, -r, rcond=None)[0]


def step_cholesky(J, r):
    import scipy.linalg as sl
    return sl.cho_solve(sl.cho_factor(J.T @ J, lower=True), -(J.T @ r))


def step_sparse(J, r):
    import scipy.sparse.linalg as spl
    H = (J.T @ J).tocsc()
    return spl.splu(H, permc_spec="COLAMD", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(-(J.T @ r))


STEPS = {"lstsq": step_lstsq, "cholesky": step_cholesky, "sparse": step_sparse}


def gauss_newton(g, x0, solver="cholesky", max_iterations=100, rel_tol=1e-5, abs_tol=1e-5, fixed=False):
    """Gauss-Newton without damping.  fixed: exactly max_iterations iterations.  Otherwise after every iteration stop when E_new <= 0, or
    (E - E_new) / E <= rel_tol, or E - E_new <= abs_tol (gtsam::checkConvergence), or at max_iterations.  Returns the poses and a dict."""
    x = np.array(x0, float)
    r, J = g.linearize(x, sparse=(solver == "sparse"))
    e0 = cur = 0.5 * float(r @ r)
    it, reason = 0, ITERATION_LIMIT
    while it < max_iterations:
        d = STEPS[solver](J, r)
        x = np.array([retract(x[i], d[6 * i:6 * i + 6]) for i in range(len(x))])
        it += 1
        r, J = g.linearize(x, sparse=(solver == "sparse"))
        new = 0.5 * float(r @ r)
        dec = cur - new
        conv = new <= 0.0 or (rel_tol != 0.0 and cur != 0.0 and dec / cur <= rel_tol) or dec <= abs_tol
        cur = new
        if conv and not fixed:
            reason = CONVERGED
            break
    return x, dict(iterations=it, initial_error=e0, final_error=cur, termination=reason)


def marginal_covariance(g, x, node):
    """the node's 6x6 block of (J^T J)^-1, tangent frame of the retraction"""
    _, J = g.linearize(x)
    return np.linalg.inv(J.T @ J)[6 * node:6 * node + 6, 6 * node:6 * node + 6]


def spread(a, b, relative):
    """(max translation difference in m, max rotation difference in rad) between two pose tables; relative: each table first expressed in its own node 0"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if relative:
        a = np.array([between(a[0], p) for p in a])
        b = np.array([between(b[0], p) for p in b])
    dt = np.linalg.norm(a[:, :3] - b[:, :3], axis=1).max()
    da = max(np.linalg.norm(so3_log(q_mul(q_conj(p[3:]), q[3:]))) for p, q in zip(a, b))
    return float(dt), float(da)


def noisy_odometry(truth, rng, rot_noise, trans_noise):
    """dead reckoning through the true relative poses disturbed per edge: what a drifting front end hands to glio_pgraph_append"""
    x = [np.array(truth[0], float)]
    for k in range(1, len(truth)):
        rel = between(truth[k - 1], truth[k])
        rel = np.r_[rel[:3] + rng.normal(0, trans_noise, 3), q_mul(rel[3:], so3_exp(rng.normal(0, rot_noise, 3)))]
        x.append(compose(x[-1], rel))
    x = np.array(x)
    x[:, 3:] /= np.linalg.norm(x[:, 3:], axis=1)[:, None]
    x[x[:, 3] < 0, 3:] *= -1
    return x


def circle_truth(n, radius=20.0, turn=0.98, z_amp=0.0):
    out = []
    for k in range(n):
        a = 2 * np.pi * turn * k / (n - 1)
        yaw = a + np.pi / 2
        out.append(np.r_[radius * np.cos(a), radius * np.sin(a), z_amp * np.sin(2 * a), np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    return np.array(out)


CIRCLE_SEED = 20240607


def circle_scene(n=60, seed=CIRCLE_SEED, loop_var=0.09):
    """the 60-node circle: radius 20 m, 0.98 of a turn, odometry noise 2e-3 rad / 5e-3 m per edge, one loop from the last node to node 2 (variance 0.09), the
    reference's prior and odometry variances.  Returns (initial poses, loop (i, j, rel, var), Graph)."""
    truth = circle_truth(n)
    x0 = noisy_odometry(truth, np.random.default_rng(seed), 2e-3, 5e-3)
    loop = (n - 1, 2, between(truth[n - 1], truth[2]), np.full(6, loop_var))
    g = Graph()
    g.add_prior(0, x0[0])
    g.add_chain(x0)
    g.add_between(*loop)
    return x0, loop, g


def figure_eight_truth(n, radius=30.0):
    out = []
    for k in range(n):
        s = 2 * np.pi * k / n * 2.0            # two laps of the lemniscate-like curve
        x, y = radius * np.sin(s), radius * np.sin(s) * np.cos(s)
        dx, dy = radius * np.cos(s), radius * (np.cos(s) ** 2 - np.sin(s) ** 2)
        yaw = np.arctan2(dy, dx)
        out.append(np.r_[x, y, 0.5 * np.sin(3 * s), np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
    return np.array(out)

"""A numpy restatement of the every-frame trajectory (include/glio_traj.h), written from the reference's lines: the IMU fill-in between two keyframes
(GLIO/src/Estimator.cpp:4279-4493), the relative measurements (:4494-4555) and optimizeLocalGraph (:3452-3527) with the factors of
LidarPoseFactor.h:11-52, 128-221.  Scalar loops in Eigen's evaluation order for the recurrence; tests/np_ceres.py::minimize for the trust-region loop.
Pose rows are t[3], q[4] (w first); measurement rows dq[4] (w first), dp[3].  `cases()` is the case builder the CPU and the GPU tests share.
`branch_cases()`, `limit_cases()` and `resolve_cases()` are fixed lists beside it that reach every branch of the trust-region loop the public API can reach
(the dogleg's three branches, the four radius rules, five ends, both sides of every pass boundary of the device's evaluate(), max_iterations 0 / 1 / 32),
each case with its margins (`assert_margins`), its one-ulp noise floor and the gate that follows from it (`noise_floor`); `local_graph` takes the census
beside np_ceres.minimize without touching its arithmetic, and `assert_same_solve` is the one comparison the device and the deliberately wrong variants of
tests/test_trajectory_restated.py are held to.  The branches that cannot be reached, and why, are listed in `branch_cases()`.  The seeds were picked by
scripts/search_trajectory_branch_cases.py."""
import numpy as np

import np_ceres

ACC_CLAMP = (15.0, 15.0, 18.0)
WEIGHT = 0.2
OPTIONS = dict(max_iterations=15, strategy="dogleg", dogleg="traditional", nonmonotonic=False)


# ------------------------------------------------------------------ Eigen's quaternion routines, as the reference's doubles go through them
def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def qinv(q):
    """inverse() = conjugate / |q|^2"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2])


def qrot(q, v):
    """q * v (_transformVector) on the quaternion as it is: v + w uv + u x uv with uv = 2 (u x v)"""
    uv = [q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    uuv = [q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]]
    return np.array([v[0] + q[0] * uv[0] + uuv[0], v[1] + q[0] * uv[1] + uuv[1], v[2] + q[0] * uv[2] + uuv[2]])


def q2R(q):
    """toRotationMatrix(), no normalisation"""
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def quat_from_matrix(m):
    """Quaterniond(Matrix3d), Eigen 3.3's quaternionbase_assign_impl: returns (q, branch) with branch 0 = trace, 1 + i = diagonal i"""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2][1] - m[1][2]) * t
        q[2] = (m[0][2] - m[2][0]) * t
        q[3] = (m[1][0] - m[0][1]) * t
        return np.array(q), 0
    i = 0
    if m[1][1] > m[0][0]:
        i = 1
    if m[2][2] > m[i][i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
    q[1 + i] = 0.5 * t
    t = 0.5 / t
    q[0] = (m[k][j] - m[j][k]) * t
    q[1 + j] = (m[j][i] + m[i][j]) * t
    q[1 + k] = (m[k][i] + m[i][k]) * t
    return np.array(q), 1 + i


def _clamp3(v):
    out = []
    for k in range(3):
        x = float(v[k])
        if x > ACC_CLAMP[k]:
            x = ACC_CLAMP[k]
        if x < -ACC_CLAMP[k]:
            x = -ACC_CLAMP[k]
        out.append(x)
    return out


class _State:
    def __init__(self, P, V, R, g):
        self.P = [float(v) for v in P]
        self.V = [float(v) for v in V]
        self.R = [[float(np.asarray(R).reshape(3, 3)[i][j]) for j in range(3)] for i in range(3)]
        self.g = [float(v) for v in g]

    def step(self, a0, gy0, a1, gy1, dt):
        """:4330-4336 with Ba = Bg = 0"""
        R, g = self.R, self.g
        un0 = [R[i][0] * a0[0] + R[i][1] * a0[1] + R[i][2] * a0[2] - g[i] for i in range(3)]
        ug = [0.5 * (gy0[k] + gy1[k]) for k in range(3)]
        D = q2R([1.0, ug[0] * dt / 2.0, ug[1] * dt / 2.0, ug[2] * dt / 2.0])
        R = [[R[i][0] * D[0][j] + R[i][1] * D[1][j] + R[i][2] * D[2][j] for j in range(3)] for i in range(3)]
        un1 = [R[i][0] * a1[0] + R[i][1] * a1[1] + R[i][2] * a1[2] - g[i] for i in range(3)]
        un = [0.5 * (un0[k] + un1[k]) for k in range(3)]
        self.P = [self.P[k] + (dt * self.V[k] + 0.5 * dt * dt * un[k]) for k in range(3)]
        self.V = [self.V[k] + dt * un[k] for k in range(3)]
        self.R = R

    def row(self):
        q, br = quat_from_matrix(self.R)
        return np.concatenate([self.P, q]), br


def fill_in_direct(stamps, acc, gyr, frame_stamps, ii, P, V, R, g):
    """Estimator.cpp:4279-4493 read straight off the buffers: frame_stamps = the stamps of frames keyframe_id_in_frame[a] .. [b], ii = imu_idx_in_kf[a].
    Returns the dead-reckoned rows [(N + 1)][7] (the last at b's stamp), the Quaterniond(Matrix3d) branch of each and the sample rows per segment as the
    reference consumed them ([(dt, acc, gyr)], the first one the start row with dt 0) -- what the library's frame_samples has to reproduce."""
    st = _State(P, V, R, g)
    M = len(frame_stamps) - 1
    rows, branches, segments = [], [], []
    ii = int(ii)
    for i in range(1, M + 1):
        last = i == M
        t0, t1 = float(frame_stamps[i - 1]), float(frame_stamps[i])
        dt1 = t0 - float(stamps[ii])
        dt2 = float(stamps[ii + 1]) - t0
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = [w1 * float(acc[ii][k]) + w2 * float(acc[ii + 1][k]) for k in range(3)]
        r = [w1 * float(gyr[ii][k]) + w2 * float(gyr[ii + 1][k]) for k in range(3)]
        if last:
            d = _clamp3(d)                       # :4413-4419; the in-between segments do not clamp their start row (:4295-4301)
        a0, gy0 = list(d), list(r)
        seg = [[0.0] + a0 + gy0]
        ii += 1
        start = t0
        while float(stamps[ii]) < t1:
            t = float(stamps[ii])
            dt = t - start
            start = t
            d = _clamp3(acc[ii])
            r = [float(gyr[ii][k]) for k in range(3)]
            st.step(a0, gy0, d, r, dt)
            seg.append([dt] + d + r)
            a0, gy0 = list(d), list(r)
            ii += 1
        dt1 = t1 - float(stamps[ii - 1])
        dt2 = float(stamps[ii]) - t1
        w1 = dt2 / (dt1 + dt2)
        w2 = dt1 / (dt1 + dt2)
        d = _clamp3([w1 * d[k] + w2 * float(acc[ii][k]) for k in range(3)])          # d, r: the last whole sample's (clamped) values, or the start row's
        r = [w1 * r[k] + w2 * float(gyr[ii][k]) for k in range(3)]
        st.step(a0, gy0, d, r, dt1)
        seg.append([dt1] + d + r)
        if not last:
            ii -= 1                              # :4375
        row, br = st.row()
        rows.append(row)
        branches.append(br)
        segments.append(np.array(seg))
    return np.array(rows), branches, segments


def dead_reckon(seg_offset, samples, P, V, R, g):
    """the kernel's reading of the same recurrence: sample rows with per-segment offsets, the first row of a segment only sets a0, gy0"""
    st = _State(P, V, R, g)
    samples = np.asarray(samples, float).reshape(-1, 7)
    rows, branches = [], []
    for s in range(len(seg_offset) - 1):
        a0 = gy0 = None
        for k in range(int(seg_offset[s]), int(seg_offset[s + 1])):
            dt, a1, gy1 = float(samples[k][0]), [float(v) for v in samples[k][1:4]], [float(v) for v in samples[k][4:7]]
            if a0 is not None:
                st.step(a0, gy0, a1, gy1, dt)
            a0, gy0 = a1, gy1
        row, br = st.row()
        rows.append(row)
        branches.append(br)
    return np.array(rows).reshape(-1, 7), branches


def measurements(prev_row, rows):
    """:4494-4555: row i relates pose row i - 1 (prev_row for i = 0) to pose row i"""
    out = []
    a = np.asarray(prev_row, float)
    for b in np.asarray(rows, float).reshape(-1, 7):
        qi = qinv(a[3:7])
        out.append(np.concatenate([qmul(qi, b[3:7]), qrot(qi, b[0:3] - a[0:3])]))
        a = b
    return np.array(out).reshape(-1, 7)


def compose(a, m):
    return np.concatenate([a[0:3] + qrot(a[3:7], m[4:7]), qmul(a[3:7], m[0:4])])


def resolve_init(meas, left, N):
    """glio_traj_resolve's initial chain: pose 0 = left (+) measurement 0, pose i + 1 = pose i (+) measurement i"""
    out, cur = [], np.asarray(left, float)
    for i in range(N):
        cur = compose(cur, meas[0 if i == 0 else i - 1])
        out.append(cur)
    return np.array(out).reshape(-1, 7)


# ------------------------------------------------------------------ the factor (LidarPoseFactor.h:11-52): residual and analytic Jacobians
def _qleft(q):
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]])


def _qright(p):
    w, x, y, z = p
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]])


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def plus_jacobian(q):
    """d ([cos|d|, sin|d| d / |d|] (x) q) / d d at 0, 4 x 3: Ceres' QuaternionParameterization"""
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]])


def quat_plus(q, d):
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if n > 0.0:
        s = np.sin(n) / n
        return qmul(np.array([np.cos(n), s * d[0], s * d[1], s * d[2]]), q)
    return np.array(q, float)


def factor_residual(m, pa, pb, wq=WEIGHT, wp=WEIGHT):
    A, u = qinv(m[0:4]), qinv(pa[3:7])
    p = qmul(qmul(A, u), pb[3:7])
    return np.concatenate([wq * (2.0 * p[1:4]), wp * (qrot(u, pb[0:3] - pa[0:3]) - m[4:7])])


def factor_global(m, pa, pb, wq=WEIGHT, wp=WEIGHT):
    """r [6] and the global Jacobians wrt (p1 [6x3], q1 [6x4], p2 [6x3], q2 [6x4])"""
    q1, q2 = pa[3:7], pb[3:7]
    A, u = qinv(m[0:4]), qinv(q1)
    Au = qmul(A, u)
    v = pb[0:3] - pa[0:3]
    n2 = q1 @ q1
    conj = np.array([q1[0], -q1[1], -q1[2], -q1[3]])
    du_dq1 = (np.diag([1.0, -1.0, -1.0, -1.0]) - 2.0 * np.outer(conj, q1) / n2) / n2
    J_q1 = np.zeros((6, 4))
    J_q2 = np.zeros((6, 4))
    J_q1[0:3] = wq * 2.0 * (_qleft(A) @ _qright(q2))[1:4] @ du_dq1
    J_q2[0:3] = wq * 2.0 * _qleft(Au)[1:4]
    w, qv = u[0], u[1:4]
    G = np.zeros((3, 4))
    G[:, 0] = 2.0 * np.cross(qv, v)
    G[:, 1:4] = -2.0 * w * _skew(v) + 2.0 * ((qv @ v) * np.eye(3) + np.outer(qv, v) - 2.0 * np.outer(v, qv))
    J_q1[3:6] = wp * G @ du_dq1
    Mu = np.eye(3) + 2.0 * w * _skew(qv) + 2.0 * (_skew(qv) @ _skew(qv))
    J_p1 = np.zeros((6, 3))
    J_p2 = np.zeros((6, 3))
    J_p1[3:6], J_p2[3:6] = -wp * Mu, wp * Mu
    return factor_residual(m, pa, pb, wq, wp), J_p1, J_q1, J_p2, J_q2


def factor_local(m, pa, pb):
    """r [6], Ja [6x6], Jb [6x6] in the local parameterisation (t, then the rotation)"""
    r, Jp1, Jq1, Jp2, Jq2 = factor_global(m, pa, pb)
    return r, np.hstack([Jp1, Jq1 @ plus_jacobian(pa[3:7])]), np.hstack([Jp2, Jq2 @ plus_jacobian(pb[3:7])])


def factor_list(N):
    """(first pose or -1 = left anchor, second pose or -1 = right anchor, measurement) of the N + 1 factors; the between factor i -> i + 1 takes
    measurement i, as written at :3490-3491"""
    out = [(-1, 0, 0)]
    for i in range(N - 1):
        out.append((i, i + 1, i))
    out.append((N - 1, -1, N))
    return out


class LocalGraph:
    def __init__(self, meas, left, right):
        self.meas, self.left, self.right = np.asarray(meas, float).reshape(-1, 7), np.asarray(left, float), np.asarray(right, float)

    def evaluate(self, x):
        N = len(x)
        H, g, cost = np.zeros((6 * N, 6 * N)), np.zeros(6 * N), 0.0
        for a, b, mi in factor_list(N):
            pa = self.left if a < 0 else x[a]
            pb = self.right if b < 0 else x[b]
            r, Ja, Jb = factor_local(self.meas[mi], pa, pb)
            cost += 0.5 * (r @ r)
            if a >= 0:
                H[6 * a:6 * a + 6, 6 * a:6 * a + 6] += Ja.T @ Ja
                g[6 * a:6 * a + 6] += Ja.T @ r
            if b >= 0:
                H[6 * b:6 * b + 6, 6 * b:6 * b + 6] += Jb.T @ Jb
                g[6 * b:6 * b + 6] += Jb.T @ r
            if a >= 0 and b >= 0:
                H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += Ja.T @ Jb
                H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += Jb.T @ Ja
        if not (np.isfinite(cost) and np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
            return None
        return cost, H, g

    @staticmethod
    def plus(x, delta):
        out = np.array(x, float)
        for k in range(len(x)):
            out[k, 0:3] = x[k, 0:3] + delta[6 * k:6 * k + 3]
            out[k, 3:7] = quat_plus(x[k, 3:7], delta[6 * k + 3:6 * k + 6])
        return out

    @staticmethod
    def flat(x):
        return np.asarray(x, float).reshape(-1)


NOT_SOLVED = 6
DOGLEG_BRANCHES = ("gn", "cauchy", "interp")
RADIUS_RULES = ("grow", "keep", "shrink_on_accept", "reject")


class CensusDogleg(np_ceres.Dogleg):
    """np_ceres.Dogleg with a log beside it: one record per step computed (which branch of the traditional dogleg, the two ratios its conditions compare
    with 1, the sign of c on the interpolated branch) and the radius rule that judged it.  Every number is the parent's: the methods record and delegate."""
    log = None          # a list, given by local_graph through a subclass of its own

    def _traditional_step(self):
        g, gn, r, a = self.grad, self.gn, self.radius, self.alpha
        ngn, ng = np.linalg.norm(gn), np.linalg.norm(g)
        branch = "gn" if ngn <= r else ("cauchy" if ng * a >= r else "interp")
        self.log.append(dict(branch=branch, gn_over_radius=float(ngn / r), cauchy_over_radius=float(ng * a / r), c=float(-a * (g @ gn) - a * a * (g @ g)), rule=None))
        return super()._traditional_step()

    def accepted(self, q):
        self.log[-1]["rule"] = "shrink_on_accept" if q < 0.25 else ("grow" if q > 0.75 else "keep")
        super().accepted(q)

    def rejected(self):
        self.log[-1]["rule"] = "reject"
        super().rejected()


def local_graph(meas, left, right, x0, max_iterations=15, dogleg=CensusDogleg, graph=None, take_candidate=False):
    """optimizeLocalGraph: returns (poses [N][7], summary, trace); summary carries accepted_mask (bit k: iteration k + 1 accepted), `qualities` (the step
    quality of every judged iteration), `census` (per judged iteration the pair (dogleg branch, radius rule) of DOGLEG_BRANCHES x RADIUS_RULES), `dogleg`
    (CensusDogleg's record of every iteration, the one a tolerance ended included) and `starts` (per iteration the gradient max norm and |x| at its start,
    and as the last row those at the loop's last test).  The census is taken beside np_ceres.minimize, not in it: `dogleg` is a subclass of np_ceres.Dogleg
    that minimize() finds under the module's name for the length of the call.
    For tests/test_trajectory_restated.py's deliberately wrong variants only: another `dogleg` class, another `graph` class (LocalGraph's interface) and
    take_candidate (the candidate's poses and cost delivered at a FUNCTION or PARAMETER tolerance end)."""
    x0 = np.asarray(x0, float).reshape(-1, 7)
    if len(x0) == 0:
        return x0, dict(termination=NOT_SOLVED, iterations=0, successful_steps=0, initial_cost=0.0, final_cost=0.0, accepted_mask=0, qualities=[], census=[],
                        dogleg=[], starts=[], hist=[]), []
    lg = (graph or LocalGraph)(meas, left, right)
    seen = []

    def evaluate(x):
        with np.errstate(over="ignore", invalid="ignore"):          # a cost that overflows is the FAILURE case, not a warning
            ev = lg.evaluate(x)
        seen.append((np.array(x, float), None if ev is None else ev[0]))
        return ev
    trace, log = [], []
    saved, np_ceres.Dogleg = np_ceres.Dogleg, type("Dogleg", (dogleg,), dict(log=log))
    try:
        x, summ, hist = np_ceres.minimize(x0, evaluate, lg.plus, lg.flat, np_ceres.Options(**dict(OPTIONS, max_iterations=max_iterations)), trace=trace)
    finally:
        np_ceres.Dogleg = saved
    if summ["termination"] == np_ceres.FAILURE and summ["iterations"] == 0:          # the evaluation at entry failed: nothing was judged
        summ = dict(summ, successful_steps=0, initial_cost=float("nan"), final_cost=float("nan"))
    mask, qualities = 0, []
    for k, row in enumerate(trace):               # one row per judged iteration (no invalid steps arise here: asserted by the case builder)
        if row["ratio"] > 1e-3:
            mask |= 1 << k
        qualities.append(float(row["ratio"]))
    starts, cur = [], x0
    for k in range(summ["iterations"] + 1):
        with np.errstate(over="ignore", invalid="ignore"):
            ev = lg.evaluate(cur)
        if ev is not None:
            starts.append((float(np.abs(lg.flat(cur) - lg.flat(lg.plus(cur, -ev[2]))).max()), float(np.linalg.norm(lg.flat(cur)))))
        if k < len(trace) and "x" in trace[k]:
            cur = trace[k]["x"].reshape(-1, 7)
    summ = dict(summ, accepted_mask=mask, qualities=qualities, hist=hist, dogleg=log, census=[(r["branch"], r["rule"]) for r in log if r["rule"] is not None],
                starts=starts)
    x = np.asarray(x, float).reshape(-1, 7)
    if take_candidate and summ["termination"] in (np_ceres.FUNCTION_TOL, np_ceres.PARAMETER_TOL):
        x, summ["final_cost"] = seen[-1][0].reshape(-1, 7), seen[-1][1]
    return x, summ, trace


def gap(seg_offset, samples, P, V, R, g, prev_row, left, right, max_iterations=15):
    """glio_traj_push_gap restated: (dead-reckoned rows, measurements, solved rows, summary, branches)"""
    rows, branches = dead_reckon(seg_offset, samples, P, V, R, g)
    meas = measurements(prev_row, rows)
    N = len(rows) - 1
    sol, summ, _ = local_graph(meas, left, right, rows[:N], max_iterations)
    return rows, meas, sol, summ, branches


# ------------------------------------------------------------------ the shared case builder
def rot_q(axis, angle):
    axis = np.asarray(axis, float)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def q2R_np(q):
    return np.array(q2R(q))


def make_gap(seed, n_frames, samples_per_segment=8, heading=(0.0, 0.0, 1.0, 0.0), acc_scale=1.0, gyr_scale=0.2, anchor_noise=(0.02, 0.01),
             right_jump=None, dt=0.005):
    """A synthetic gap: sample rows per segment (start row + samples_per_segment whole rows + the closing row; samples_per_segment may be a list),
    a start state with the given heading (axis x, y, z, angle), anchors near the dead-reckoned ends.  right_jump = (dx, dy, dz, angle): the right anchor
    moved away by that much.  Returns a dict with the arguments of glio_traj_push_gap."""
    rng = np.random.RandomState(seed)
    per = samples_per_segment if isinstance(samples_per_segment, (list, tuple)) else [samples_per_segment] * (n_frames + 1)
    assert len(per) == n_frames + 1
    g = np.array([0.0, 0.0, 9.805])
    q0 = rot_q(heading[0:3], heading[3]) if heading[3] != 0.0 else np.array([1.0, 0, 0, 0])
    R0 = q2R_np(q0)
    offs, rows = [0], []
    for s in range(n_frames + 1):
        n = per[s] + 2 if per[s] >= 0 else 1
        for k in range(n):
            a = R0.T @ g + acc_scale * rng.randn(3)
            w = gyr_scale * rng.randn(3)
            rows.append(np.concatenate([[0.0 if k == 0 else dt * (0.5 + rng.rand())], a, w]))
        offs.append(len(rows))
    samples = np.array(rows)
    P, V = rng.randn(3), 2.0 * rng.randn(3)
    prev = np.concatenate([P + 0.001 * rng.randn(3), q0])
    dr, _ = dead_reckon(offs, samples, P, V, R0, g)
    left = np.concatenate([prev[0:3] + anchor_noise[0] * rng.randn(3), qmul(prev[3:7], rot_q(rng.randn(3), anchor_noise[1]))])
    end = dr[-1]
    right = np.concatenate([end[0:3] + anchor_noise[0] * rng.randn(3), qmul(end[3:7], rot_q(rng.randn(3), anchor_noise[1]))])
    if right_jump is not None:
        right = np.concatenate([right[0:3] + np.asarray(right_jump[0:3], float), qmul(right[3:7], rot_q([0.3, -0.5, 0.8], right_jump[3]))])
    return dict(n_frames=n_frames, seg_offset=np.array(offs, np.int32), samples=samples, start_state=np.concatenate([P, V, R0.reshape(-1)]), gravity=g,
                prev_row=prev, anchor_left=left, anchor_right=right)


def restate(c, max_iterations=15):
    s = c["start_state"]
    return gap(c["seg_offset"], c["samples"], s[0:3], s[3:6], s[6:15].reshape(3, 3), c["gravity"], c["prev_row"], c["anchor_left"], c["anchor_right"], max_iterations)


FUNCTION_TOLERANCE, MIN_RELATIVE_DECREASE, PARAMETER_TOLERANCE, GRADIENT_TOLERANCE = 1e-6, 1e-3, 1e-8, 1e-10


def assert_margins(name, summ):
    """The conditions the GPU comparison relies on: every decision of the restated loop is away from its knife edge.
      * the step quality of every judged iteration is not within 0.05 of 0.25, 0.75 or min_relative_decrease;
      * at a FUNCTION_TOLERANCE end the ratio |cost change| / cost is not within a factor 2 of the tolerance, and no earlier iteration's ratio, nor any
        iteration's of a case that ends otherwise, was within a factor 2 of it either;
      * the same for the parameter tolerance with dx / (1e-8 (|x| + 1e-8)): below 0.5 at a PARAMETER_TOLERANCE end, above 2 at every other iteration;
      * the gradient max norm is below 0.5e-10 at a GRADIENT_TOLERANCE end and above 2e-10 at every iteration's start;
      * the two ratios the dogleg's branch conditions compare with 1, |gn| / radius and |g| alpha / radius, are not within 5 % of 1 at any iteration.
    A FAILURE at entry (the first evaluation is not finite) judges nothing and has no margin."""
    term = summ["termination"]
    if term == NOT_SOLVED or (term == np_ceres.FAILURE and summ["iterations"] == 0):
        return
    for q in summ["qualities"]:
        for edge in (0.25, 0.75, MIN_RELATIVE_DECREASE):
            assert abs(q - edge) > 0.05, (name, "step quality", q, "near", edge)
    ended = term in (np_ceres.FUNCTION_TOL, np_ceres.PARAMETER_TOL)
    assert len(summ["qualities"]) == summ["iterations"] - (1 if ended else 0), (name, "an invalid step arose")
    hist, starts = summ["hist"], summ["starts"]
    assert len(hist) == summ["iterations"] and len(starts) == summ["iterations"] + 1 and len(summ["dogleg"]) == summ["iterations"], (name, "an invalid step arose")
    cur = summ["initial_cost"]
    k = 0
    for ccost, radius, dx in hist:
        last = k == len(hist) - 1
        pratio = dx / (PARAMETER_TOLERANCE * (starts[k][1] + PARAMETER_TOLERANCE))
        if last and term == np_ceres.PARAMETER_TOL:
            assert pratio < 0.5, (name, "terminating parameter ratio", pratio)
            break
        assert pratio > 2.0, (name, "parameter ratio", pratio, "iteration", k + 1)
        ratio = abs(cur - ccost) / cur if cur > 0 else 0.0
        if last and term == np_ceres.FUNCTION_TOL:
            assert ratio < 0.5 * FUNCTION_TOLERANCE, (name, "terminating ratio", ratio)
        else:
            assert ratio > 2.0 * FUNCTION_TOLERANCE, (name, "ratio", ratio, "iteration", k + 1)
            if summ["qualities"][k] > MIN_RELATIVE_DECREASE:
                cur = ccost
        k += 1
    for k in range(summ["iterations"]):
        assert starts[k][0] > 2.0 * GRADIENT_TOLERANCE, (name, "gradient max norm", starts[k][0], "iteration", k + 1)
    if term == np_ceres.GRADIENT_TOL:
        assert starts[-1][0] < 0.5 * GRADIENT_TOLERANCE, (name, "terminating gradient max norm", starts[-1][0])
    for k, rec in enumerate(summ["dogleg"]):
        for key in ("gn_over_radius", "cauchy_over_radius"):
            assert abs(rec[key] - 1.0) > 0.05, (name, key, rec[key], "iteration", k + 1)
    assert term in (np_ceres.FUNCTION_TOL, np_ceres.NO_CONVERGENCE, np_ceres.GRADIENT_TOL, np_ceres.PARAMETER_TOL), (name, term)


_CASES = None


def cases():
    """[(name, gap dict, restated (rows, meas, sol, summary, branches))]: computed once, shared, left unchanged"""
    global _CASES
    if _CASES is None:
        specs = [
            ("nominal_3", dict(seed=11, n_frames=3)),
            ("nominal_1", dict(seed=12, n_frames=1)),
            ("nominal_2", dict(seed=13, n_frames=2)),
            ("two_passes_11", dict(seed=14, n_frames=11, samples_per_segment=2)),
            ("full_32", dict(seed=15, n_frames=32, samples_per_segment=1)),
            ("far_anchor_3", dict(seed=21, n_frames=3, right_jump=(5.0, 3.0, 0.5, 1.0))),
        ]
        out = []
        for name, kw in specs:
            c = make_gap(**kw)
            res = restate(c)
            assert_margins(name, res[3])
            out.append((name, c, res))
        _CASES = out
    return _CASES


# ------------------------------------------------------------------ the comparison the GPU tests and the CPU check of the case list share
def rel_dev(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0


def decisions(summ):
    return (summ["termination"], summ["iterations"], summ["successful_steps"], summ["accepted_mask"])


def assert_same_solve(name, got_poses, got_summ, want_poses, want_summ, gate=1e-9):
    """A solve (the device's, or a variant of the restatement) against the restatement: termination, iterations, successful_steps and accepted_mask equal;
    initial cost, final cost and poses within `gate` relative to max(1, |value|).  The costs of a FAILURE at entry are not finite and not compared.
    Returns (pose deviation, cost deviation)."""
    assert decisions(got_summ) == decisions(want_summ), (name, "decisions", decisions(got_summ), "restated", decisions(want_summ))
    d_pose = rel_dev(got_poses, want_poses)
    d_cost = 0.0
    if np.isfinite(want_summ["initial_cost"]) and np.isfinite(want_summ["final_cost"]):
        d_cost = max(rel_dev(got_summ["initial_cost"], want_summ["initial_cost"]), rel_dev(got_summ["final_cost"], want_summ["final_cost"]))
    assert d_pose <= gate, (name, "poses deviate by", d_pose, "gate", gate)
    assert d_cost <= gate, (name, "costs deviate by", d_cost, "gate", gate)
    return d_pose, d_cost


def one_ulp_up(a):
    return np.nextafter(np.asarray(a, float), np.inf)


def noise_floor(name, run, want):
    """The restatement's own noise on a case: `run()` solves it again with every input one ulp up and returns (poses, summary); the decisions must be the
    same and the largest pose / cost deviation relative to max(1, |value|) is the floor.  Returns (floor, gate = max(1e-9, 100 floor)): the factor 100 is for
    the device's other summation order (lane-strided partial sums joined by a butterfly against numpy's)."""
    poses, summ = run()
    w_poses, w_summ = want
    assert decisions(summ) == decisions(w_summ) and summ["census"] == w_summ["census"], (name, "one ulp on the inputs changes the decisions")
    floor = rel_dev(poses, w_poses)
    if np.isfinite(w_summ["initial_cost"]):
        floor = max(floor, rel_dev(summ["initial_cost"], w_summ["initial_cost"]), rel_dev(summ["final_cost"], w_summ["final_cost"]))
    assert floor <= 1e-7, (name, "noise floor", floor)
    return floor, max(1e-9, 100.0 * floor)


def gap_one_ulp_up(c):
    return dict(c, **{k: one_ulp_up(c[k]) for k in ("samples", "start_state", "gravity", "prev_row", "anchor_left", "anchor_right")})


def shifted(c, shift):
    """the gap moved as a whole by `shift` metres along every axis (UTM-like coordinates): start position, previous row and both anchors"""
    out = dict(c)
    for key in ("start_state", "prev_row", "anchor_left", "anchor_right"):
        v = np.array(c[key], float)
        v[0:3] += shift
        out[key] = v
    return out


# ------------------------------------------------------------------ stored gaps solved again between new keyframe rows (glio_traj_resolve)
def resolve_gap(spec, left):
    """One gap of a resolve: spec = dict(seed, n_frames, kind[, jump]); `left` the left keyframe row.  The right row is, by kind,
      consistent   compose(x[-1], meas[N]) of the start chain x: every factor is satisfied, GRADIENT_TOLERANCE before the first iteration;
      disturbed    left (+) the gap's own anchor-to-anchor relative pose, moved by a centimetre;
      closure      the same moved by jump = (dx, dy, dz, angle): a loop-closure-sized correction.
    Returns the gap's push arguments (`case`), its restated measurements, both rows and the restated resolve (`poses`, `summary`)."""
    N = spec["n_frames"]
    c = make_gap(seed=spec["seed"], n_frames=N, samples_per_segment=1)
    s = c["start_state"]
    rows, _ = dead_reckon(c["seg_offset"], c["samples"], s[0:3], s[3:6], s[6:15].reshape(3, 3), c["gravity"])
    meas = measurements(c["prev_row"], rows)
    left = np.asarray(left, float)
    x0 = resolve_init(meas, left, N)
    if spec["kind"] == "consistent":
        right = compose(x0[-1] if N else left, meas[N])
    else:
        rel = measurements(c["anchor_left"], [c["anchor_right"]])[0]
        rel[4:7] += 0.01 * np.random.RandomState(spec["seed"]).randn(3)
        right = compose(left, rel)
        if spec["kind"] == "closure":
            j = spec["jump"]
            right = np.concatenate([right[0:3] + np.asarray(j[0:3], float), qmul(right[3:7], rot_q([0.3, -0.5, 0.8], j[3]))])
    g = dict(spec=spec, case=c, meas=meas, left=left, right=right)
    g["poses"], g["summary"] = resolve_restated(g)
    return g


def resolve_restated(g, ulp=False):
    meas, left, right = (one_ulp_up(g[k]) for k in ("meas", "left", "right")) if ulp else (g["meas"], g["left"], g["right"])
    N = g["spec"]["n_frames"]
    poses, summ, _ = local_graph(meas, left, right, resolve_init(meas, left, N))
    return poses, summ


# ------------------------------------------------------------------ the branch cases: every trust-region branch and pass boundary the public API reaches
# (name, make_gap arguments, extras).  Extras: shift = the whole gap moved by that many metres (shifted()); anchor_right_x = that value put into
# anchor_right[0].  The seeds and jumps are the outcome of scripts/search_trajectory_branch_cases.py, pasted, not searched again here.
_J = dict(samples_per_segment=1)
BRANCH_SPECS = [
    # (a) a nominal gap at every size next to a pass boundary of evaluate() (nine poses per pass: 9 | 10, 18 | 19, 27 | 28)
    ("nominal_9", dict(seed=31, n_frames=9, **_J), {}),
    ("nominal_10", dict(seed=32, n_frames=10, **_J), {}),
    ("nominal_18", dict(seed=33, n_frames=18, **_J), {}),
    ("nominal_19", dict(seed=34, n_frames=19, **_J), {}),
    ("nominal_27", dict(seed=35, n_frames=27, **_J), {}),
    ("nominal_28", dict(seed=36, n_frames=28, **_J), {}),
    # (b) the Cauchy branch in every pass-count class (1, 2, 3, 4 passes)
    ("cauchy_1", dict(seed=300, n_frames=1, right_jump=(163000.0, 227300.0, -167600.0, 2.573), **_J), {}),
    ("cauchy_2", dict(seed=598, n_frames=2, right_jump=(-46310.0, -21370.0, -28030.0, 2.47), **_J), {}),
    ("cauchy_10", dict(seed=494, n_frames=10, right_jump=(13810.0, -41970.0, 9805.0, 0.8004), **_J), {}),
    ("cauchy_19", dict(seed=1080, n_frames=19, right_jump=(11160.0, 4850.0, -22690.0, 0.4011), **_J), {}),
    ("cauchy_32", dict(seed=1184, n_frames=32, right_jump=(12300.0, -19960.0, -817.3, 2.61), **_J), {}),
    # (b, c) the interpolated branch in every class; each of these takes all four radius rules
    ("interp_9", dict(seed=537, n_frames=9, right_jump=(-76.52, 619.9, 79.43, 1.682), **_J), {}),
    ("interp_10", dict(seed=580, n_frames=10, right_jump=(-625.3, -102.5, -1764.0, 1.538), **_J), {}),
    ("interp_18", dict(seed=486, n_frames=18, right_jump=(3.54, 16.95, -10.08, 2.048), **_J), {}),
    ("interp_18_far", dict(seed=334, n_frames=18, right_jump=(163.1, 780.3, 1086.0, 2.488), **_J), {}),
    ("interp_19", dict(seed=527, n_frames=19, right_jump=(-325.5, -43.89, -340.4, 3.01), **_J), {}),
    ("interp_27", dict(seed=366, n_frames=27, right_jump=(974.2, 254.4, -161.2, 2.822), **_J), {}),
    ("interp_28", dict(seed=547, n_frames=28, right_jump=(-7982.0, 3485.0, 4378.0, 0.6273), **_J), {}),
    ("interp_32", dict(seed=415, n_frames=32, right_jump=(-0.5151, -6.051, -9.648, 0.9572), **_J), {}),
    # a FUNCTION_TOLERANCE end after eight iterations over two passes, one step kept
    ("function_tol_18", dict(seed=217, n_frames=18, right_jump=(-1.294, -0.3379, -0.8139, 1.244), **_J), {}),
    # (d) PARAMETER_TOLERANCE, the normal end in UTM-like coordinates: at iteration 1 (1e7 m) and at iteration 2 (1e5 m)
    ("parameter_tol_3_at_1", dict(seed=40, n_frames=3, **_J), dict(shift=1e7)),
    ("parameter_tol_3_at_2", dict(seed=40, n_frames=3, **_J), dict(shift=1e5)),
    ("parameter_tol_18_at_2", dict(seed=40, n_frames=18, **_J), dict(shift=1e5)),
    ("parameter_tol_19_at_1", dict(seed=40, n_frames=19, **_J), dict(shift=1e7)),
    # GRADIENT_TOLERANCE through a push: one frame has no between factor, so anchors on the dead-reckoned ends satisfy both factors
    ("gradient_tol_1", dict(seed=50, n_frames=1, anchor_noise=(0.0, 0.0), **_J), {}),
    # (e) FAILURE at entry: the first cost overflows
    ("failure_at_entry_3", dict(seed=51, n_frames=3, **_J), dict(anchor_right_x=1e160)),
]
REQUIRED_CENSUS = dict(dogleg=set(DOGLEG_BRANCHES), rules=set(RADIUS_RULES),
                       ends={np_ceres.FUNCTION_TOL, np_ceres.NO_CONVERGENCE, np_ceres.PARAMETER_TOL, np_ceres.GRADIENT_TOL, np_ceres.FAILURE})
# (name of a branch case, max_iterations): glio_traj_create takes 0 .. 32.  At 1 a gap whose first step is the Cauchy step and one whose first is the
# Gauss-Newton step; at 32 a gap that is still NO_CONVERGENCE with its 32nd step accepted (bit 31 of accepted_mask; 21 of the 32 accepted).
LIMIT_SPECS = [("nominal_10", 0), ("cauchy_1", 1), ("nominal_9", 1), ("interp_18_far", 32)]


def build_gap(kw, extra):
    c = make_gap(**kw)
    if "shift" in extra:
        c = shifted(c, extra["shift"])
    if "anchor_right_x" in extra:
        c["anchor_right"] = np.array(c["anchor_right"], float)
        c["anchor_right"][0] = extra["anchor_right_x"]
    return c


def pass_class(N):
    """how many passes evaluate() makes, as a class 0 .. 3: N <= 9, 10 .. 18, 19 .. 27, 28 .. 32"""
    return (max(N, 1) - 1) // 9


def _judged_case(name, c, max_iterations):
    res = restate(c, max_iterations)
    assert_margins(name, res[3])
    floor, gate = noise_floor(name, lambda: restate(gap_one_ulp_up(c), max_iterations)[2:4], res[2:4])
    return dict(name=name, gap=c, max_iterations=max_iterations, restated=res, floor=floor, gate=gate)


_BRANCH_CASES = _LIMIT_CASES = _RESOLVE_CASES = None


def branch_cases():
    """[dict(name, gap, max_iterations, restated = (rows, meas, sol, summary, branches), floor, gate)]: computed once, shared, left unchanged.  Every case
    holds assert_margins and the one-ulp condition (noise_floor: the same decisions with every input one ulp up, and a floor of at most 1e-7); `gate` is
    what the device is held to on that case, max(1e-9, 100 floor).

    What the list reaches (tests/test_trajectory_restated.py asserts the union): the three branches of the traditional dogleg -- gn, cauchy and interp with
    c > 0 -- in each pass-count class; the four radius rules on gaps of more than one pass; the ends FUNCTION_TOLERANCE, NO_CONVERGENCE,
    PARAMETER_TOLERANCE, GRADIENT_TOLERANCE and FAILURE (at entry).

    NOT reachable through the public API, so nobody need hunt for them:
      * interp with c <= 0.  c = -alpha g.gn - alpha^2 |g|^2, and -g.gn = g' B^-1 g >= alpha |g|^2 by Cauchy-Schwarz for the positive definite model
        B = Hs + mu D^2 (alpha = |g|^2 / g' Hs g), so c >= 0, with equality only where the Gauss-Newton and the Cauchy step coincide -- and there the
        Gauss-Newton condition or the Cauchy condition has taken the step already.
      * the escalation of mu after a failed Cholesky, and FAILURE after five invalid steps: the model is J'J plus a positive diagonal (the clamp keeps D^2 at
        1e-6 or more), its factorisation does not fail and its model cost change is positive.
      * MIN_RADIUS: the radius starts at 1e4 and halves per rejection, 1e-32 is about 120 consecutive rejections away, and max_iterations is at most 32.
      * a non-finite candidate cost (a rejection without a judgement): the inputs that overflow the cost overflow it at entry."""
    global _BRANCH_CASES
    if _BRANCH_CASES is None:
        _BRANCH_CASES = [_judged_case(name, build_gap(kw, extra), 15) for name, kw, extra in BRANCH_SPECS]
    return _BRANCH_CASES


def limit_cases():
    """the gaps of LIMIT_SPECS solved with their own max_iterations: the same dicts as branch_cases()"""
    global _LIMIT_CASES
    if _LIMIT_CASES is None:
        by_name = {b["name"]: b for b in branch_cases()}
        _LIMIT_CASES = [_judged_case(f"{name}_limit_{m}", by_name[name]["gap"], m) for name, m in LIMIT_SPECS]
    return _LIMIT_CASES


# gaps of one resolve, in the store's order; keyframe row k + 1 is gap k's right row, so every gap's left row is what the gaps before it made of row 0.
# The closures' seeds and jumps come from `scripts/search_trajectory_branch_cases.py resolve`: tens of metres and up to 2.5 rad reach the interpolated
# branch; the Cauchy branch needs 1e4 m and more (below that the Gauss-Newton step stays inside the initial radius of 1e4 long enough), so the last two
# gaps, which no later gap's left row depends on, are that far.
RESOLVE_SPECS = [
    dict(seed=500, n_frames=0, kind="consistent"),
    dict(seed=501, n_frames=1, kind="consistent"),
    dict(seed=86, n_frames=9, kind="closure", jump=(12.1, -5.427, -24.74, 0.8312)),
    dict(seed=503, n_frames=10, kind="disturbed"),
    dict(seed=264, n_frames=18, kind="closure", jump=(2.838, 5.398, -15.9, 2.204)),
    dict(seed=114, n_frames=19, kind="closure", jump=(1.459, -17.13, 5.307, 0.8358)),
    dict(seed=506, n_frames=27, kind="consistent"),
    dict(seed=198, n_frames=28, kind="closure", jump=(-20.46, 5.521, -6.808, 2.127)),
    dict(seed=348, n_frames=32, kind="closure", jump=(-3.724, 7.73, -7.525, 1.895)),
    dict(seed=509, n_frames=32, kind="disturbed"),
    dict(seed=510, n_frames=9, kind="consistent"),
    dict(seed=811, n_frames=19, kind="disturbed"),
    dict(seed=512, n_frames=0, kind="disturbed"),
    dict(seed=513, n_frames=32, kind="consistent"),
    dict(seed=514, n_frames=28, kind="disturbed"),
    dict(seed=515, n_frames=1, kind="disturbed"),
    dict(seed=29, n_frames=1, kind="closure", jump=(81520.0, 130100.0, 130300.0, 0.4317)),
    dict(seed=3073, n_frames=18, kind="closure", jump=(7289.0, -27680.0, -3232.0, 0.8988)),
]


def resolve_cases():
    """(gaps, keyframe rows [len(gaps) + 1][7]): resolve_gap() of RESOLVE_SPECS chained from one left row, each with its margins asserted and its `floor`
    and `gate` (noise_floor with measurements and both rows one ulp up); computed once, shared, left unchanged"""
    global _RESOLVE_CASES
    if _RESOLVE_CASES is None:
        kf, gaps = [np.array([0.3, -0.2, 0.1, 1.0, 0.0, 0.0, 0.0])], []
        for k, spec in enumerate(RESOLVE_SPECS):
            g = resolve_gap(spec, kf[-1])
            name = f"resolve {k} ({spec['kind']}, {spec['n_frames']} frames)"
            assert_margins(name, g["summary"])
            g["name"] = name
            g["floor"], g["gate"] = noise_floor(name, lambda: resolve_restated(g, ulp=True), (g["poses"], g["summary"]))
            gaps.append(g)
            kf.append(g["right"])
        _RESOLVE_CASES = (gaps, np.array(kf))
    return _RESOLVE_CASES

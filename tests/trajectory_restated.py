"""A numpy restatement of the every-frame trajectory (include/glio_traj.h), written from the reference's lines: the IMU fill-in between two keyframes
(GLIO/src/Estimator.cpp:4279-4493), the relative measurements (:4494-4555) and optimizeLocalGraph (:3452-3527) with the factors of
LidarPoseFactor.h:11-52, 128-221.  Scalar loops in Eigen's evaluation order for the recurrence; tests/np_ceres.py::minimize for the trust-region loop.
Pose rows are t[3], q[4] (w first); measurement rows dq[4] (w first), dp[3].  `cases()` is the case builder the CPU and the GPU tests share."""
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


def local_graph(meas, left, right, x0, max_iterations=15):
    """optimizeLocalGraph: returns (poses [N][7], summary, trace); summary carries accepted_mask (bit k: iteration k + 1 accepted) and `verdicts`,
    per iteration (accepted, step quality or None, the function-tolerance ratio at a terminating iteration or None)"""
    x0 = np.asarray(x0, float).reshape(-1, 7)
    if len(x0) == 0:
        return x0, dict(termination=NOT_SOLVED, iterations=0, successful_steps=0, initial_cost=0.0, final_cost=0.0, accepted_mask=0, qualities=[]), []
    lg = LocalGraph(meas, left, right)
    trace = []
    x, summ, hist = np_ceres.minimize(x0, lg.evaluate, lg.plus, lg.flat, np_ceres.Options(**dict(OPTIONS, max_iterations=max_iterations)), trace=trace)
    mask, qualities = 0, []
    for k, row in enumerate(trace):               # one row per judged iteration (no invalid steps arise here: asserted by the case builder)
        if row["ratio"] > 1e-3:
            mask |= 1 << k
        qualities.append(float(row["ratio"]))
    summ = dict(summ, accepted_mask=mask, qualities=qualities, hist=hist)
    return np.asarray(x, float).reshape(-1, 7), summ, trace


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


FUNCTION_TOLERANCE, MIN_RELATIVE_DECREASE = 1e-6, 1e-3


def assert_margins(name, summ):
    """The conditions the GPU comparison relies on: every decision of the restated loop is away from its knife edge.
      * the step quality of every judged iteration is not within 0.05 of 0.25, 0.75 or min_relative_decrease;
      * at a FUNCTION_TOLERANCE end the ratio |cost change| / cost is not within a factor 2 of the tolerance; at a NO_CONVERGENCE end no iteration's
        ratio was within a factor 2 of it either; GRADIENT_TOLERANCE ends only arise here with an exactly consistent chain (gradient 0)."""
    for q in summ["qualities"]:
        for edge in (0.25, 0.75, MIN_RELATIVE_DECREASE):
            assert abs(q - edge) > 0.05, (name, "step quality", q, "near", edge)
    ended = summ["termination"] in (np_ceres.FUNCTION_TOL, np_ceres.PARAMETER_TOL)
    assert len(summ["qualities"]) == summ["iterations"] - (1 if ended else 0), (name, "an invalid step arose")
    cur = summ["initial_cost"]
    hist = summ["hist"]
    k = 0
    for ccost, radius, dx in hist:
        ratio = abs(cur - ccost) / cur if cur > 0 else 0.0
        last = k == len(hist) - 1 and summ["termination"] == np_ceres.FUNCTION_TOL
        if last:
            assert ratio < 0.5 * FUNCTION_TOLERANCE, (name, "terminating ratio", ratio)
        else:
            assert ratio > 2.0 * FUNCTION_TOLERANCE, (name, "ratio", ratio, "iteration", k + 1)
            if summ["qualities"][k] > MIN_RELATIVE_DECREASE:
                cur = ccost
        k += 1
    assert summ["termination"] in (np_ceres.FUNCTION_TOL, np_ceres.NO_CONVERGENCE, np_ceres.GRADIENT_TOL), (name, summ["termination"])


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

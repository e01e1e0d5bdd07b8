"""CPU restatement of Preprocessing::cloudHandler (reference GLIO/src/Preprocessing.cpp:353-681) -- TEST INFRASTRUCTURE ONLY, the checker of
glio_features_*.  Every step cites the line it restates.

Rounding follows the reference's build: float arithmetic where the reference has float operands (numpy float32 element-wise + - * /, which
round like scalar code), the reference's own libm for atan2f / atanf / sqrtf (ctypes on libm.so.6, not numpy's float32 ufuncs, which may
dispatch to SIMD implementations with other rounding), math.acos / math.sin for the double slerp, Eigen's operation order for slerp, the
quaternion product, inverse() and q * v (as glio_device.h restates them), and the reference's float/double promotions (thresholds are doubles).
Deviation: ties of the unstable std::sort by curvature (:553-554) are ordered by (curvature, index), as DESIGN.md §2 does for kd-tree ties.
"""
import ctypes
import math
import sys

import numpy as np

_M = ctypes.CDLL("libm.so.6")
for _f in ("atan2f", "atanf", "sqrtf"):
    getattr(_M, _f).restype = ctypes.c_float
_M.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_M.atanf.argtypes = [ctypes.c_float]
_M.sqrtf.argtypes = [ctypes.c_float]
F = np.float32
DBL_EPS = sys.float_info.epsilon


def atan2f(y, x):
    return F(_M.atan2f(float(y), float(x)))


def _vec(fn, *a):
    return np.array([fn(*v) for v in zip(*[x.tolist() for x in a])], np.float32)


def survivors(xyz, min_range=3.0):
    """removeNaNFromPointCloud (x y z finite) + removeClosedPointCloud (:144-168, :396-397): order kept, float x*x + y*y + z*z < thres*thres drops"""
    x, y, z = (np.asarray(xyz[:, k], np.float32) for k in range(3))
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    thr = F(min_range)
    with np.errstate(invalid="ignore", over="ignore"):
        close = (x * x + y * y + z * z) < thr * thr
    return np.nonzero(fin & ~close)[0]


def scan_ids(p, n_scans):
    """:430-488 -- angle = atan(z / sqrt(x*x + y*y)) * 180 / M_PI (sqrtf, atanf, float product, double quotient stored as float); -1 = dropped"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    s = _vec(_M.sqrtf, x * x + y * y)
    at = _vec(_M.atanf, z / s)
    angle = ((at * F(180)).astype(np.float64) / math.pi).astype(np.float32)
    a64 = angle.astype(np.float64)
    if n_scans == 16:
        sid = np.trunc(((angle + F(15)) / F(2)).astype(np.float64) + 0.5).astype(np.int64)
        bad = (sid > 15) | (sid < 0)
    elif n_scans == 32:
        sid = np.trunc((a64 + 92.0 / 3.0) * 3.0 / 4.0).astype(np.int64)
        bad = (sid > 31) | (sid < 0)
    elif n_scans == 64:
        up = np.trunc((F(2) - angle).astype(np.float64) * 3.0 + 0.5)
        low = 32 + np.trunc((-8.83 - a64) * 2.0 + 0.5)
        sid = np.where(a64 >= -8.83, up, low).astype(np.int64)
        bad = (a64 > 2) | (a64 < -24.33) | (sid > 50) | (sid < 0)
    else:
        raise ValueError(n_scans)
    return np.where(bad, -1, sid), angle


def _qmul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def _qinv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]                # Quaternion::inverse(): conjugate / squaredNorm
    return (q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)


def _qrot(q, v):
    uv = [q[2] * v[2] - q[3] * v[1], q[3] * v[0] - q[1] * v[2], q[1] * v[1] - q[2] * v[0]]
    uv = [u + u for u in uv]
    uuv = [q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]]
    return [v[k] + q[0] * uv[k] + uuv[k] for k in range(3)]


def undistort(p, inten, q_imu, q_lb):
    """undistortion (:176-200): dt_i = intensity - int(intensity) (a FLOAT difference), ratio = dt_i / 0.1 capped at 1, Eigen's slerp from the
    identity (linear branch at |d| >= 1 - epsilon), q_lb * q_si * q_lb.inverse(), q * v in double, stored as float"""
    qw, qx, qy, qz = (float(v) for v in q_imu)
    d = 0.0 * qx + 0.0 * qy + 0.0 * qz + 1.0 * qw
    ad = abs(d)
    ql = tuple(float(v) for v in q_lb)
    qi = _qinv(ql)
    out = np.zeros((len(p), 3), np.float32)
    for i in range(len(p)):
        f = F(inten[i])
        line = int(f)
        t = float(F(f - F(line))) / 0.1
        if t >= 1.0:
            t = 1.0
        if ad >= 1.0 - DBL_EPS:
            s0, s1 = 1.0 - t, t
        else:
            th = math.acos(ad)
            sth = math.sin(th)
            s0 = math.sin((1.0 - t) * th) / sth
            s1 = math.sin(t * th) / sth
        if d < 0.0:
            s1 = -s1
        qs = (s0 * 1.0 + s1 * qw, s0 * 0.0 + s1 * qx, s0 * 0.0 + s1 * qy, s0 * 0.0 + s1 * qz)
        qf = _qmul(_qmul(ql, qs), qi)
        out[i] = _qrot(qf, [float(p[i, 0]), float(p[i, 1]), float(p[i, 2])])
    return out


def _dist(values, const):
    """smallest |value - const| in radians (inf over nothing): how far a comparison is from going the other way"""
    v = np.abs(np.asarray(values, np.float64) - const)
    return float(v.min()) if v.size else math.inf


def _project(raw, n_scans, q_imu, q_lb, min_range):
    """project() and orientation_report() in one pass: the masks that pick every orientation are the ones the report counts"""
    raw = np.asarray(raw, np.float32)
    keep = survivors(raw[:, :3], min_range)
    p = raw[keep, :3]
    ns = len(p)
    if ns == 0:
        return (np.zeros((0, 4), np.float32), np.zeros(n_scans, int), np.zeros(n_scans, int), 0, np.zeros(0, int)), None
    start = -atan2f(p[0, 1], p[0, 0])                                                 # :401
    end = F(float(-atan2f(p[-1, 1], p[-1, 0])) + 2 * math.pi)                         # :402-404
    span0 = float(end - start)
    end_minus = span0 > 3 * math.pi                                                   # :406-410
    end_plus = not end_minus and span0 < math.pi
    if end_minus:
        end = F(float(end) - 2 * math.pi)
    elif end_plus:
        end = F(float(end) + 2 * math.pi)
    sid, _ = scan_ids(p, n_scans)
    ori_raw = -_vec(_M.atan2f, p[:, 1], p[:, 0])                                      # :489
    o64 = ori_raw.astype(np.float64)
    f_lo = o64 < float(start) - math.pi / 2                                           # :491
    f_hi = ~f_lo & (o64 > float(start) + math.pi * 3 / 2)                             # :493
    first = np.where(f_lo, (o64 + 2 * math.pi).astype(np.float32), np.where(f_hi, (o64 - 2 * math.pi).astype(np.float32), ori_raw))
    valid = sid >= 0
    turn = (first - start).astype(np.float64)
    flip = np.nonzero(valid & (turn > math.pi))[0]                                    # halfPassed (:496-497): the first valid point that sets it
    half = flip[0] if len(flip) else ns
    sec = (o64 + 2 * math.pi).astype(np.float32)                                      # :500-504
    s64 = sec.astype(np.float64)
    s_lo = s64 < float(end) - math.pi * 3 / 2                                         # :501
    s_hi = ~s_lo & (s64 > float(end) + math.pi / 2)                                   # :503
    sec = np.where(s_lo, (s64 + 2 * math.pi).astype(np.float32), np.where(s_hi, (s64 - 2 * math.pi).astype(np.float32), sec))
    in_first = np.arange(ns) <= half                                                  # the point that sets halfPassed is still on the first branch
    ori = np.where(in_first, first, sec)
    rel = (ori - start) / (end - start)                                               # :507
    inten = (sid.astype(np.float64) + 0.1 * rel.astype(np.float64)).astype(np.float32)   # :509
    vi = np.nonzero(valid)[0]
    und = undistort(p[vi], inten[vi], q_imu, q_lb)
    pts = np.concatenate([und, inten[vi, None]], 1)
    order = np.argsort(sid[vi], kind="stable")                                        # laserCloudScans[scanID].push_back, concatenated (:514, :522-526)
    cut = np.ascontiguousarray(pts[order])
    size = np.bincount(sid[vi], minlength=n_scans)[:n_scans]
    rstart = np.concatenate([[0], np.cumsum(size)[:-1]])
    a, b = valid & in_first, valid & ~in_first                                        # the points whose comparisons decide an output
    margin = min(_dist([span0], 3 * math.pi), _dist([span0], math.pi),
                 _dist(o64[a], float(start) - math.pi / 2), _dist(o64[a], float(start) + math.pi * 3 / 2), _dist(turn[a], math.pi),
                 _dist(s64[b], float(end) - math.pi * 3 / 2), _dist(s64[b], float(end) + math.pi / 2))
    report = {"start": float(start), "end": float(end), "end_minus": bool(end_minus), "end_plus": bool(end_plus),
              "n491": int((a & f_lo).sum()), "n493": int((a & f_hi).sum()), "n501": int((b & s_lo).sum()), "n503": int((b & s_hi).sum()),
              "half_passed": bool(len(flip)), "half": int(half), "rel_min": float(rel[valid].min()) if len(vi) else math.nan,
              "rel_max": float(rel[valid].max()) if len(vi) else math.nan, "margin": margin, "rel": rel[vi].copy(), "ring": sid[vi].copy()}
    return (cut, rstart, size, ns, sid), report


def project(raw, n_scans=32, q_imu=(1.0, 0, 0, 0), q_lb=(1.0, 0, 0, 0), min_range=3.0):
    """Steps 1-3: survivors, startOri / endOri, scanID, orientation, relTime, intensity, undistortion, the stable ring bucketing (:396-526).
    Returns (cut [n][4] float32, ring_start[n_scans], ring_size[n_scans], kept, ring of every survivor (-1 dropped))."""
    return _project(raw, n_scans, q_imu, q_lb, min_range)[0]


def orientation_report(raw, n_scans=32, min_range=3.0):
    """What the orientation state machine (:401-410, :489-507) did on this scan, from the pass that project() is: end_minus / end_plus (:406 / :409
    fired), n491 / n493 / n501 / n503 (valid points that took each adjustment), half_passed and the index of the survivor that set it (the number
    of survivors if none did), rel_min / rel_max, start / end, rel and ring of every valid survivor in raw order, and margin: the smallest
    distance in radians between a compared quantity and its constant -- endOri - startOri before its adjustment against 3 pi and pi, the raw ori
    of every valid first-branch point against startOri - pi/2 and startOri + 3 pi/2 and its ori - startOri against pi, ori + 2 pi of every
    valid second-branch point against endOri - 3 pi/2 and endOri + pi/2.  A scan whose margin is far above an ulp of atan2f (2.4e-7 near pi)
    takes the same branches with any atan2f.  None for a scan without survivors."""
    return _project(raw, n_scans, (1.0, 0, 0, 0), (1.0, 0, 0, 0), min_range)[1]


def voxel_grid(pts, leaf):
    """pcl::VoxelGrid as oracle/orc_assoc.c defines it, plus PCL's overflow rule: (int64)((max - min) * inv) + 1 per axis, a product above
    INT32_MAX passes the cloud through unfiltered"""
    from oracle import pyoracle as po
    pts = np.ascontiguousarray(pts, np.float32)
    if len(pts) == 0:
        return pts.reshape(0, 4)
    inv = F(1.0) / F(leaf)
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    d = [int(F(mx[k] - mn[k]) * inv) + 1 for k in range(3)]
    if d[0] * d[1] * d[2] > 2 ** 31 - 1:
        return pts.copy()
    return po.voxel_grid(pts, leaf)[0]


def curvature(cut):
    """:529-538 over the concatenated cloud, i in [5, n - 6]: float sums left to right, 10 * x a float product"""
    n = len(cut)
    c = np.zeros(n, np.float32)
    if n < 11:
        return c
    i = np.arange(5, n - 5)
    d = []
    for k in range(3):
        v = cut[:, k]
        s = v[i - 5] + v[i - 4]
        s = s + v[i - 3]
        s = s + v[i - 2]
        s = s + v[i - 1]
        s = s - F(10) * v[i]
        for l in range(1, 6):
            s = s + v[i + l]
        d.append(s)
    c[i] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    return c


def _near(p):
    return float(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) < 0.25                    # :603, :641 (float sum, double comparison)


def _mark(cut, picked, ind):
    for l in range(1, 6):                                                              # :579-586
        d = cut[ind + l, :3] - cut[ind + l - 1, :3]
        if float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > 0.05:
            break
        picked[ind + l] = 1
    for l in range(-1, -6, -1):                                                        # :587-596
        d = cut[ind + l, :3] - cut[ind + l + 1, :3]
        if float(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) > 0.05:
            break
        picked[ind + l] = 1


def select(cut, rstart, rsize, ds_rate=1, edge_threshold=1.0, surf_threshold=0.1, ds_leaf=0.4):
    """Steps 4-6 (:522-654) from the cut cloud and its rings.  Returns dict sharp, less_sharp, flat, surf ([n][4] float32) and labels."""
    cut = np.asarray(cut, np.float32)
    n = len(cut)
    curv = curvature(cut)
    picked = np.zeros(n, np.int8)
    label = np.zeros(n, np.int8)
    sharp, less_sharp, flat, surf = [], [], [], []
    for r in range(len(rsize)):
        S, E = int(rstart[r]) + 5, int(rstart[r]) + int(rsize[r]) - 6                  # scanStartInd / scanEndInd (:522-526)
        if E - S < 6 or r % ds_rate != 0:                                              # :542
            continue
        lf = []
        for j in range(6):
            sp = S + (E - S) * j // 6                                                  # :550-551 (non-negative: floor = C truncation)
            ep = S + (E - S) * (j + 1) // 6 - 1
            idx = np.arange(sp, ep + 1)
            order = idx[np.lexsort((idx, curv[idx]))]                                   # std::sort by curvature, ties by index
            largest = 0
            for ind in order[::-1]:                                                    # :557-598
                if picked[ind] == 0 and float(curv[ind]) > edge_threshold:
                    largest += 1
                    if largest <= 2:
                        label[ind] = 2
                        sharp.append(cut[ind]); less_sharp.append(cut[ind])
                    elif largest <= 10:
                        label[ind] = 1
                        less_sharp.append(cut[ind])
                    else:
                        break
                    picked[ind] = 1
                    _mark(cut, picked, ind)
            smallest = 0
            for ind in order:                                                          # :600-637
                if _near(cut[ind]):
                    continue
                if picked[ind] == 0 and float(curv[ind]) < surf_threshold:
                    label[ind] = -1
                    flat.append(cut[ind])
                    smallest += 1
                    if smallest >= 4:
                        break
                    picked[ind] = 1
                    _mark(cut, picked, ind)
            for k in range(sp, ep + 1):                                                # :639-645
                if not _near(cut[k]) and label[k] <= 0:
                    lf.append(cut[k])
        surf.append(voxel_grid(np.array(lf, np.float32).reshape(-1, 4), ds_leaf))      # :648-654
    arr = lambda a: np.array(a, np.float32).reshape(-1, 4)
    return {"sharp": arr(sharp), "less_sharp": arr(less_sharp), "flat": arr(flat),
            "surf": np.concatenate(surf).astype(np.float32) if surf else np.zeros((0, 4), np.float32), "label": label, "curv": curv}


def rings_of_cut(cut, n_scans):
    """ring boundaries of a cut cloud from its intensities (scanID + 0.1 relTime, relTime within [-0.5, 1.5]: the nearest integer)"""
    rid = np.rint(np.asarray(cut)[:, 3].astype(np.float64)).astype(int)
    size = np.bincount(rid, minlength=n_scans)[:n_scans]
    return np.concatenate([[0], np.cumsum(size)[:-1]]), size


def extract(raw, n_scans=32, q_imu=(1.0, 0, 0, 0), ds_rate=1, edge_threshold=1.0, surf_threshold=0.1, ds_leaf=0.4, q_lb=(1.0, 0, 0, 0), min_range=3.0):
    """the whole cloudHandler per scan"""
    cut, rstart, size, kept, _ = project(raw, n_scans, q_imu, q_lb, min_range)
    out = select(cut, rstart, size, ds_rate, edge_threshold, surf_threshold, ds_leaf)
    out.update(cut=cut, kept=kept, ring_start=rstart, ring_size=size)
    return out

"""The cases the static map's tests share (CPU: tests/test_static_map_restated.py; GPU: tests/test_hip_static_map.py, tests/test_hip_static_map_e2e.py).

mini_cases()   two-frame calls on a 4 x 8 image (cols_per_quadrant = 2, rows of 20 degrees) whose answers follow from how they are built: frame 0 is a view
               with one point in the middle of every cell, frame 1 holds the probes.  Each deliberate mistake of static_map_restated.WRONG changes the answer
               of at least one of them.
street()       the end-to-end scene: a street between two walls closed by a building, a car-sized box that crosses it ahead of the sensor, 8 scans
               of 16 lines x 225 azimuths from a sensor that drives along; with the labels (which points lie on the box)."""
import numpy as np

import static_map_restated as R

F32 = np.float32
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def mini_params(**kw):
    d = dict(rows=4, cols_per_quadrant=2, neighbourhood=1, min_votes=1, elev_min_deg=-40.0, elev_max_deg=40.0, min_range=0.5, max_range=100.0, range_gain=1.0,
             range_margin=0.0)
    d.update(kw)
    return d


def cell_point(P, row, col, rng_m, frac=(0.5, 0.5)):
    """a point at range rng_m in cell (row, col), frac of the way across it in elevation and azimuth"""
    e = np.deg2rad(P.elev_min_deg + (P.elev_max_deg - P.elev_min_deg) * (row + frac[0]) / P.rows)
    a = 2.0 * np.pi * (col + frac[1]) / P.cols
    return [rng_m * np.cos(e) * np.cos(a), rng_m * np.cos(e) * np.sin(a), rng_m * np.sin(e)]


def grid_cloud(P, ranges):
    """one point in the middle of every cell with ranges[row][col] > 0, row major; intensity = the cell index"""
    pts = [cell_point(P, r, c, ranges[r][c]) + [r * P.cols + c] for r in range(P.rows) for c in range(P.cols) if ranges[r][c] > 0]
    return np.array(pts, np.float64).astype(F32)


def probes(P, rows):
    """probe points [(row, col, range)] -> cloud; intensity = 100 + index"""
    return np.array([cell_point(P, r, c, d, (0.4, 0.6)) + [100 + i] for i, (r, c, d) in enumerate(rows)], np.float64).astype(F32)


def mini_cases():
    """-> list of dict(name, opts (glio_static_opts fields), clouds [2], poses [2][7], view_offsets, views, dynamic: expected flags of frame 1's points)"""
    P = R.Params(**mini_params())
    full = np.full((P.rows, P.cols), 10.0)
    out = []

    def case(name, ranges, extra, probe_rows, dynamic, **okw):
        view = grid_cloud(P, ranges)
        if len(extra):
            view = np.vstack([view, np.array(extra, np.float64).astype(F32)])
        out.append(dict(name=name, opts=mini_params(**okw), clouds=[np.ascontiguousarray(view), probes(P, probe_rows)], poses=np.array([IDENTITY, IDENTITY]),
                        view_offsets=np.array([0, 0, 1], np.int32), views=np.array([0], np.int32), dynamic=np.array(dynamic, bool)))

    # everything at 10 m, the probe at 7 m in a middle row: every neighbour is farther -> seen through; the same in an edge row is never tested
    case("plain", full, [], [(1, 3, 7.0), (2, 6, 7.0), (1, 4, 12.0)], [True, True, False])
    case("edge_rows", full, [], [(0, 3, 7.0), (3, 5, 7.0), (2, 2, 7.0)], [False, False, True])
    # a neighbour cell at 5 m blocks the probe in the cell beside it
    near = full.copy(); near[1, 2] = 5.0
    case("floor", near, [], [(1, 3, 7.0), (2, 1, 7.0), (2, 6, 7.0)], [False, False, True])
    # the blocking neighbour lies across the seam between the last and the first column, either way
    seam7 = full.copy(); seam7[2, 7] = 5.0
    case("wrap_low", seam7, [], [(2, 0, 7.0), (1, 4, 7.0)], [False, True])
    seam0 = full.copy(); seam0[1, 0] = 5.0
    case("wrap_high", seam0, [], [(1, 7, 7.0), (2, 4, 7.0)], [False, True])
    # two points in one cell: the nearer one counts
    case("two_in_cell", full, [cell_point(P, 2, 5, 5.0, (0.3, 0.3)) + [77]], [(2, 5, 7.0), (1, 1, 7.0)], [False, True])
    # an empty neighbour: nothing is known in that direction
    hole = full.copy(); hole[2, 3] = 0.0
    case("empty_neighbour", hole, [], [(1, 2, 7.0), (1, 6, 7.0)], [False, True])
    # nb = 0: the cell alone decides
    case("nb0", near, [], [(1, 3, 7.0), (1, 2, 7.0), (0, 3, 7.0)], [True, False, True], neighbourhood=0)
    # the knife edge of rule 4: with gain 1 and margin 0 a probe that IS the nearest point of its neighbourhood meets F == r2' exactly -> no vote
    ke = full.copy(); ke[1, 5] = 6.0
    view = grid_cloud(P, ke)
    at = view[1 * P.cols + 5].copy(); at[3] = 100
    pr = np.vstack([at[None, :], probes(P, [(2, 1, 7.0)])[0][None, :]]).astype(F32)
    out.append(dict(name="knife_edge", opts=mini_params(), clouds=[view, np.ascontiguousarray(pr)], poses=np.array([IDENTITY, IDENTITY]),
                    view_offsets=np.array([0, 0, 1], np.int32), views=np.array([0], np.int32), dynamic=np.array([False, True])))
    return out


def run_restated(case, wrong=None, tables=None, rel_fn=R.relative_pose):
    """the restatement's answer for a case: (per-frame results, images, Params)"""
    o = {k: v for k, v in case["opts"].items() if k not in ("max_views", "image_path")}
    P = R.Params(**o)
    s2, dirs = R.tables(P) if tables is None else tables
    rel = R.relative_poses(case["poses"], case["view_offsets"], case["views"], rel_fn)
    res, images = R.classify(case["clouds"], rel, case["view_offsets"], case["views"], s2, dirs, P, wrong)
    return res, images, P


KNIFE_POSE = np.array([1.0, 2.0, 0.3, np.cos(0.15), 0.02, -0.01, np.sin(0.15)])
KNIFE_FAR = np.array([1.0e6 + 1.0, -1.0e6 + 2.0, 0.3, np.cos(0.15), 0.02, -0.01, np.sin(0.15)])


def knife_case(ulps, rel_fn=R.relative_pose, far=False, **okw):
    """Rule 4 on its edge with the default gain and margin and a GENERAL relative pose: frame 1 holds one probe, frame 0 (its view) has a point in every cell at
    30 m except the probe's cell (1, 5), whose point is tuned -- its z moved by ulps until its float32 r2 is EXACTLY (g2 r2') + m2 (ulps = 0: no vote) or that
    many float32 steps above (ulps = 1: a vote).  rel_fn forms T(v, f): the tuning has to see the r2' that the code under test will see.  far: both poses
    1e6 m from the origin."""
    o = mini_params(range_gain=1.05, range_margin=0.3, **okw)
    P = R.Params(**o)
    s2, dirs = R.tables(P)
    pose_v = KNIFE_FAR.copy() if far else IDENTITY.copy()
    pose_f = (KNIFE_FAR + np.array([1.5, -0.7, 0.2, 0.01, 0.03, 0.0, -0.02])) if far else KNIFE_POSE
    want = np.array(cell_point(P, 1, 5, 7.0))                          # where the probe lies, in the view's frame
    Td = R.relative_pose(pose_f, pose_v, np.float64)                   # view -> frame, double
    probe = np.r_[Td[:, :3] @ want + Td[:, 3], 100.0].astype(F32)[None, :]
    T = rel_fn(pose_v, pose_f)
    c, r2 = R.cells(R.transform(probe[:, :3], T), s2, dirs, P)
    assert c[0] == 1 * P.cols + 5
    target = (P.g2 * r2[0]) + P.m2
    for _ in range(int(ulps)):
        target = np.nextafter(target, F32(np.inf))
    ranges = np.full((P.rows, P.cols), 30.0)
    view = grid_cloud(P, ranges)
    i = 1 * P.cols + 5
    view[i, :3] = np.array(cell_point(P, 1, 5, float(np.sqrt(np.float64(target))))).astype(F32)
    for _ in range(100000):
        got = ((view[i, 0] * view[i, 0]) + (view[i, 1] * view[i, 1])) + (view[i, 2] * view[i, 2])
        if got == target:
            break
        view[i, 2] = np.nextafter(view[i, 2], F32(-np.inf) if got < target else F32(0))      # (z < 0: away from zero lengthens)
    assert got == target and R.cells(view[i:i + 1, :3], s2, dirs, P)[0][0] == i
    return dict(name="knife_%d%s" % (ulps, "_far" if far else ""), opts=o, clouds=[np.ascontiguousarray(view), np.ascontiguousarray(probe)],
                poses=np.array([pose_v, pose_f]), view_offsets=np.array([0, 0, 1], np.int32), views=np.array([0], np.int32), dynamic=np.array([ulps > 0]))


# ---------------------------------------------------------------- the street
STREET_FRAMES, STREET_LINES, STREET_AZIMUTHS = 8, 16, 225
SENSOR_HEIGHT, WALL_Y, END_X, WALL_TOP = 1.8, 10.0, 60.0, 6.0
BOX_SIZE = (1.8, 4.5, 1.5)                 # a car that crosses the street: width along x, length along y, height
HALF_WINDOW = 3


def _ray_box(o, d, lo, hi):
    """slab test for rays o [3], d [n][3] against the box [lo, hi]: the entry distance, inf when missed"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    return np.where((tn <= tf) & (tn > 0), tn, np.inf)


def street_poses():
    """the sensor drives along x at 1 m per frame with a little sway and yaw: poses [8][7] (t, q)"""
    p = []
    for f in range(STREET_FRAMES):
        yaw = 0.02 * np.sin(0.9 * f)
        p.append([1.0 * f, -1.5 + 0.1 * np.cos(0.7 * f), SENSOR_HEIGHT, np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])
    return np.array(p)


def box_at(f):
    """the box at frame f: it crosses the street 18 m down the road at 2 m per frame -> (lo, hi) world corners"""
    cx, cy = 18.0, -7.0 + 2.0 * f
    lo = np.array([cx - BOX_SIZE[0] / 2, cy - BOX_SIZE[1] / 2, 0.0])
    return lo, lo + np.array(BOX_SIZE)


def street(offset=(0.0, 0.0, 0.0)):
    """-> clouds [8] ([n][4] float32, LiDAR frame, intensity = the line), poses [8][7], on_box [8] (bool per point).  `offset` moves the whole world (and the
    poses with it): the clouds do not change."""
    poses = street_poses()
    el = np.deg2rad(-15.5 + np.arange(STREET_LINES))                      # 1 degree apart, in the middle of the default image's rows
    clouds, labels = [], []
    for f in range(STREET_FRAMES):
        az = np.deg2rad(-90.0 + 0.8 * (np.arange(STREET_AZIMUTHS) + 0.5) + 0.05 * np.sin(1.3 * f))     # the front half, 0.8 degrees apart
        E, A = np.meshgrid(el, az, indexing="ij")
        dl = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
        Rw = R.rotation(poses[f, 3:])
        o, d = poses[f, :3], dl @ Rw.T
        with np.errstate(divide="ignore", invalid="ignore"):
            t_ground = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)
            t_left = np.where(d[:, 1] > 0, (WALL_Y - o[1]) / d[:, 1], np.inf)
            t_right = np.where(d[:, 1] < 0, (-WALL_Y - o[1]) / d[:, 1], np.inf)
            t_end = np.where(d[:, 0] > 0, (END_X - o[0]) / d[:, 0], np.inf)
        for t in (t_left, t_right, t_end):
            z = o[2] + t * d[:, 2]
            t[~((z >= 0) & (z <= WALL_TOP))] = np.inf
        t_box = _ray_box(o, d, *box_at(f))
        t = np.minimum.reduce([t_ground, t_left, t_right, t_end, t_box])
        hit = np.isfinite(t) & (t < 79.0)
        pts = dl[hit] * t[hit, None]
        line = np.repeat(np.arange(STREET_LINES), STREET_AZIMUTHS)[hit]
        clouds.append(np.ascontiguousarray(np.c_[pts, line].astype(F32)))
        labels.append((t_box[hit] == t[hit]))
    poses = poses.copy()
    poses[:, :3] += np.asarray(offset, np.float64)
    return clouds, poses, labels


def street_call(poses):
    off, views = R.static_views(poses, HALF_WINDOW, 0.5)
    return off, views

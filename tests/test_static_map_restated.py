"""CPU: the numpy restatement of the static map's rules (tests/static_map_restated.py) held to independent statements of the same thing -- the two bisections
against float64 arctan2, the library's tables and relative poses against numpy's double values to one float ulp (no device needed), the cases of
tests/static_map_cases.py against the answers they were built to have, each deliberate mistake refused by them, and the end-to-end scene's conditions."""
import numpy as np
import pytest

import static_map_cases as Cs
import static_map_restated as R

F32 = np.float32


def ulp_diff(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F32)).astype(np.float64)


@pytest.mark.parametrize("kw", [dict(), Cs.mini_params(), dict(rows=7, cols_per_quadrant=5, elev_min_deg=-25.0, elev_max_deg=3.0),
                                dict(rows=64, cols_per_quadrant=256, elev_min_deg=-60.0, elev_max_deg=60.0)])
def test_the_bisections_against_arctan2(kw):
    """points at least 1e-3 rad from every row and column edge land where float64 arctan2 puts them; points outside the elevation range are skipped"""
    P = R.Params(**kw)
    s2, dirs = R.tables(P)
    rng = np.random.default_rng(3)
    n = 20000
    az = rng.uniform(0.0, 2 * np.pi, n)
    el = np.deg2rad(rng.uniform(P.elev_min_deg - 8.0, P.elev_max_deg + 8.0, n))
    r = rng.uniform(2.0, 70.0, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F32)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    az64 = np.arctan2(y, x) % (2 * np.pi)
    el64 = np.arctan2(z, np.hypot(x, y))
    fc, fr = az64 / (2 * np.pi / P.cols), (el64 - np.deg2rad(P.elev_min_deg)) / (np.deg2rad(P.elev_max_deg - P.elev_min_deg) / P.rows)
    clear = (np.abs(fc - np.round(fc)) * (2 * np.pi / P.cols) >= 1e-3) & (np.abs(fr - np.round(fr)) * (np.deg2rad(P.elev_max_deg - P.elev_min_deg) / P.rows) >= 1e-3)
    inside = (fr >= 0) & (fr < P.rows)
    want = np.where(inside, np.floor(fr).astype(np.int64) * P.cols + np.floor(fc).astype(np.int64) % P.cols, -1)
    got, r2 = R.cells(xyz, s2, dirs, P)
    assert clear.sum() > n // 2 and (want[clear] >= 0).sum() > n // 4 and (want[clear] < 0).sum() > 100
    assert np.array_equal(got[clear], want[clear])
    assert np.allclose(r2, x * x + y * y + z * z, rtol=3e-7)


def test_the_special_points():
    P = R.Params(**Cs.mini_params())
    s2, dirs = R.tables(P)
    pts = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0],                     # the axes open the quadrants 0, 1, 2, 3
                    [0, 0, 5], [0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [1, 1, -np.inf],      # rho2 == 0, non-finite
                    [0.5, 0, 0], [0.4999, 0, 0], [100, 0, 0], [99.99, 0, 0],                    # r2 == min2 kept, below skipped, r2 == max2 skipped, below kept
                    [3, 3, 0], [3, 3, -1e-3]], F32)                                              # z = 0 sits on the edge between rows 1 and 2: it belongs to row 2
    c, _ = R.cells(pts, s2, dirs, P)
    assert list(c[:4]) == [2 * 8 + 0, 2 * 8 + 2, 2 * 8 + 4, 2 * 8 + 6]
    assert list(c[4:9]) == [-1] * 5
    assert list(c[9:13]) == [16, -1, -1, 16]
    assert list(c[13:]) == [2 * 8 + 1, 1 * 8 + 1] or list(c[13:]) == [2 * 8 + 0, 1 * 8 + 0]       # (45 degrees is a column edge: either side of float rounding)


def test_the_library_tables_are_numpys_to_one_ulp():
    from glio_amd import capi
    for kw in (dict(), Cs.mini_params(), dict(rows=7, cols_per_quadrant=5, elev_min_deg=-25.0, elev_max_deg=3.0), dict(rows=256, cols_per_quadrant=512)):
        P = R.Params(**kw)
        fields = {k: v for k, v in kw.items() if k in ("rows", "cols_per_quadrant", "elev_min_deg", "elev_max_deg")}
        s2, dirs = capi.static_tables(capi.static_opts(**fields))
        want_s2, want_d = R.tables(P)
        assert s2.shape == want_s2.shape and dirs.shape == want_d.shape
        assert ulp_diff(s2, want_s2).max() <= 1.0
        assert np.abs(dirs.astype(np.float64) - want_d).max() <= 2.0 ** -24           # one ulp of a value of magnitude <= 1 (near a zero the relative gap is void)
        assert np.all(np.diff(s2.astype(np.float64)) > 0)


def random_pose(rng, scale):
    q = rng.normal(size=4)
    return np.r_[rng.uniform(-scale, scale, 3), q * rng.uniform(0.5, 2.0)]


@pytest.mark.parametrize("scale,base", [(30.0, 0.0), (30.0, 1.0e6)])
def test_the_library_relative_pose_is_numpys_to_one_ulp(scale, base):
    """the positions' difference is taken in double: 1e6 m from the origin the pair's relative pose is as good as at the origin"""
    from glio_amd import capi
    rng = np.random.default_rng(11)
    for _ in range(200):
        pv, pf = random_pose(rng, scale), random_pose(rng, scale)
        pv[:3] += base; pf[:3] += base
        got, want = capi.static_relative_pose(pv, pf), R.relative_pose(pv, pf, np.float64)
        assert got.dtype == F32 and got.shape == (3, 4)
        # one float ulp of the entry, or of 1 for the rotation's entries near zero (their double values come from cancelling sums of magnitude 1)
        tol = np.spacing(np.maximum(np.abs(want), np.c_[np.ones((3, 3)), np.zeros(3)]).astype(F32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want) <= tol), (pv, pf)
    ident = capi.static_relative_pose(Cs.IDENTITY, Cs.IDENTITY)
    assert np.array_equal(ident, np.eye(3, 4, dtype=F32))


CASES = Cs.mini_cases() + [Cs.knife_case(0), Cs.knife_case(1), Cs.knife_case(0, far=True), Cs.knife_case(1, far=True)]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_cases_have_the_answers_they_were_built_to_have(case):
    res, images, P = Cs.run_restated(case)
    assert np.array_equal(res[1]["dynamic"], case["dynamic"])
    assert np.array_equal(res[1]["kept"], case["clouds"][1][~case["dynamic"]])
    assert np.array_equal(res[0]["kept"], case["clouds"][0]) and not res[0]["tested"].any()            # a frame without a view is copied whole
    raw, fl = images[0]
    assert raw.shape == (P.rows, P.cols) and np.array_equal(fl, R.floor_image(raw, P))                  # the vectorised floor is the loop's
    if P.nb == 1:
        assert not fl[0].any() and not fl[-1].any()


@pytest.mark.parametrize("wrong", R.WRONG)
def test_each_deliberate_mistake_is_refused_by_the_cases(wrong):
    refused = []
    for case in CASES:
        res, images, P = Cs.run_restated(case, wrong)
        ok = np.array_equal(res[1]["dynamic"], case["dynamic"]) and np.array_equal(res[1]["kept"], case["clouds"][1][~case["dynamic"]])
        if not ok:
            refused.append(case["name"])
        assert np.array_equal(images[0][1], R.floor_image(images[0][0], P, wrong))
    assert refused, wrong


def test_static_views():
    from glio_amd import static_map
    rng = np.random.default_rng(5)
    poses = np.c_[np.cumsum(rng.choice([0.0, 0.3, 1.0], 30))[:, None] * np.array([[1.0, 0.2, 0.0]]), np.tile([1.0, 0, 0, 0], (30, 1))]
    for hw, mb in ((1, 0.5), (3, 0.5), (6, 1.2), (3, 0.0)):
        off, views = static_map.static_views(poses, hw, mb)
        want_off, want_views = R.static_views(poses, hw, mb)
        assert np.array_equal(off, want_off) and np.array_equal(views, want_views)
        for f in range(30):
            v = views[off[f]:off[f + 1]]
            assert f not in v and len(v) <= 2 * hw and len(set(v)) == len(v)
            assert all(np.linalg.norm(poses[j, :3] - poses[f, :3]) >= mb for j in v)
    off, views = static_map.static_views(np.tile(Cs.IDENTITY, (5, 1)), 3)          # a stationary vehicle gives no parallax: no views
    assert not off.any() and len(views) == 0


@pytest.fixture(scope="module")
def street():
    clouds, poses, labels = Cs.street()
    off, views = Cs.street_call(poses)
    P = R.Params()
    s2, dirs = R.tables(P)
    res, _ = R.classify(clouds, R.relative_poses(poses, off, views), off, views, s2, dirs, P)
    return clouds, labels, off, res


def test_the_street_with_default_options(street):
    """the caps of the end-to-end scene: at most 0.1 % of the static points removed, at least half of the box's points in every frame with >= 4 views"""
    clouds, labels, off, res = street
    assert len(clouds) == Cs.STREET_FRAMES and all(1000 < len(c) <= Cs.STREET_LINES * Cs.STREET_AZIMUTHS for c in clouds)
    n_static = sum(int((~l).sum()) for l in labels)
    lost = sum(int((r["dynamic"] & ~l).sum()) for r, l in zip(res, labels))
    print("static points removed: %d of %d" % (lost, n_static))
    assert lost <= 0.001 * n_static
    seen = 0
    for f, (r, l) in enumerate(zip(res, labels)):
        nv = off[f + 1] - off[f]
        print("frame %d: %d views, %d of %d box points removed" % (f, nv, int((r["dynamic"] & l).sum()), int(l.sum())))
        if nv >= 4:
            seen += 1
            assert l.sum() >= 50 and (r["dynamic"] & l).sum() >= 0.5 * l.sum(), f
    assert seen >= 4


def test_the_street_does_not_sit_on_the_knife_edge_of_rule_4(street):
    """no decision of the scene changes when the bound of rule 4 moves by a part in 10^4 either way"""
    clouds, poses, labels = Cs.street()
    off, views = Cs.street_call(poses)
    rel = R.relative_poses(poses, off, views)
    for gain in (1.05 * (1 - 1e-4), 1.05 * (1 + 1e-4)):
        P = R.Params(range_gain=gain)
        s2, dirs = R.tables(P)
        res, _ = R.classify(clouds, rel, off, views, s2, dirs, P)
        for a, b in zip(res, street[3]):
            assert np.array_equal(a["dynamic"], b["dynamic"])


def test_without_the_floor_the_ground_goes(street):
    """why neighbourhood 1 is the default: with the cell alone more than 1 % of the static points are voted out"""
    clouds, poses, labels = Cs.street()
    off, views = Cs.street_call(poses)
    P = R.Params(neighbourhood=0)
    s2, dirs = R.tables(P)
    res, _ = R.classify(clouds, R.relative_poses(poses, off, views), off, views, s2, dirs, P)
    lost = sum(int((r["dynamic"] & ~l).sum()) for r, l in zip(res, labels))
    assert lost > 0.01 * sum(int((~l).sum()) for l in labels)

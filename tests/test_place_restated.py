"""CPU: the numpy restatement of the place-recognition rules (tests/place_restated.py) held against an independent, textbook Scan Context, against the
rotation property the column shift rests on, and the library's two host tables (glio_place_tables, no device) against numpy's."""
import numpy as np
import pytest

import place_restated as R

MAX_RADIUS, LIDAR_HEIGHT = 80.0, 2.0
EPS32 = 2.0 ** -24                     # float32's unit roundoff


def polar_cloud(seed, n, edge_margin=0.15):
    """n points whose polar coordinates stay away from every ring and sector edge by `edge_margin` of a bin: a rotation by k * 6 deg cannot move one across"""
    rng = np.random.default_rng(seed)
    ring = rng.integers(0, R.RINGS, n)
    sector = rng.integers(0, R.SECTORS, n)
    r = (ring + rng.uniform(edge_margin, 1 - edge_margin, n)) * (MAX_RADIUS / R.RINGS)
    th = (sector + rng.uniform(edge_margin, 1 - edge_margin, n)) * (2 * np.pi / R.SECTORS)
    z = rng.uniform(-3.0, 6.0, n)
    return np.stack([r * np.cos(th), r * np.sin(th), z, np.zeros(n)], axis=1), ring, sector


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_binning_against_a_textbook_scan_context(seed):
    rb2, dirs = R.tables(MAX_RADIUS)
    rng = np.random.default_rng(seed)
    pts = np.c_[rng.uniform(-90, 90, (4000, 2)), rng.uniform(-3, 6, 4000), np.zeros(4000)].astype(np.float32)
    kept, ring, sector, _ = R.cells(pts, rb2, dirs)
    _, nring, nsector, nkeep = R.naive_scan_context(pts, MAX_RADIUS, LIDAR_HEIGHT)
    # away from the bin edges (1 mm radially, 1e-5 rad in angle) the two agree point by point
    r = np.hypot(pts[:, 0].astype(float), pts[:, 1].astype(float))
    th = np.mod(np.arctan2(pts[:, 1].astype(float), pts[:, 0].astype(float)), 2 * np.pi)
    fr, fs = np.mod(r, MAX_RADIUS / R.RINGS), np.mod(th, 2 * np.pi / R.SECTORS)
    clear = (np.minimum(fr, MAX_RADIUS / R.RINGS - fr) > 1e-3) & (np.minimum(fs, 2 * np.pi / R.SECTORS - fs) > 1e-5)
    assert clear.sum() > 3500
    assert np.array_equal(kept[clear], nkeep[clear])
    both = clear & kept
    assert both.sum() > 2000 and np.array_equal(ring[both], nring[both]) and np.array_equal(sector[both], nsector[both])
    # ... and so do the descriptors of the cloud without its edge points (a float add against a double add: half an ulp)
    h, mask = R.descriptor(pts[clear], rb2, dirs, LIDAR_HEIGHT)
    hn = R.naive_scan_context(pts[clear], MAX_RADIUS, LIDAR_HEIGHT)[0]
    assert np.all(np.abs(h - hn) <= 2 * EPS32 * np.abs(hn)) and h.dtype == np.float32
    assert mask == sum(1 << s for s in range(R.SECTORS) if np.any(sector[both] == s))


def test_the_special_points():
    rb2, dirs = R.tables(MAX_RADIUS)
    pts = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, -1, 0, 0],            # on the axes: sectors 0, 15, 30, 45
                    [0, 0, 5, 0], [np.nan, 1, 1, 0], [1, np.inf, 1, 0], [1, 1, -np.inf, 0],  # origin and non-finite: skipped
                    [4, 0, 1, 0], [80, 0, 1, 0], [79.99, 0, -7, 0]], np.float32)            # r2 == rb2[1] -> ring 1; r2 == rb2[20] -> skipped; a negative value
    kept, ring, sector, _ = R.cells(pts, rb2, dirs)
    assert list(kept) == [True] * 4 + [False] * 4 + [True, False, True]
    assert list(sector[:4]) == [0, 15, 30, 45] and list(ring[:4]) == [0, 0, 0, 0] and ring[8] == 1 and ring[10] == 19
    h, mask = R.descriptor(pts, rb2, dirs, LIDAR_HEIGHT)
    assert mask == (1 | 1 << 15 | 1 << 30 | 1 << 45)
    assert h[1, 0] == np.float32(3) and h[19, 0] == np.float32(-5) and h[0, 0] == np.float32(2) and h[5, 5] == 0 and not np.signbit(h[5, 5])
    # a value of -0 is stored as +0
    h0, _ = R.descriptor(np.array([[1, 0, -2, 0]], np.float32), rb2, dirs, LIDAR_HEIGHT)
    assert h0[0, 0] == 0 and not np.signbit(h0[0, 0])


@pytest.mark.parametrize("k", [0, 1, 7, 30, 59])
def test_a_rotation_by_k_sectors_shifts_the_columns_by_k(k):
    """the candidate's cloud is the query's cloud turned by +k * 6 deg: its descriptor is the query's rolled by k columns, and the pair's shift is k"""
    rb2, dirs = R.tables(MAX_RADIUS)
    pts, _, _ = polar_cloud(11, 3000)
    a = k * 2 * np.pi / R.SECTORS
    rot = pts.copy()
    rot[:, 0] = np.cos(a) * pts[:, 0] - np.sin(a) * pts[:, 1]
    rot[:, 1] = np.sin(a) * pts[:, 0] + np.cos(a) * pts[:, 1]
    hq, mq = R.descriptor(pts.astype(np.float32), rb2, dirs, LIDAR_HEIGHT)
    hc, mc = R.descriptor(rot.astype(np.float32), rb2, dirs, LIDAR_HEIGHT)
    assert np.array_equal(hc, np.roll(hq, k, axis=1))
    assert mc == R.rotated_mask(mq, (R.SECTORS - k) % R.SECTORS)
    uq, pq = R.unit_columns(hq, mq)
    uc, pc = R.unit_columns(hc, mc)
    d, s = R.pair(uq, pq, uc, pc)
    assert s == k and abs(float(d)) <= 64 * EPS32
    assert R.pair(uc, pc, uq, pq)[1] == (R.SECTORS - k) % R.SECTORS
    assert abs(float(R.yaw_of_shift(s)) - a) <= 4 * EPS32 * max(a, 1.0)
    # the fp64 twin: the same shift, a distance within the float32 rounding of a 20-term dot product and a 60-term mean
    d64, s64 = R.pair(uq, pq, uc, pc, np.float64)
    assert s64 == k and abs(float(d) - float(d64)) <= 32 * EPS32


def test_levelling_takes_a_tilt_out():
    """a cloud seen by a sensor rolled by 0.2 rad, levelled with the roll's quaternion, has the level cloud's descriptor away from the bin edges"""
    rb2, dirs = R.tables(MAX_RADIUS)
    pts, _, _ = polar_cloud(5, 1500, edge_margin=0.3)
    c, s = np.cos(0.2), np.sin(0.2)
    Rx = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    tilted = pts.copy()
    tilted[:, :3] = pts[:, :3] @ Rx                              # p_sensor = Rx^T p_level
    q = [np.cos(0.1), np.sin(0.1), 0.0, 0.0]
    h, m = R.descriptor(tilted.astype(np.float32), rb2, dirs, LIDAR_HEIGHT, q)
    h0, m0 = R.descriptor(pts.astype(np.float32), rb2, dirs, LIDAR_HEIGHT)
    assert m == m0 and np.abs(h - h0).max() < 1e-4


def test_distance_rules():
    rb2, dirs = R.tables(MAX_RADIUS)
    pts, _, _ = polar_cloud(3, 2000)
    h, m = R.descriptor(pts.astype(np.float32), rb2, dirs, LIDAR_HEIGHT)
    u, pm = R.unit_columns(h, m)
    # no common column at any shift: exactly 1, shift 0
    d, s = R.pair(u, pm, np.zeros_like(u), 0)
    assert d == np.float32(1) and s == 0
    # 60 identical columns: every shift ties, the lowest wins
    hi = np.repeat(h[:, :1] + np.float32(1), R.SECTORS, axis=1)
    ui, pi = R.unit_columns(hi, R.MASK60)
    assert pi == R.MASK60 and R.pair(ui, pi, ui, pi)[1] == 0
    # a column whose heights are all zero is absent although it holds points
    hz = h.copy(); hz[:, 4] = 0
    assert (R.unit_columns(hz, m | 1 << 4)[1] >> 4) & 1 == 0
    # absent columns leave the count, not only the sum
    hm = h.copy(); mm = m & ~0xff
    um, pmm = R.unit_columns(hm, mm)
    assert np.all(um[:, :8] == 0) and abs(float(R.pair(um, pmm, u, pm)[0])) <= 64 * EPS32


def test_the_library_tables_are_numpys_to_one_ulp():
    from glio_amd import build, capi
    build.build()
    for radius in (80.0, 33.3, 120.0):
        rb2, dirs = capi.place_tables(radius)
        want_rb2, want_dirs = R.tables(radius)
        assert rb2.dtype == np.float32 and dirs.shape == (R.SECTORS, 2)
        assert np.array_equal(rb2, want_rb2) and rb2[0] == 0 and rb2[20] == np.float32(np.float32(radius).astype(np.float64) ** 2)
        assert np.abs(dirs.view(np.int32).astype(np.int64) - want_dirs.view(np.int32).astype(np.int64))[np.abs(want_dirs) > 1e-6].max() <= 1
        assert np.abs(dirs - want_dirs).max() <= 1e-7          # (the four axis entries near zero: absolute; the binning never reads them)
    lib = capi.load()
    import ctypes as C
    assert lib.glio_place_tables(0.0, C.cast(0, C.POINTER(C.c_float)), C.cast(0, C.POINTER(C.c_float))) == capi.E_ARG
    assert lib.glio_place_tables(float("nan"), rb2.ctypes.data_as(C.POINTER(C.c_float)), dirs.ctypes.data_as(C.POINTER(C.c_float))) == capi.E_ARG

"""GPU: place recognition on the device (glio_place_*, include/glio_place.h).  The descriptor bit for bit against the numpy restatement
(tests/place_restated.py) on the smallest clouds that can go wrong; the query against the restatement at the gate of tests/place_cases.py, shift and place
exact on cases vetted on the CPU; the invariances the header promises; the refusals, which leave the store byte-equal."""
import numpy as np
import pytest

import place_cases as Cs
import place_restated as R

pytestmark = pytest.mark.gpu

CAP = 300                              # points per resident frame: more than one pass of the 256-thread workgroup
K_FRAMES = 8
MAX_RADIUS, LIDAR_HEIGHT = 80.0, 2.0


@pytest.fixture(scope="module")
def tables():
    from glio_amd import capi
    rb2, dirs = capi.place_tables(MAX_RADIUS)
    want = R.tables(MAX_RADIUS)
    assert np.array_equal(rb2, want[0]) and np.abs(dirs - want[1]).max() <= 1e-7
    return rb2, dirs


@pytest.fixture(scope="module")
def owner():
    from glio_amd import batch
    ba = batch.BatchAssociation(K_FRAMES, CAP, 16)
    yield ba
    ba.close()


@pytest.fixture()
def pr(owner):
    from glio_amd import place
    p = place.PlaceRecognition(owner, max_places=64)
    yield p
    p.close()


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(-90, 90, (n, 2)), rng.uniform(-6, 6, n), rng.uniform(0, 255, n)].astype(np.float32)


def special_cloud():
    """points on the axes, exactly on ring edges (r2 == rb2[k] for k = 1, 7, 19) and on the outer edge (r2 == rb2[20]: skipped), at the origin, non-finite,
    with a negative z + lidar_height, on a sector edge direction, and two in one cell"""
    p = [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [3, 0, -9], [0, 3, 4], [4, 0, 1], [0, 28, 1], [-76, 0, 1], [80, 0, 1], [0, -80, 1], [0, 0, 5], [0, 0, 0],
         [np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf], [10, 10, -2], [10, 10.01, -2.5], [-20, 5, -7.25],
         [np.cos(np.float32(0.1)) * 30, np.sin(np.float32(0.1)) * 30, 0.5], [5, -60, 2], [56.5, 56.5, 1], [56.6, 56.6, 1]]
    return np.c_[np.array(p, np.float32), np.zeros(len(p), np.float32)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def store_bytes(p, places):
    out = []
    for k in places:
        h, m, t, v = p.read_descriptor(k)
        out.append((h.tobytes(), m, t, v))
    return out


TILT = [np.cos(0.06), np.sin(0.06) * 0.6, np.sin(0.06) * -0.8, 0.0]


@pytest.mark.parametrize("name,cloud,level_q", [
    ("n1", random_cloud(1, 1)[:1] * np.float32(0.5), None), ("n63", random_cloud(63, 2), None), ("n64", random_cloud(64, 3), None), ("n65", random_cloud(65, 4), None),
    ("cap", random_cloud(CAP, 5), None), ("cap_levelled", random_cloud(CAP, 6), TILT), ("special", special_cloud(), None), ("special_levelled", special_cloud(), TILT),
    ("all_out_of_range", random_cloud(70, 7) * np.float32(100) + np.float32(9000), None)])
def test_descriptor_bit_for_bit(owner, pr, tables, name, cloud, level_q):
    owner.set_frame(2, cloud)
    pr.add_frames([2], [5], [12.5], None if level_q is None else [level_q])
    h, mask, t, valid = pr.read_descriptor(5)
    want_h, want_mask = R.descriptor(cloud, tables[0], tables[1], LIDAR_HEIGHT, level_q)
    assert valid and t == 12.5 and mask == want_mask
    assert np.array_equal(bits(h), bits(want_h)), (name, np.argwhere(bits(h) != bits(want_h))[:5])
    if name == "all_out_of_range":
        assert mask == 0 and not h.any()
    if name.startswith("special"):
        assert np.any(h < 0) and (level_q is not None or mask == want_mask != 0)
    # an untouched place reads as invalid zeros
    h9, m9, t9, v9 = pr.read_descriptor(9)
    assert not v9 and m9 == 0 and t9 == 0 and not h9.any()


def test_one_launch_for_many_frames_gives_the_same_bytes(owner, pr, tables):
    clouds = [random_cloud(n, 20 + n) for n in (1, 64, 129, CAP, 7)]
    for k, c in enumerate(clouds):
        owner.set_frame(k, c)
    lq = [TILT, [1, 0, 0, 0], TILT, [0.5, 0, 0, 0.5], [1, 0.01, 0, 0]]
    pr.add_frames([0, 1, 2, 3, 4], [10, 3, 7, 0, 63], [1.0, 2.0, 3.0, 4.0, 5.0], lq)
    many = store_bytes(pr, [10, 3, 7, 0, 63])
    pr.clear()
    assert not pr.read_descriptor(10)[3]
    for f, (k, p) in enumerate(zip([0, 1, 2, 3, 4], [10, 3, 7, 0, 63])):
        pr.add_frames([k], [p], [1.0 + f], [lq[f]])
    assert store_bytes(pr, [10, 3, 7, 0, 63]) == many
    for f, p in enumerate([10, 3, 7, 0, 63]):
        want_h, want_m = R.descriptor(clouds[f], tables[0], tables[1], LIDAR_HEIGHT, lq[f])
        assert many[f] == (want_h.tobytes(), want_m, 1.0 + f, True)


def test_refusals_leave_the_store_byte_equal(owner, pr):
    from glio_amd import capi
    owner.set_frame(0, random_cloud(50, 31)); owner.set_frame(1, random_cloud(60, 32)); owner.set_frame(7, np.zeros((0, 4), np.float32))
    pr.add_frames([0, 1], [0, 1], [1.0, 2.0])
    before = store_bytes(pr, range(4))
    ref = pr.query(0, 0.5, 2)
    nan = float("nan")
    for frames, places, times, lq in (([0, K_FRAMES], [2, 3], [1, 2], None), ([0, -1], [2, 3], [1, 2], None), ([0, 1], [2, 64], [1, 2], None), ([0, 1], [-1, 2], [1, 2], None),
                                      ([0, 7], [2, 3], [1, 2], None), ([0, 1], [2, 3], [1, nan], None), ([0, 1], [2, 3], [float("inf"), 2], None),
                                      ([0, 1], [2, 3], [1, 2], [[1, 0, 0, 0], [nan, 0, 0, 0]]), ([0, 1], [2, 3], [1, 2], [[1, 0, 0, 0], [0, 0, 0, 0]]),
                                      ([0, 1, 0], [2, 3, 2], [1, 2, 3], None), ([0, 1], [1, 1], [1, 2], None)):
        with pytest.raises(capi.GlioError):
            pr.add_frames(frames, places, times, lq)
        assert store_bytes(pr, range(4)) == before, (frames, places)
    h = np.ones((R.RINGS, R.SECTORS), np.float32)
    bad_h = h.copy(); bad_h[3, 3] = np.inf
    for place, hh, mask, t in ((64, h, 1, 0.0), (-1, h, 1, 0.0), (2, bad_h, 1, 0.0), (2, h, 1 << 60, 0.0), (2, h, 1, nan)):
        with pytest.raises(capi.GlioError):
            pr.set_descriptor(place, hh, mask, t)
        assert store_bytes(pr, range(4)) == before
    for args in ((2, 0.5, 1), (64, 0.5, 1), (0, 0.5, 0), (0, 0.5, 9), (0, -1.0, 1), (0, nan, 1)):
        with pytest.raises(capi.GlioError):
            pr.query(*args)
    with pytest.raises(capi.GlioError):
        pr.query_many(60, 5, 0.5)
    assert store_bytes(pr, range(4)) == before and pr.query(0, 0.5, 2).tobytes() == ref.tobytes()


def test_the_owner_may_overwrite_a_frame_right_after_add_frames(owner, pr, tables):
    first, second = random_cloud(CAP, 41), random_cloud(CAP, 42)
    owner.set_frame(3, first)
    pr.add_frames([3], [0], [1.0])
    owner.set_frame(3, second)                     # no host wait in between: the owner's write comes behind the read on the device
    h, m, _, _ = pr.read_descriptor(0)
    want_h, want_m = R.descriptor(first, tables[0], tables[1], LIDAR_HEIGHT)
    assert m == want_m and np.array_equal(bits(h), bits(want_h))
    pr.add_frames([3], [1], [2.0])
    h, m, _, _ = pr.read_descriptor(1)
    want_h, want_m = R.descriptor(second, tables[0], tables[1], LIDAR_HEIGHT)
    assert m == want_m and np.array_equal(bits(h), bits(want_h))


def test_on_a_dense_store(tables):
    from glio_amd import mapping, place
    rng = np.random.default_rng(51)
    cloud = np.c_[rng.uniform(-60, 60, (3000, 2)), rng.uniform(-2, 5, 3000), np.zeros(3000)].astype(np.float32)
    dense = mapping.DenseClouds(2, 4096, 4096)
    n = dense.set_frame(1, cloud, 0.4)
    p = place.PlaceRecognition(dense, max_places=4, max_radius=50.0, lidar_height=1.5)
    p.add_frames([1], [2], [3.0], [TILT])
    resident = dense.read_frame(1)
    assert len(resident) == n > 100
    rb2, dirs = R.tables(50.0)
    from glio_amd import capi
    lrb2, ldirs = capi.place_tables(50.0)
    assert np.array_equal(rb2, lrb2)
    want_h, want_m = R.descriptor(resident, lrb2, ldirs, 1.5, TILT)
    h, m, t, v = p.read_descriptor(2)
    assert v and t == 3.0 and m == want_m and np.array_equal(bits(h), bits(want_h)) and h.any()
    p.close(); dense.close()


# ---------------------------------------------------------------------------------------------- the query
BANKS = {"n15": (15, 1, ()), "n16": (16, 2, ()), "n17_gap": (17, 3, (5,)), "n33_gaps": (33, 4, (2, 9, 10))}
_vetted = {}


def vetted(name):
    """(entries, restated store, {query: top_k it is vetted at}) -- built once per bank and never changed"""
    if name not in _vetted:
        n, seed, gaps = BANKS[name]
        e = Cs.bank(n, seed, gaps)
        st = Cs.restated_store(e, e[-1][0] + 1)
        ok = {}
        for place, _, m, _ in e:
            if m != 0:
                ok[place] = next((k for k in (8, 4, 1) if Cs.separated(st, place, 1.5, k)), 0)
        _vetted[name] = (e, st, ok)
    return _vetted[name]


def load_bank(p, entries):
    for place, h, m, t in entries:
        p.set_descriptor(place, h, m, t)


def check_matches(got, want):
    """place and shift exact (the callers assert the separation that makes them so), the distance within the gate"""
    assert len(got) == len(want), (got, want)
    for g, (d, c, s) in zip(got, want):
        assert Cs.within_gate(g["distance"], d), (g, d, c, s)
        assert (int(g["place"]), int(g["shift"])) == (c, s), (g, d, c, s)
        assert g["yaw"] == R.yaw_of_shift(s)


def report():
    print(f"largest |device - restated| distance compared so far: {Cs.LARGEST['deviation']:.3e} (gate {Cs.GATE:.3e})")


@pytest.mark.parametrize("name", list(BANKS))
def test_query_against_the_restatement(pr, name):
    entries, st, ok = vetted(name)
    assert sum(1 for k in ok.values() if k >= 1) >= (2 * len(ok)) // 3 and sum(1 for k in ok.values() if k == 8) >= 3, ok
    load_bank(pr, entries)
    first, n = entries[0][0], entries[-1][0] + 1
    many = {k: pr.query_many(0, n, 1.5, False, k) for k in (8, 4, 1)}
    for q, k in ok.items():
        if k == 0:
            continue
        want = st.query(q, 1.5, k)
        got = pr.query(q, 1.5, k)
        check_matches(got, want)
        mm, nf = many[k]
        assert nf[q] == len(got) and mm[q, :nf[q]].tobytes() == got.tobytes()          # the two calls: bit for bit
    # invalid slots inside the range find nothing; the all-absent place is at exactly 1 from everything, in place order
    for g in BANKS[name][2]:
        assert many[8][1][g] == 0
    empty = next(p for p, _, m, _ in entries if m == 0)
    got = pr.query(empty, 1.5, 8)
    assert np.all(got["distance"] == np.float32(1)) and np.all(got["shift"] == 0) and list(got["place"]) == st.candidates(empty, 1.5)[:8]
    for q in list(ok)[:4]:
        full = pr.query(q, 1.5, 8)
        hit = full[full["place"] == empty]
        assert len(hit) == 0 or (hit["distance"][0] == np.float32(1) and hit["shift"][0] == 0)
    # earlier_only: the candidates are those with a smaller time
    q = max(p for p, k in ok.items() if k >= 1)
    got, nf = pr.query_many(q, 1, 1.5, True, 8)
    want = st.query(q, 1.5, 8, earlier_only=True)
    assert Cs.separated(st, q, 1.5, 8, True)
    assert nf[0] == len(want) and all(int(p) < q for p in got[0, :nf[0]]["place"])
    check_matches(got[0, :nf[0]], want)
    report()


def test_small_stores_and_the_time_gap(pr):
    entries, st, ok = vetted("n15")
    e0, e3 = entries[0], entries[3]
    pr.set_descriptor(e0[0], e0[1], e0[2], e0[3])
    assert len(pr.query(e0[0], 0.0, 8)) == 0                                   # a store of 1: nothing found
    pr.set_descriptor(e3[0], e3[1], e3[2], e3[3])
    got = pr.query(e3[0], 0.0, 8)                                             # a store of 2, top_k above the eligible places
    st2 = Cs.restated_store([e0, e3], e3[0] + 1)
    assert len(got) == 1 and Cs.separated(st2, e3[0], 0.0, 1)
    check_matches(got, st2.query(e3[0], 0.0, 8))
    assert len(pr.query(e3[0], 3.0, 8)) == 0 and len(pr.query(e3[0], 1e9, 1)) == 0          # |3 - 0| > 3 is false: everything excluded by the time gap
    assert len(pr.query(e3[0], 2.999, 8)) == 1
    mm, nf = pr.query_many(0, 64, 0.0, True, 2)
    assert list(np.flatnonzero(nf)) == [e3[0]] and nf[e3[0]] == 1 and mm[e3[0], 0]["place"] == e0[0]


@pytest.mark.parametrize("k", [0, 59, 1])
def test_a_descriptor_rolled_by_k_columns_is_found_at_shift_k(pr, k):
    """the candidate is the query's descriptor rolled by k columns (the cloud turned by +k sectors): distance 0 at shift k, for k = 0 and 59 too"""
    entries, _, _ = vetted("n15")
    h, m = entries[1][1], entries[1][2]                                       # (seven absent columns)
    assert m != R.MASK60
    hk, mk = np.roll(h, k, axis=1), R.rotated_mask(m, (R.SECTORS - k) % R.SECTORS)
    pr.set_descriptor(0, h, m, 0.0)
    pr.set_descriptor(1, hk, mk, 10.0)
    st = R.Store(2)
    st.set(0, h, m, 0.0); st.set(1, hk, mk, 10.0)
    assert Cs.separated(st, 0, 1.5, 1) and Cs.separated(st, 1, 1.5, 1)
    got = pr.query(0, 1.5, 1)
    check_matches(got, st.query(0, 1.5, 1))
    assert int(got[0]["shift"]) == k and abs(float(got[0]["distance"])) <= Cs.GATE
    back = pr.query(1, 1.5, 1)
    check_matches(back, st.query(1, 1.5, 1))
    assert int(back[0]["shift"]) == (R.SECTORS - k) % R.SECTORS
    report()


def test_exact_ties(pr):
    entries, st, ok = vetted("n16")
    h, m = entries[1][1], entries[1][2]
    q = entries[0]
    # two places set to identical bytes: the same distance bits, the lower index first
    pr.set_descriptor(0, q[1], q[2], 0.0)
    pr.set_descriptor(9, h, m, 10.0)
    pr.set_descriptor(4, h, m, 20.0)
    pr.set_descriptor(12, entries[2][1], entries[2][2], 30.0)
    got = pr.query(0, 1.5, 3)
    twins = got[np.isin(got["place"], (4, 9))]
    assert list(twins["place"]) == [4, 9] and twins["distance"][0] == twins["distance"][1] and twins["shift"][0] == twins["shift"][1]
    # a descriptor whose 60 columns are identical, against another such: every shift ties, shift 0
    pr.clear()
    col_a, col_b = q[1][:, :1] + np.float32(0.5), entries[2][1][:, 7:8] + np.float32(0.25)
    pr.set_descriptor(0, np.repeat(col_a, R.SECTORS, axis=1), R.MASK60, 0.0)
    pr.set_descriptor(1, np.repeat(col_b, R.SECTORS, axis=1), R.MASK60, 5.0)
    pr.set_descriptor(2, np.repeat(col_a, R.SECTORS, axis=1), R.MASK60, 9.0)
    got = pr.query(0, 1.5, 2)
    assert list(got["place"]) == [2, 1] and list(got["shift"]) == [0, 0] and abs(float(got["distance"][0])) <= Cs.GATE
    st3 = R.Store(3)
    for k, c, t in ((0, col_a, 0.0), (1, col_b, 5.0), (2, col_a, 9.0)):
        st3.set(k, np.repeat(c, R.SECTORS, axis=1), R.MASK60, t)
    check_matches(got, st3.query(0, 1.5, 2))
    report()


def test_a_pairs_bits_depend_on_the_two_descriptors_only(pr):
    entries, st, ok = vetted("n33_gaps")
    few = entries[:6]
    load_bank(pr, few)
    q = few[1][0]
    base = {int(g["place"]): g.tobytes() for g in pr.query(q, 1.5, 8)}
    assert len(base) >= 3
    q_last = few[-1][0]
    earlier = pr.query_many(q_last, 1, 1.5, True, 8)
    assert earlier[1][0] >= 3
    load_bank(pr, entries[6:])                                             # 27 more places, on both sides of the run length
    for top_k in (8, 5):
        full = pr.query(q, 1.5, top_k)
        again = pr.query(q, 1.5, top_k)
        assert full.tobytes() == again.tobytes()                             # run to run
        mm, nf = pr.query_many(0, entries[-1][0] + 1, 1.5, False, top_k)
        assert mm[q, :nf[q]].tobytes() == full.tobytes()
        hits = [g for g in full if int(g["place"]) in base]
        assert len(hits) >= 1 and all(g.tobytes() == base[int(g["place"])] for g in hits)
    # the places earlier than the small store's last are the same in both stores: the whole answer is unchanged
    again = pr.query_many(q_last, 1, 1.5, True, 8)
    assert again[1][0] == earlier[1][0] and again[0].tobytes() == earlier[0].tobytes()
    ms = pr.last_device_ms()
    assert 0 < ms < 1000

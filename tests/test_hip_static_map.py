"""GPU: the static map on the device (glio_static_*, include/glio_static.h).  Everything bit for bit against the numpy restatement
(tests/static_map_restated.py) fed with the library's own tables and relative poses: the raw and the floor image on the smallest clouds that can go wrong, the
votes with 1 .. 32 views at identity and general poses (one set 1e6 m from the origin), the knife edge of rule 4, the static frames, the invariances the header
promises, and the refusals, which leave store, counts and votes byte-equal."""
import numpy as np
import pytest

import static_map_cases as Cs
import static_map_restated as R

pytestmark = pytest.mark.gpu

CAP = 300                              # points per resident frame: more than one pass of a 256-thread workgroup
K_FRAMES = 8
F32 = np.float32
MID = dict(rows=6, cols_per_quadrant=3, elev_min_deg=-45.0, elev_max_deg=45.0, min_range=0.5, max_range=60.0)      # 6 x 12: 300 random points fill every cell


@pytest.fixture(scope="module")
def owner():
    from glio_amd import batch
    ba = batch.BatchAssociation(K_FRAMES, CAP, 16)
    yield ba
    ba.close()


def make(owner, kw):
    """a StaticClouds with the glio_static_opts fields kw, the restatement's Params and the LIBRARY's tables"""
    from glio_amd import capi, static_map
    st = static_map.StaticClouds(owner, **kw)
    P = R.Params(**{k: v for k, v in kw.items() if k not in ("max_views", "image_path")})
    tab = capi.static_tables(st.opts)
    want = R.tables(P)
    assert np.abs(tab[0].astype(np.float64) - want[0]).max() <= np.spacing(np.abs(want[0]).max()) and np.abs(tab[1] - want[1]).max() <= 2.0 ** -24
    return st, P, tab


def random_cloud(n, seed, lo=3.0, hi=40.0, el=50.0):
    rng = np.random.default_rng(seed)
    az, e, r = rng.uniform(0, 2 * np.pi, n), np.deg2rad(rng.uniform(-el, el, n)), rng.uniform(lo, hi, n)
    return np.c_[r * np.cos(e) * np.cos(az), r * np.cos(e) * np.sin(az), r * np.sin(e), rng.uniform(0, 255, n)].astype(F32)


def special_cloud():
    """for the 4 x 8 image of Cs.mini_params (rows of 20 degrees from -40, min_range 0.5, max_range 100): points on the axes and quadrant boundaries, exactly on
    a row edge (z = 0: s2[2] = 0) and on column-edge directions, at r2 == min_range^2 and r2 == max_range^2, at the origin and on the z axis, non-finite, two in
    one cell with tied r2, just outside and just inside the top and bottom rows, and on the 20 degree row edge as float32 has it"""
    t40, t20 = np.tan(np.deg2rad(40.0)), np.tan(np.deg2rad(20.0))
    p = [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [2, 0, 0.5], [0, 2, -0.5], [-2, 0, 0.3], [0, -2, -0.3], [3, 3, 0], [-3, 3, 1], [-3, -3, -1], [3, -3, 0.5],
         [0.5, 0, 0], [0.3, 0.4, 0], [0.49, 0, 0], [100, 0, 0], [60, 80, 0], [99.9, 0, 0], [0, 0, 5], [0, 0, -5], [0, 0, 0],
         [np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [1, 1, np.inf],
         [5, 2, 1], [5, 2, 1], [4, 1, 2], [10, 0, 10 * t40 * 1.001], [10, 0, 10 * t40 * 0.999], [0, -10, -10 * t40 * 1.001], [0, -10, -10 * t40 * 0.999],
         [10, 0, 10 * t20], [7, 7, -np.hypot(7, 7) * t20], [1e-20, 0, 0], [3e19, 0, 0], [-7, 2, 3], [6, -1, -4]]
    return np.c_[np.array(p, np.float64).astype(F32), np.arange(len(p), dtype=F32)]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def one_frame_call(st, k=2):
    return st.classify([k], [Cs.IDENTITY], [0, 0], [])


# ---------------------------------------------------------------------------------------------- the images
IMAGE_CLOUDS = [("n1", random_cloud(1, 1)), ("n63", random_cloud(63, 2)), ("n64", random_cloud(64, 3)), ("n65", random_cloud(65, 4)), ("n257", random_cloud(257, 5)),
                ("n300", random_cloud(CAP, 6)), ("special", special_cloud())]


@pytest.mark.parametrize("path", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("size", ["4x8", "6x12", "44x360"])
def test_raw_and_floor_image_bit_for_bit(owner, size, path):
    kw = dict(Cs.mini_params() if size == "4x8" else MID if size == "6x12" else {}, image_path=path)
    st, P, tab = make(owner, kw)
    for name, cloud in IMAGE_CLOUDS:
        for nb in ((1, 0) if name in ("n300", "special") else (1,)):
            if nb != P.nb:
                st.close()
                st, P, tab = make(owner, dict(kw, neighbourhood=nb))
            owner.set_frame(2, cloud)
            info = one_frame_call(st)
            assert info.lds_path == (path == 0) and info.n_points == len(cloud) and info.n_dynamic == 0 and info.n_tested == 0
            raw, fl = st.read_image(0)
            want_raw = R.raw_image(cloud, tab[0], tab[1], P)
            assert np.array_equal(bits(raw), bits(want_raw)), (name, np.argwhere(bits(raw) != bits(want_raw))[:5])
            assert np.array_equal(bits(fl), bits(R.floor_image_fast(want_raw, P))), name
            if size != "44x360":
                assert np.array_equal(bits(fl), bits(R.floor_image(want_raw, P)))
            if name == "special" and size == "4x8":
                assert np.count_nonzero(raw) >= 12 and not np.signbit(raw).any()
            assert np.array_equal(st.read_frame(2).view(np.uint32), cloud.view(np.uint32))         # no view: the frame is copied whole, NaNs and all
    st.close()


def run_case(owner, case, path=0):
    """a case of static_map_cases on the device, its frames in the owner's frames 0 .. n-1: (device result per frame, restated result, images, info)"""
    from glio_amd import capi
    st, P, tab = make(owner, dict(case["opts"], image_path=path))
    for k, c in enumerate(case["clouds"]):
        owner.set_frame(k, c)
    n = len(case["clouds"])
    info = st.classify(list(range(n)), case["poses"], case["view_offsets"], case["views"])
    want, images, _ = Cs.run_restated(case, None, tab, capi.static_relative_pose)
    got = []
    for k in range(n):
        th, te = st.read_votes(k)
        got.append(dict(through=th, tested=te, kept=st.read_frame(k), image=st.read_image(k)))
    st.close()
    return got, want, images, info


def assert_equal_to_restated(got, want, images, name=""):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["through"], w["through"]) and np.array_equal(g["tested"], w["tested"]), (name, k)
        assert g["kept"].shape == w["kept"].shape and np.array_equal(g["kept"].view(np.uint32), w["kept"].view(np.uint32)), (name, k)
        assert np.array_equal(bits(g["image"][0]), bits(images[k][0])) and np.array_equal(bits(g["image"][1]), bits(images[k][1])), (name, k)


MINI = Cs.mini_cases()


@pytest.mark.parametrize("path", [0, 1], ids=["lds", "global"])
@pytest.mark.parametrize("case", MINI, ids=[c["name"] for c in MINI])
def test_the_built_cases(owner, case, path):
    """column wrap at both ends, the top and the bottom row, an empty neighbour, two points in a cell, nb = 0, F == r2': the answers the cases were built to have"""
    got, want, images, info = run_case(owner, case, path)
    assert_equal_to_restated(got, want, images, case["name"])
    dyn = got[1]["through"] >= case["opts"]["min_votes"]
    assert np.array_equal(dyn, case["dynamic"])
    assert info.n_dynamic == int(case["dynamic"].sum()) and info.n_points == sum(len(c) for c in case["clouds"]) and info.n_frames == 2
    assert info.n_tested == int((got[1]["tested"] > 0).sum())


@pytest.mark.parametrize("far", [False, True], ids=["near", "1e6"])
@pytest.mark.parametrize("ulps", [0, 1])
def test_the_knife_edge_of_rule_4(owner, ulps, far):
    """F == (g2 r2') + m2 exactly: no vote; one float32 step above: a vote -- at a general relative pose, tuned against the library's own T(v, f)"""
    from glio_amd import capi
    case = Cs.knife_case(ulps, capi.static_relative_pose, far)
    got, want, images, _ = run_case(owner, case)
    assert_equal_to_restated(got, want, images, case["name"])
    assert got[1]["tested"][0] == 1 and got[1]["through"][0] == ulps and len(got[1]["kept"]) == 1 - ulps


# ---------------------------------------------------------------------------------------------- votes and static frames
def general_poses(n, seed, base=0.0):
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 7))
    for f in range(n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        a = rng.uniform(-0.2, 0.2)
        p[f] = np.r_[rng.uniform(-1.5, 1.5, 3) + base, np.cos(a / 2), np.sin(a / 2) * ax]
    return p


def votes_case(kind, n_views, min_votes, seed, opts=MID):
    """8 random frames (sizes 300, 257, 1, 65, 300, 64, 63, 300) in shells of 5 m at different ranges, the four dense ones farthest, so that the near ones are
    seen through; frame f views n_views[f] others (repeats allowed beyond 7)"""
    sizes, near = (CAP, 257, 1, 65, CAP, 64, 63, CAP), (9.0, 14.0, 4.0, 4.0, 19.0, 6.0, 6.0, 24.0)
    clouds = [random_cloud(n, seed + i, near[i], near[i] + 5.0, 44.0) for i, n in enumerate(sizes)]
    poses = np.tile(Cs.IDENTITY, (8, 1)) if kind == "identity" else general_poses(8, seed, 1.0e6 if kind == "far" else 0.0)
    rng = np.random.default_rng(seed + 100)
    off, views = [0], []
    for f in range(8):
        others = [v for v in range(8) if v != f]
        views += [int(others[i % 7]) for i in rng.permutation(max(n_views[f], 7))[:n_views[f]]]
        off.append(len(views))
    return dict(name=kind, opts=dict(opts, min_votes=min_votes, max_views=max(max(n_views), min_votes)), clouds=clouds, poses=poses,
                view_offsets=np.array(off, np.int32), views=np.array(views, np.int32))


@pytest.mark.parametrize("kind,n_views,min_votes", [("identity", (1, 2, 3, 4, 5, 6, 7, 0), 1), ("general", (7, 1, 5, 2, 3, 0, 4, 6), 2), ("far", (7, 7, 2, 5, 1, 6, 4, 3), 3),
                                                    ("general", (32, 9, 1, 16, 31, 2, 8, 32), 2)])
def test_votes_and_static_frames_on_random_clouds(owner, kind, n_views, min_votes):
    case = votes_case(kind, n_views, min_votes, 40 + min_votes)
    got, want, images, info = run_case(owner, case)
    assert_equal_to_restated(got, want, images, kind)
    th = np.concatenate([g["through"] for g in got])
    assert (th >= min_votes).sum() > 20 and (th < min_votes).sum() > 200 and (th == min_votes - 1).sum() > 0      # both outcomes, and the count just below the threshold
    assert info.n_dynamic == int((th >= min_votes).sum()) and info.n_points == sum(len(c) for c in case["clouds"])
    for f in range(8):
        if n_views[f] == 0:
            assert np.array_equal(got[f]["kept"].view(np.uint32), case["clouds"][f].view(np.uint32)) and not got[f]["tested"].any()


def test_the_default_image_and_both_paths_agree(owner):
    """44 x 360 with nb = 0 (300 points leave the 3 x 3 neighbourhoods of a 1 degree image empty): LDS path == global path == the restatement"""
    case = votes_case("general", (7, 1, 5, 2, 3, 0, 4, 6), 1, 77, dict(neighbourhood=0))
    # (the frames are near copies of each other, so that cells are hit: frame f = frame 0 pushed out by up to 30 %)
    base = random_cloud(CAP, 5, el=12.0)
    base[:, 2] -= F32(0.15) * np.abs(base[:, 0])
    rng = np.random.default_rng(9)
    case["clouds"] = [np.ascontiguousarray(np.c_[base[:n, :3] * rng.uniform(0.7, 1.3, (n, 1)).astype(F32), base[:n, 3]].astype(F32)) for n in (CAP, 257, 1, 65, CAP, 64, 63, CAP)]
    case["poses"] = np.tile(Cs.IDENTITY, (8, 1))
    a, want, images, info_a = run_case(owner, case, 0)
    b, _, _, info_b = run_case(owner, case, 1)
    assert info_a.lds_path and not info_b.lds_path
    assert_equal_to_restated(a, want, images, "lds")
    assert_equal_to_restated(b, want, images, "global")
    assert sum(int(g["through"].sum()) for g in a) > 50


def test_everything_removed_and_nothing_removed(owner):
    P = R.Params(**Cs.mini_params())
    view = Cs.grid_cloud(P, np.full((4, 8), 30.0))
    inner = Cs.probes(P, [(r, c, 7.0) for r in (1, 2) for c in range(8)] * 17)            # 272 probes in the middle rows: all seen through
    outer = Cs.probes(P, [(r, c, 35.0) for r in (1, 2) for c in range(8)])                # behind the view's points: all kept
    case = dict(opts=Cs.mini_params(), clouds=[view, inner, outer], poses=np.tile(Cs.IDENTITY, (3, 1)), view_offsets=np.array([0, 0, 1, 2], np.int32),
                views=np.array([0, 0], np.int32))
    got, want, images, info = run_case(owner, case)
    assert_equal_to_restated(got, want, images)
    assert len(got[1]["kept"]) == 0 and got[1]["through"].min() == 1
    assert np.array_equal(got[2]["kept"].view(np.uint32), outer.view(np.uint32)) and got[2]["tested"].min() == 1 and got[2]["through"].max() == 0
    assert (info.n_points, info.n_tested, info.n_dynamic) == (32 + 272 + 16, 272 + 16, 272)


# ---------------------------------------------------------------------------------------------- invariances
def test_a_frames_result_does_not_depend_on_what_else_is_in_the_call(owner):
    case = votes_case("general", (3, 2, 4, 1, 2, 3, 1, 2), 2, 61)
    got, _, _, _ = run_case(owner, case)
    st, P, tab = make(owner, case["opts"])
    for k, c in enumerate(case["clouds"]):
        owner.set_frame(k, c)
    for f in (0, 2, 4):
        vs = [int(v) for v in case["views"][case["view_offsets"][f]:case["view_offsets"][f + 1]]]
        members = [f] + sorted(set(vs), reverse=True)                                    # another order, other call-local indices, nothing else in the call
        local = {k: i for i, k in enumerate(members)}
        off = [0, len(vs)] + [len(vs)] * (len(members) - 1)
        st.classify(members, case["poses"][members], off, [local[v] for v in vs])
        th, te = st.read_votes(f)
        assert np.array_equal(th, got[f]["through"]) and np.array_equal(te, got[f]["tested"])
        assert np.array_equal(st.read_frame(f).view(np.uint32), got[f]["kept"].view(np.uint32))
        for v in set(vs):
            assert np.array_equal(bits(st.read_image(local[v])[1]), bits(got[v]["image"][1]))
    st.close()


def test_run_to_run_and_owner_kinds(owner):
    """bit-identical from run to run; a dense store as the owner gives what the batch association gives; the owner's store is byte-equal afterwards"""
    from glio_amd import mapping, static_map
    case = votes_case("general", (3, 2, 4, 1, 2, 3, 1, 2), 2, 61)
    first, _, _, _ = run_case(owner, case)
    again, _, _, _ = run_case(owner, case)
    dense = mapping.DenseClouds(K_FRAMES, CAP, CAP)
    for k, c in enumerate(case["clouds"]):
        assert dense.set_frame(k, c, 0.0) == len(c)
    st = static_map.StaticClouds(dense, **case["opts"])
    st.classify(list(range(8)), case["poses"], case["view_offsets"], case["views"])
    for k in range(8):
        th, te = st.read_votes(k)
        for other in (again[k], dict(through=th, tested=te, kept=st.read_frame(k), image=st.read_image(k))):
            assert np.array_equal(first[k]["through"], other["through"]) and np.array_equal(first[k]["tested"], other["tested"])
            assert np.array_equal(first[k]["kept"].view(np.uint32), other["kept"].view(np.uint32))
            assert np.array_equal(bits(first[k]["image"][0]), bits(other["image"][0])) and np.array_equal(bits(first[k]["image"][1]), bits(other["image"][1]))
        assert np.array_equal(dense.read_frame(k).view(np.uint32), case["clouds"][k].view(np.uint32))
        assert st.frame_count(k) == len(first[k]["kept"])
    ms = st.last_device_ms()
    assert len(ms) == 4 and all(m >= 0 for m in ms) and ms[0] > 0 and ms[2] > 0
    st.close(); dense.close()


def test_the_owner_may_overwrite_a_frame_right_after_classify(owner):
    case = votes_case("general", (3, 2, 4, 1, 2, 3, 1, 2), 2, 61)
    want, _, _, _ = run_case(owner, case)
    st, P, tab = make(owner, case["opts"])
    for k, c in enumerate(case["clouds"]):
        owner.set_frame(k, c)
    st.classify(list(range(8)), case["poses"], case["view_offsets"], case["views"])
    for k in range(8):
        owner.set_frame(k, random_cloud(CAP, 900 + k))                     # no host wait in between: the owner's write comes behind the read on the device
    for k in range(8):
        assert np.array_equal(st.read_frame(k).view(np.uint32), want[k]["kept"].view(np.uint32))
    st.close()


# ---------------------------------------------------------------------------------------------- refusals
def state_bytes(st):
    out = []
    for k in range(K_FRAMES):
        th, te = st.read_votes(k)
        out.append((st.frame_count(k), st.read_frame(k).tobytes(), th.tobytes(), te.tobytes()))
    return out


def test_refusals_leave_store_counts_and_votes_byte_equal(owner):
    from glio_amd import capi
    import ctypes as C
    from glio_amd import ctypes_types as T
    case = votes_case("general", (2, 2, 2, 1, 0, 0, 0, 0), 1, 71)
    case["opts"]["max_views"] = 2
    st, P, tab = make(owner, case["opts"])
    for k, c in enumerate(case["clouds"]):
        owner.set_frame(k, c)
    owner.set_frame(7, np.zeros((0, 4), F32))
    off, views = np.array([0, 2, 4, 6, 7], np.int32), np.array([1, 2, 0, 3, 3, 1, 0], np.int32)
    st.classify([0, 1, 2, 3], case["poses"][:4], off, views)
    before = state_bytes(st)
    assert before[0][0] > 0 and before[5][0] == 0
    nan, P4 = float("nan"), case["poses"][:4]

    def poses_with(f, c, v):
        p = P4.copy(); p[f, c] = v
        return p

    zero_q = P4.copy(); zero_q[2, 3:] = 0.0
    bad = [([0, 1, 2, K_FRAMES], P4, off, views), ([0, -1, 2, 3], P4, off, views),                                  # an index out of range
           ([0, 1, 2, 7], P4, off, views), ([0, 1, 2, 6][:0], P4[:0], [0], []),                                     # an empty frame; n = 0
           ([0, 1, 2, 3], poses_with(1, 0, nan), off, views), ([0, 1, 2, 3], poses_with(3, 4, float("inf")), off, views), ([0, 1, 2, 3], zero_q, off, views),
           ([0, 1, 2, 3], P4, off, np.r_[0, views[1:]]),                                                            # frame 0 views itself
           ([0, 1, 2, 3], P4, off, np.r_[views[:-1], 4]), ([0, 1, 2, 3], P4, off, np.r_[-1, views[1:]]),            # a view out of range
           ([0, 1, 2, 3], P4, [0, 3, 4, 6, 7], views),                                                              # more than max_views
           ([0, 1, 2, 3], P4, [0, 2, 1, 6, 7], views), ([0, 1, 2, 3], P4, [1, 2, 4, 6, 7], views),                  # offsets descend; do not start at 0
           ([0, 1, 2, 0], P4, off, views)]                                                                          # a frame twice
    for frames, poses, o, v in bad:
        with pytest.raises((capi.GlioError, AssertionError)):
            st.classify(frames, poses, o, v)
        assert state_bytes(st) == before, (frames, list(o), list(v))
    lib = capi.load()
    fr, po, of, vi = np.array([0, 1, 2, 3], np.int32), np.ascontiguousarray(P4), np.ascontiguousarray(off, np.int32), np.ascontiguousarray(views, np.int32)
    info = T.GlioStaticInfo()
    for args in ((9, T.iptr(fr), T.dptr(po), T.iptr(of), T.iptr(vi)), (4, None, T.dptr(po), T.iptr(of), T.iptr(vi)), (4, T.iptr(fr), None, T.iptr(of), T.iptr(vi)),
                 (4, T.iptr(fr), T.dptr(po), None, T.iptr(vi)), (4, T.iptr(fr), T.dptr(po), T.iptr(of), None)):
        assert lib.glio_static_classify(st._h, *args, C.byref(info)) == capi.E_ARG
        assert state_bytes(st) == before
    for call in (lambda: st.read_frame(8), lambda: st.read_votes(-1), lambda: st.read_image(4), lambda: st.frame_count(8)):
        with pytest.raises(capi.GlioError):
            call()
    # and the same call goes through afterwards, to the same bytes
    st.classify([0, 1, 2, 3], P4, off, views)
    assert state_bytes(st) == before
    st.close()


def test_read_image_before_the_first_call_is_a_state_error(owner):
    from glio_amd import capi, static_map
    st = static_map.StaticClouds(owner, **Cs.mini_params())
    with pytest.raises(capi.GlioError, match="-3"):
        st.read_image(0)
    with pytest.raises(capi.GlioError, match="-3"):
        st.last_device_ms()
    assert st.frame_count(0) == 0 and len(st.read_frame(0)) == 0
    st.close()

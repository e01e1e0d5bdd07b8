"""GPU: place recognition end to end on the scenes scripts/search_place_cases.py kept (tests/golden/place_scenes.json): every revisit finds its true place
and heading where the position rule of the loop thread, with 100 m of drift, finds nothing; and the heading is what lets the device ICP converge."""
import math

import numpy as np
import pytest

import loop_restated as lr
import place_cases as Cs
import place_restated as R
import place_scenes as S

pytestmark = pytest.mark.gpu

N_PLACES = 12
TIME_THRES = 30.0                      # lc_time_thres of the yaml
ICP_THRES = 0.2                        # lc_icp_thres of the yaml


class World:
    pass


@pytest.fixture(scope="module")
def world():
    from glio_amd import batch, capi, place
    g = S.kept()
    assert len(g["seeds"]) >= 12 and g["candidates"] - len(g["seeds"]) == len(g["refused"])
    seeds = [s for s in g["seeds"] if s != g["align"]["seed"]][:N_PLACES - 1] + [g["align"]["seed"]]
    w = World()
    w.golden, w.seeds, w.n = g, seeds, len(seeds)
    w.params = [S.parameters(s) for s in seeds]
    w.places = [S.place_scan(p) for p in w.params]
    w.visits = [S.revisit_scan(p) for p in w.params]
    cap = max(len(c) for c in w.places + w.visits)
    w.owner = batch.BatchAssociation(2 * w.n, cap, 16)
    for k, c in enumerate(w.places + w.visits):
        w.owner.set_frame(k, c)
    w.pr = place.PlaceRecognition(w.owner, max_places=2 * w.n, max_radius=g["max_radius"], lidar_height=g["lidar_height"])
    w.times = [40.0 * i for i in range(w.n)] + [1000.0 + 0.1 * i for i in range(w.n)]          # (the revisits are within lc_time_thres of each other)
    w.pr.add_frames(list(range(2 * w.n)), list(range(2 * w.n)), w.times)          # one launch for all 24 clouds
    # the restatement of the same store, once
    tabs = capi.place_tables(g["max_radius"])
    w.st = R.Store(2 * w.n)
    w.desc = []
    for k, c in enumerate(w.places + w.visits):
        h, m = R.descriptor(c, tabs[0], tabs[1], g["lidar_height"])
        w.desc.append((h, m))
        w.st.set(k, h, m, w.times[k])
    yield w
    w.pr.close(); w.owner.close()


def test_descriptors_of_real_scans_bit_for_bit(world):
    for k in range(2 * world.n):
        h, m, t, v = world.pr.read_descriptor(k)
        assert v and t == world.times[k] and m == world.desc[k][1] and np.array_equal(h.view(np.uint32), world.desc[k][0].view(np.uint32)), k
    assert bin(world.desc[0][1]).count("1") >= 50


def test_every_revisit_finds_its_place_where_the_radius_rule_finds_none(world):
    from glio_amd import loop, place
    w = world
    # the places laid out 1 km apart in one world; the revisit's pose carries 100 m of drift
    positions = np.array([p["origin"] + [1000.0 * i, 0, 0] for i, p in enumerate(w.params)], np.float32)
    many, nf = w.pr.query_many(w.n, w.n, TIME_THRES, True, 3)
    for i, p in enumerate(w.params):
        q = w.n + i
        assert Cs.separated(w.st, q, TIME_THRES, 3)                           # (vetted on the CPU: place and shift are exact)
        want = w.st.query(q, TIME_THRES, 3)
        got = w.pr.query(q, TIME_THRES, 3)
        assert len(got) == 3
        for gm, (d, c, s) in zip(got, want):
            assert Cs.within_gate(gm["distance"], d) and (int(gm["place"]), int(gm["shift"])) == (c, s)
        assert nf[i] == 3 and many[i].tobytes() == got.tobytes()
        rest = w.golden["restated"][str(w.seeds[i])]
        assert int(got[0]["place"]) == i and float(got[0]["distance"]) <= w.golden["distance_threshold"] and int(got[0]["shift"]) == rest["shift"]
        assert float(got[1]["distance"]) - float(got[0]["distance"]) >= w.golden["margin"]
        # half a sector plus what the restatement itself shows on this revisit
        yaw_err = S.angle_diff(float(got[0]["yaw"]), p["yaw"])
        print(f"seed {w.seeds[i]}: distance {float(got[0]['distance']):.4f}, next {float(got[1]['distance']):.4f}, yaw error {math.degrees(yaw_err):.2f} deg "
              f"(restated {math.degrees(rest['yaw_error']):.2f})")
        assert yaw_err <= math.radians(3.0) + rest["yaw_error"]
        t_now = w.times[q]
        closest, yaw, dist = place.detect_candidate_by_appearance(w.pr, q, TIME_THRES, t_now, -1.0)
        assert (closest, yaw, dist) == (i, float(got[0]["yaw"]), float(got[0]["distance"]))
        assert place.detect_candidate_by_appearance(w.pr, q, TIME_THRES, t_now, t_now - 0.1)[0] == -1          # the 0.2 s gate behind the last loop
        assert place.detect_candidate_by_appearance(w.pr, q, TIME_THRES, t_now, -1.0, dist_thres=0.5 * dist)[0] == -1
        here = positions[i] + p["offset"].astype(np.float32)
        assert loop.detect_candidate(positions, w.times[:w.n], here, t_now, -1.0, 25.0, TIME_THRES) == i
        assert loop.detect_candidate(positions, w.times[:w.n], here + np.float32([100.0, 0, 0]), t_now, -1.0, 25.0, TIME_THRES) == -1
    print(f"largest |device - restated| distance on the scenes: {Cs.LARGEST['deviation']:.3e} (gate {Cs.GATE:.3e})")


def test_the_heading_is_what_lets_the_icp_converge(world):
    from glio_amd import loop, place
    w = world
    i = w.n - 1
    p = w.params[i]
    assert w.seeds[i] == w.golden["align"]["seed"] and abs(p["yaw"] - math.pi / 2) < math.radians(15)
    assert w.golden["align"]["fitness_with_guess"] < 0.5 * ICP_THRES and w.golden["align"]["fitness_without"] > 2 * ICP_THRES          # established on the CPU
    closest, yaw, _ = place.detect_candidate_by_appearance(w.pr, w.n + i, TIME_THRES, w.times[w.n + i], -1.0)
    assert closest == i
    pose_closest = np.r_[p["origin"], 1.0, 0.0, 0.0, 0.0]
    guess = place.initial_guess(pose_closest, yaw)
    assert np.allclose(guess[:3], p["origin"]) and np.allclose(guess[3:], [math.cos(yaw / 2), 0, 0, math.sin(yaw / 2)])
    assert np.allclose(place.initial_guess(pose_closest, yaw, q_query=[math.cos(0.3), 0, 0, math.sin(0.3)]), guess)          # a level query: its own heading drops out
    lp = loop.LoopClosure(w.owner)
    lp.build_submap(loop.TARGET, [i], [pose_closest])
    lp.build_submap(loop.SOURCE, [w.n + i], [guess])
    r = lp.align()
    src, tgt = lp.read_submap(loop.SOURCE), lp.read_submap(loop.TARGET)
    want = lr.icp(src, tgt)
    dt, dr = lr.pose_error(r.transform, want["transform"])
    print(f"with the guess: {r.as_dict()['state']} after {r.iterations} rounds, fitness {r.fitness:.4f}; vs the restatement |dt| {dt:.2e} m, |dR| {dr:.2e} rad")
    assert r.converged and r.fitness < ICP_THRES
    assert (r.iterations, r.state, r.converged) == (want["iterations"], want["state"], want["converged"]) and dt < 1e-4 and dr < 1e-5          # tests/test_hip_loop.py's gate
    # the rotation it found is the heading's remainder (point-to-point ICP slides along the corridor: the translation is not held to the offset)
    assert S.angle_diff(math.atan2(float(r.transform[1, 0]), float(r.transform[0, 0])), p["yaw"] - yaw) < math.radians(1.0)
    lp.build_submap(loop.SOURCE, [w.n + i], [pose_closest])                  # the same pair without the heading
    r0 = lp.align()
    print(f"without: converged {r0.converged} after {r0.iterations} rounds, fitness {r0.fitness:.4f}")
    assert not (r0.converged and r0.fitness < ICP_THRES)
    lp.close()

"""GPU: the C++ host (glio::SlidingWindowBackend through host_demo / host_demo_map_schedule, opt-in argument `arm`) and the Python calls agree through a
loop closure with the speed-bias priors armed: the first window after it (factors installed before the solve, the marginalization carries the blocks of
slots 1 .. W-2), marginalize-and-keep with the factors installed, and the solve of the next window on the wider resident prior."""
import numpy as np
import pytest

from glio_amd import synth
from glio_amd.host import window_io

pytestmark = pytest.mark.gpu


def test_cpp_armed_sequence_matches_python_sequence(tmp_path):
    from glio_amd import capi
    W = 4
    win = synth.make_window(W=W, pts_per_scan=3000, seed=synth.SEED_BASE + 31)
    path = str(tmp_path / "win.bin")
    window_io.write_window(path, win)
    info, trans, quat = window_io.run_demo(path, arm=True)
    plain, trans0, _ = window_io.run_demo(path)
    ctx = capi.Context(win.opts)
    ctx.set_map(win.map_pts)
    kept = 0
    for s in range(W):
        q2, t2 = capi.lidar_pose(win.opts, win.init.quat[s], win.init.trans[s])
        kept += ctx.associate(s, win.scans[s], q2, t2)
    ctx.load_window(win, None, use_gnss=False, use_prior=False)
    ctx.set_speed_bias_priors(win.init.speed_bias[:W - 1])          # what solve() installs when armed: tmpSpeedBias[0 .. W-2] before the solve
    sol, summ = ctx.solve(win.init)
    assert info["kept"] == kept and info["iterations"] == summ.iterations and info["termination"] == summ.termination
    assert np.isclose(info["final_cost"], summ.final_cost, rtol=1e-12)
    assert np.abs(trans - sol.trans).max() < 1e-12
    assert np.abs(trans - trans0).max() > 1e-6 and plain["final_cost"] != info["final_cost"]      # the argument is not a no-op
    qs = sol.quat * np.where(sol.quat[:, :1] < 0, -1.0, 1.0)
    st = sol.copy(); st.quat = qs
    out = ctx.marginalize(st)
    assert out["n"] == 6 * (W - 1) + 9 + 9 * (W - 3)
    assert info["prior"]["n"] == out["n"] and info["prior"]["n_blocks"] == len(out["blk_slot"])
    assert np.isclose(info["prior"]["jac_fro2"], (out["lin_jac"] ** 2).sum(), rtol=1e-9)
    assert np.isclose(info["prior"]["res2"], out["lin_res"] @ out["lin_res"], rtol=1e-7, atol=1e-12)
    ctx.set_speed_bias_priors(None)                                   # the read-back marginalization disarms and clears the context
    poses = [capi.lidar_pose(win.opts, st.quat[s], st.trans[s]) for s in range(W)]
    counts = ctx.associate_window(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
    ctx.set_speed_bias_priors(st.speed_bias[:W - 1])                  # armed again: installed at the state the second solve starts from
    again, summ_a = ctx.solve(st)
    again.quat *= np.where(again.quat[:, :1] < 0, -1.0, 1.0)
    assert info["rearmed"]["iterations"] == summ_a.iterations and np.isclose(info["rearmed"]["final_cost"], summ_a.final_cost, rtol=1e-12)
    ctx.marginalize_keep(again)
    sol2, summ2 = ctx.solve(again)
    assert info["resident"]["kept"] == int(np.sum(counts)) and info["resident"]["iterations"] == summ2.iterations
    assert np.isclose(info["resident"]["final_cost"], summ2.final_cost, rtol=1e-12)
    n, nb = ctx.marginalize_size()
    assert (info["next"]["n"], info["next"]["n_blocks"], info["next"]["armed"]) == (n, nb, 0) and n == 6 * (W - 1) + 9 + 9 * (W - 4)
    ctx.close()


def test_map_schedule_demo_arms_at_the_loop_closure(tmp_path):
    W, width, NK, pts, cap, loop_after = 3, 3, 5, 1500, 2048, 2
    win = synth.make_window(W=NK, pts_per_scan=pts, seed=synth.SEED_BASE + 84, scan_radius=25.0)
    opts = synth.default_opts(W, pts=cap, map_pts=1 << 16)
    pose_info = np.tile(np.c_[win.gt.trans[:NK], win.gt.quat[:NK]], (NK, 1, 1))
    path = str(tmp_path / "schedule.bin")
    window_io.write_map_schedule(path, opts, cap, width, 0.4, win.scans[:NK], pose_info, loop_after=loop_after)
    plain = window_io.run_demo_map_schedule(path, str(tmp_path / "maps.bin"))
    armed = window_io.run_demo_map_schedule(path, str(tmp_path / "maps_armed.bin"), arm=True)
    assert [r[3] for r in armed] == [1 if j >= loop_after else 0 for j in range(NK)]
    for a, b in zip(plain, armed):
        assert a[:2] == b[:2] and np.array_equal(a[2], b[2])

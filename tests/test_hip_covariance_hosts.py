"""The two hosts of the window's marginal covariance: host_demo_stream cov=1 (glio::SlidingWindowBackend::covariance) against the Python drivers with
covariance=True on the same short stream, and glio::pose3Covariance against sliding.pose3_covariance."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trace(cov):
    tr = 0.0
    for c in range(15):          # (the order host_demo_stream sums in)
        tr += float(cov[c, c])
    return tr


@pytest.mark.gpu
def test_cpp_stream_covariance_equals_the_python_driver(tmp_path):
    """The keyframe cycle of host_demo_stream with cov=1 -- the newest keyframe's 15 x 15 block asked between solve() and the marginalization -- against the
    same C entry points driven from Python (the stream's own order of calls): the same traces to the bit, keyframe by keyframe; the Pose3 block of the last
    one; and the solved poses with cov=1 equal those without it.  Then sliding.ResidentSlidingWindow(covariance=True) on the last window: a fourth value,
    the bits of Context.covariance at the solved state."""
    from glio_amd import capi, sliding, synth
    from glio_amd.capi import lidar_pose
    from glio_amd.host import window_io
    W, pts, NK = 5, 1024, 3
    long = synth.make_window(W=W + NK, pts_per_scan=pts, with_gnss=False, with_prior=False, seed=synth.SEED_BASE + 723)
    wins = [synth.sub_window(long, j, W) for j in range(NK + 1)]
    opts = wins[0].opts
    opts.max_map_points = 1 << 16
    path = str(tmp_path / "stream.bin")
    window_io.write_stream(path, long, wins, W, NK, pts)
    plain = window_io.run_demo_stream(path, search_range=6)           # (search_range 6: the 8-keyframe stream never reaches the batch association)
    got = window_io.run_demo_stream(path, search_range=6, cov=True)
    assert "covariance_newest_trace" not in plain and len(got["covariance_newest_trace"]) == NK + 1
    for key in ("iterations", "correspondences_kept", "last_trans", "last_quat", "trans_checksum"):
        assert got[key] == plain[key], key
    ahead = window_io.run_demo_stream(path, search_range=6, cov=True, ahead=True, map_ahead=True)
    assert ahead["covariance_newest_trace"] == got["covariance_newest_trace"] and ahead["last_trans"] == got["last_trans"]
    ctx = capi.Context(opts)
    ctx.localmap_config(50, 0.4, pts)
    tlb = np.array(opts.t_lb, np.float32)
    for j in range(W - 1):
        c = long.scans[j].copy(); c[:, :3] -= tlb
        ctx.localmap_push(np.ascontiguousarray(c), long.gt.quat[j], long.gt.trans[j])
    for s in range(W - 1):
        ctx.set_scan(s + 1, long.scans[s])
    ctx.set_prior(None)
    traces, sol, cov = [], None, None
    for j in range(NK + 1):
        win = wins[j]
        state = win.init.copy()
        if j > 0:
            state.trans[:-1], state.quat[:-1], state.speed_bias[:-1] = sol.trans[1:], sol.quat[1:], sol.speed_bias[1:]
        new = j + W - 1
        ctx.slide_window(); ctx.set_scan(W - 1, long.scans[new])
        ctx.localmap_push_scan(W - 1, tlb, long.gt.quat[new], long.gt.trans[new]); ctx.localmap_build()
        poses = [lidar_pose(opts, state.quat[s], state.trans[s]) for s in range(W)]
        ctx.associate_window_async(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]))
        ctx.set_imu(win.preints); ctx.set_gnss(win.frame, win.dd, win.dop)
        ctx.associate_window_counts()
        sol, summ = ctx.solve(state)
        sliding.unify_quaternions(sol)
        cov, info = ctx.covariance(sol, slots=[W - 1])
        assert info.n == 15 * W and info.n_free == 0 and info.bad_pivot == -1
        traces.append(_trace(cov))
        ctx.marginalize_keep(sol)
    assert np.array_equal(np.array(got["last_trans"]).reshape(W, 3), sol.trans)
    assert got["covariance_newest_trace"] == traces
    p3 = sliding.pose3_covariance(cov[:6, :6], sol.quat[W - 1])
    assert np.abs(np.array(got["covariance_last_pose3"]).reshape(6, 6) - p3).max() <= 1e-13 * np.abs(p3).max()
    assert got["covariance_last_device_ms"] > 0
    ctx.close()
    # the resident driver on the last window's inputs: step() returns the block as a fourth value
    win = wins[NK]
    for flag in (False, True):
        c2 = capi.Context(win.opts)
        drv = sliding.ResidentSlidingWindow(c2, win.opts, covariance=flag)
        st = win.init.copy(); st.n_ddt = 0
        drv.start(st)
        res = drv.step(long.map_pts, win.scans, win.preints)
        if flag:
            assert len(res) == 4 and res[3].shape == (15, 15) and np.array_equal(res[3], res[3].T) and np.all(np.diag(res[3]) > 0)
            assert drv.last_covariance_info.bad_pivot == -1
            assert np.array_equal(res[0].trans, base[0].trans) and res[1].as_dict() == base[1].as_dict()
        else:
            assert len(res) == 3 and drv.last_covariance is None
            base = res
        c2.close()


def test_pose3_covariance_cpp_equals_python(tmp_path):
    """glio::pose3Covariance against sliding.pose3_covariance on random blocks and quaternions (not normalised on purpose): the same A Sigma A^T up to the
    order of two 6-term sums, 1e-13 of the largest entry"""
    from glio_amd import sliding
    here = os.path.join(ROOT, "glio_amd", "host")
    src = tmp_path / "p3.cpp"
    src.write_text('#include "glio_backend.hpp"\n#include <cstdio>\n#include <cstdlib>\n'
                   'int main(int argc, char** argv) { double c[36], q[4]; for (int k = 0; k < 36; ++k) c[k] = strtod(argv[1 + k], nullptr);\n'
                   '  for (int k = 0; k < 4; ++k) q[k] = strtod(argv[37 + k], nullptr);\n'
                   '  const std::array<double, 36> p = glio::pose3Covariance(c, q); for (double v : p) printf("%.17g ", v); printf("\\n"); return 0; }\n')
    exe = str(tmp_path / "p3")
    subprocess.check_call(["g++", "-std=c++14", "-O1", str(src), "-I" + here, "-I" + os.path.join(ROOT, "include"), "-o", exe])
    rng = np.random.default_rng(13)
    for _ in range(5):
        M = rng.normal(0, 1, (6, 6))
        S = M @ M.T
        q = rng.normal(0, 1, 4) * 3.0
        out = subprocess.run([exe] + [repr(float(v)) for v in S.ravel()] + [repr(float(v)) for v in q], capture_output=True, text=True, check=True).stdout.split()
        got = np.array([float(v) for v in out]).reshape(6, 6)
        want = sliding.pose3_covariance(S, q)
        assert np.array_equal(got, got.T) and np.abs(got - want).max() <= 1e-13 * np.abs(want).max()

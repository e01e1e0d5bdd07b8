"""GPU: the two hosts of the GNSS frame estimate -- host_demo_align (glio::GnssAlignment, host/glio_align_backend.hpp) and align.GnssAlignment -- agree bit for
bit on one case, a pose table passed as it lies included."""
import ctypes as C

import numpy as np
import pytest

import gnss_align_restated as R


@pytest.mark.gpu
def test_cpp_and_python_hosts_agree_bit_for_bit(tmp_path):
    from glio_amd import align, capi
    from glio_amd import ctypes_types as T
    from glio_amd.host import window_io
    c = R.make_case("K24", "wrap_1km")
    opts = capi.align_opts(n_hypotheses=36, max_yaw_sigma=0.01)
    start = align.frame_of(c["start_psi"], c["start_anc"])
    poses = np.zeros((len(c["P"]), 7)); poses[:, :3] = c["P"]; poses[:, 3] = 1.0          # [n][7], stride 7
    path = str(tmp_path / "align.bin")
    window_io.write_align_case(path, opts, start, c["dd"], poses)
    cpp = window_io.run_demo_align(path)
    al = align.GnssAlignment(len(c["dd"]), len(poses), opts=opts)
    al.set_factors(c["dd"]); al.set_positions(poses)
    out, info = T.GlioGnssFrame(), T.GlioAlignInfo()
    capi._check(capi.load().glio_align_solve(al._h, C.byref(start), C.byref(out), C.byref(info)))
    coarse = al.read_coarse()
    cost, nd = al.cost(out, 6.0)
    al.close()
    assert cpp["frame"] == bytes(out) and cpp["info"] == bytes(info) and cpp["coarse"] == coarse.tobytes()
    assert cpp["cost"] == np.float64(cost).tobytes() and (cpp["status"], cpp["rows"], cpp["downweighted"]) == (align.WEAK, c["fs"].n_rows, nd)
    want = R.restate(c, 36, max_yaw_sigma=0.01)
    assert info.winner == want["winner"] and info.status == want["status"] == R.WEAK

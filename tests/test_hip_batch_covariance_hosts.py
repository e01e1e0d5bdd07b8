"""The two hosts of the batch stage's per-keyframe covariance: host_demo_batch_cov (glio::BatchBackend::covariance) against batch.BatchStage.covariance
on one case -- the 15-state problem with DD pseudoranges, an anchor inside a super-block and the (k, k + 1) blocks -- byte for byte."""
import ctypes as C

import numpy as np
import pytest

import batch_covariance_problems as problems


@pytest.mark.gpu
def test_cpp_covariance_equals_the_python_host(tmp_path):
    from glio_amd import synth
    from glio_amd.host import window_io
    p = problems.build(dict(family="imu", K=13, band=6, gnss=True, anchor=4))
    st = problems.stage(p)
    diag, nxt, info = st.covariance(p["init"], p["sb0"], anchor=4, cross=True)
    st.close()
    path = str(tmp_path / "cov.bin")
    window_io.write_batch_cov_case(path, p["K"], p["band"], 4, True, p["init"], p["sb0"], p["con"], p["dq"], p["frame"], p["dd"], p["imu"], synth.GRAVITY)
    got = window_io.run_demo_batch_cov(path)
    assert got["B"] == 15 and got["bad_keyframe"] == -1 and got["levels"] == info.levels
    assert got["diag"] == diag.tobytes() and got["next"] == nxt.tobytes()
    assert got["info"] == C.string_at(C.addressof(info), C.sizeof(info))
    assert not diag[4][:6].any() and np.all(np.diag(diag[3]) > 0)

"""GPU: the two hosts of the static map -- glio::StaticClouds, glio::staticViews and glio::GlobalMap on the static store (host/glio_static_backend.hpp,
through host_demo_static_map) and glio_amd.static_map / mapping.GlobalMap -- agree byte for byte on the first five scans of the street."""
import numpy as np
import pytest

import static_map_cases as Cs

pytestmark = pytest.mark.gpu


def test_the_cpp_host_and_the_python_host_agree_byte_for_byte(tmp_path):
    from glio_amd import capi, mapping, static_map
    from glio_amd.host import window_io
    clouds, poses, labels = Cs.street()
    clouds, poses = clouds[:5], poses[:5]
    K, cap, half_window, min_baseline = len(clouds), 4096, 2, 0.5
    opts = capi.static_opts(min_votes=1)
    gopts = mapping.default_opts(max_voxels=1 << 16, max_points_per_add=1 << 16)
    path = str(tmp_path / "static_case.bin")
    window_io.write_static_map_case(path, opts, gopts, cap, half_window, min_baseline, clouds, poses)
    cpp = window_io.run_demo_static_map(path)

    dense = mapping.DenseClouds(K, cap, cap)
    for k, c in enumerate(clouds):
        dense.set_frame(k, c, 0.0)
    off, views = static_map.static_views(poses, half_window, min_baseline)
    assert cpp["view_offsets"] == off.tobytes() and cpp["views"] == views.tobytes() and len(views) == 14
    st = static_map.StaticClouds(dense, opts)
    info = st.classify(range(K), poses, off, views)
    got = np.frombuffer(cpp["info"], [("p", "<i8"), ("t", "<i8"), ("d", "<i8"), ("n", "<i4"), ("l", "<i4")])[0]
    assert (int(got["p"]), int(got["t"]), int(got["d"]), int(got["n"]), int(got["l"])) == (info.n_points, info.n_tested, info.n_dynamic, K, 1) and info.n_dynamic > 100
    for k in range(K):
        th, te = st.read_votes(k)
        assert cpp["frame%d" % k] == st.read_frame(k).tobytes() and cpp["through%d" % k] == th.tobytes() and cpp["tested%d" % k] == te.tobytes()
    assert cpp["floor"] == st.read_image(K - 1)[1].tobytes()
    gm = mapping.GlobalMap(st, gopts)
    gi = gm.add(list(range(K)), poses)
    assert int.from_bytes(cpp["voxels"], "big") == gi.n_voxels > 1000 and cpp["map"] == gm.read().tobytes()
    gm.close(); st.close(); dense.close()

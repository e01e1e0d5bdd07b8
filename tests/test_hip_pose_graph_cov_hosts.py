"""GPU: the covariance of every pose-graph node through both hosts.  host_demo_pose_graph_cov (C++: glio::PoseGraph::marginalCovariances,
glio_posegraph_backend.hpp) and the Python twin (posegraph.PoseGraph.marginal_covariances) build the same graph from the same bytes, solve it and ask: the same
library, the same bits."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cov_restated as R
from glio_amd import posegraph
from glio_amd import ctypes_types as T
from glio_amd.host import window_io

pytestmark = pytest.mark.gpu


def test_cpp_host_and_python_twin_agree_bit_for_bit(tmp_path):
    sc = R.scenes()["gps_loops"]
    path = str(tmp_path / "case.bin")
    window_io.write_pose_graph_cov_case(path, sc["x0"], sc["loops"], sc["gps"], 5)
    cpp = window_io.run_demo_pose_graph_cov(path)
    pg = posegraph.PoseGraph(posegraph.default_opts(max_nodes=40, max_loops=3, max_unary=3, segment_nodes=5))
    pg.set_prior(sc["x0"][0]); pg.append(sc["x0"])
    for lp in sc["loops"]:
        pg.add_between(*lp)
    for gp in sc["gps"]:
        pg.add_gps(*gp)
    pg.solve()
    diag, nxt, info = pg.marginal_covariances(next=True, with_info=True)
    pg.close()
    assert cpp["diag"] == diag.tobytes() and cpp["next"] == nxt.tobytes()
    ci = T.GlioPgraphCovInfo.from_buffer_copy(cpp["info"])
    assert len(cpp["info"]) == C.sizeof(T.GlioPgraphCovInfo) and ci.as_dict() == info
    assert (cpp["nodes"], cpp["separators"], cpp["full_row_separators"], cpp["bad_node"]) == (40, info["separators"], 3, -1)
    assert np.isfinite(diag).all() and (np.abs(diag).reshape(40, -1).max(axis=1) > 0).all()

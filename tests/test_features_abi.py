"""glio_feat_opts / glio_feat_counts: the ctypes mirrors against the compiled library, the defaults against config_urban_hk.yaml."""
import ctypes as C

from glio_amd import capi, features
from glio_amd import ctypes_types as T


def test_feature_struct_sizes_match_the_library():
    lib = capi.load()
    out = (C.c_int32 * 2)()
    assert lib.glio_feat_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioFeatOpts), C.sizeof(T.GlioFeatCounts)]


def test_feature_defaults_are_the_yaml_and_the_node():
    lib = capi.load()
    lib.glio_feat_opts_default.restype = None
    o = T.GlioFeatOpts()
    lib.glio_feat_opts_default(C.byref(o))
    # config_urban_hk.yaml:14-18,90-93: line_num 32, ds_rate 1, edgeThreshold 1.0, surfThreshold 0.1, ql2b identity; ds_v 0.4 and the 3 m cut
    assert (o.n_scans, o.ds_rate, o.edge_threshold, o.surf_threshold) == (32, 1, 1.0, 0.1)
    assert abs(o.ds_leaf - 0.4) < 1e-7 and o.min_range == 3.0 and list(o.q_lb) == [1.0, 0.0, 0.0, 0.0]
    assert o.max_raw_points == T.FEAT_MAX_RAW_POINTS == 400000
    p = features.default_opts()
    assert bytes(p) == bytes(o)

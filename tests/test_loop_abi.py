"""glio_loop_opts / glio_loop_result / glio_loop_step_result: the ctypes mirrors against the compiled library, the defaults against the reference's
statements (Estimator.cpp:855, :5197-5200) and PCL 1.8.1's."""
import ctypes as C

from glio_amd import capi, loop
from glio_amd import ctypes_types as T


def test_loop_struct_sizes_match_the_library():
    lib = capi.load()
    out = (C.c_int32 * 3)()
    assert lib.glio_loop_struct_sizes(out, 3) == 3
    assert list(out) == [C.sizeof(T.GlioLoopOpts), C.sizeof(T.GlioLoopResult), C.sizeof(T.GlioLoopStepResult)]


def test_loop_defaults_are_the_reference_and_pcl():
    lib = capi.load()
    lib.glio_loop_opts_default.restype = None
    o = T.GlioLoopOpts()
    lib.glio_loop_opts_default(C.byref(o))
    # Estimator.cpp:855 ds_filter_his_frames.setLeafSize(0.4, 0.4, 0.4); :5197-5200 setMaxCorrespondenceDistance(30), setMaximumIterations(100),
    # setTransformationEpsilon(1e-6), setEuclideanFitnessEpsilon(1e-6)
    assert abs(o.leaf - 0.4) < 1e-7 and o.max_corr_dist == 30.0 and o.max_iterations == 100 and o.transformation_eps == 1e-6 and o.fitness_eps == 1e-6
    # PCL 1.8.1: DefaultConvergenceCriteria::mse_threshold_absolute_ 1e-12, Registration::min_number_correspondences_ 3
    assert o.abs_mse_eps == 1e-12 and o.min_correspondences == 3
    # capacities: the reference's 6 and 2 * lc_map_width + 1 = 51 keyframes fit
    assert o.max_frames_per_submap == 64 >= 2 * 25 + 1 and o.max_source_points == 65536 and o.max_target_points == 262144
    assert bytes(loop.default_opts()) == bytes(o)
    assert loop.default_opts(max_iterations=7).max_iterations == 7
    assert (T.LOOP_SOURCE, T.LOOP_TARGET) == (0, 1) and len(T.LOOP_STATE_NAMES) == 6 and T.LOOP_STATE_NAMES[T.LOOP_NO_CORRESPONDENCES] == "NO_CORRESPONDENCES"


def test_loop_entry_points_resolve():
    lib = capi.load()
    for name in ("glio_loop_create", "glio_loop_destroy", "glio_loop_build_submap", "glio_loop_set_submap", "glio_loop_read_submap", "glio_loop_align",
                 "glio_loop_reset_current", "glio_loop_step", "glio_loop_read_correspondences", "glio_loop_read_current", "glio_loop_read_fallbacks",
                 "glio_loop_last_device_ms"):
        assert getattr(lib, name) is not None

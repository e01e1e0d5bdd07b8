"""glio_imu_noise / glio_imu_sample: the ctypes mirrors against the compiled library, the default noise against config_urban_hk.yaml."""
import ctypes as C

from glio_amd import capi, imu, synth
from glio_amd import ctypes_types as T


def test_imu_struct_sizes_match_the_library():
    lib = capi.load()
    out = (C.c_int32 * 2)()
    assert lib.glio_imu_struct_sizes(out, 2) == 2
    assert list(out) == [C.sizeof(T.GlioImuNoise), C.sizeof(T.GlioImuSample)]
    assert C.sizeof(T.GlioImuSample) == 7 * 8          # a [n][7] float64 array is an array of samples


def test_imu_noise_default_is_the_yaml():
    n = imu.default_noise()          # config_urban_hk.yaml:7-10
    assert (n.acc_n, n.gyr_n, n.acc_w, n.gyr_w) == (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
    assert (n.acc_n, n.gyr_n, n.acc_w, n.gyr_w) == (3.9939570888238808e-03, 1.5636343949698187e-03, 6.4356659353532566e-05, 3.5640318696367613e-05)

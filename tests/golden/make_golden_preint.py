"""Records tests/golden/preint_cases.npz: raw IMU edges and what the reference's own `class Preintegration` (compiled unmodified,
oracle.pyref.preintegrate) makes of them.  Runs only where the reference tree exists; the fixture holds data only (inputs and the
resulting glio_preint bytes).  tests/test_preint_golden.py holds it to the numpy restatement, tests/test_hip_imu.py holds the device to it.

    python tests/golden/make_golden_preint.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from glio_amd import ctypes_types as T  # noqa: E402
from glio_amd import synth  # noqa: E402
from oracle import pyref  # noqa: E402

YAML = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)      # config_urban_hk.yaml:7-10
HEADER = (0.00059, 0.000061, 0.000011, 0.000001)                 # Preintegration.h:48-51

# (name, samples, dt rule, noise, biases?, |gyr|)
CASES = [
    ("n0", 0, 0.01, YAML, False, 0.1), ("n1", 1, 0.01, YAML, False, 0.1), ("n2", 2, 0.01, YAML, True, 0.1), ("n3", 3, 0.0025, YAML, False, 0.1),
    ("n40_dt10", 40, 0.01, YAML, False, 0.1), ("n40_dt2p5_bias", 40, 0.0025, YAML, True, 0.1), ("n40_jitter_bias", 40, "jitter", YAML, True, 0.1),
    ("n40_header", 40, 0.01, HEADER, False, 0.1), ("n40_header_jitter_bias", 40, "jitter", HEADER, True, 0.1),
    ("n100_bias", 100, 0.01, YAML, True, 0.1), ("n100_header_jitter", 100, "jitter", HEADER, False, 0.1),
    ("n160_dt2p5_bias", 160, 0.0025, YAML, True, 0.1), ("n160_jitter", 160, "jitter", YAML, False, 0.1), ("n160_header_bias", 160, 0.01, HEADER, True, 0.1),
    ("n400_bias", 400, 0.0025, YAML, True, 0.1), ("n1000", 1000, 0.0025, YAML, False, 0.05),
    ("n40_first_dt0", 40, "first0", YAML, True, 0.1), ("n2_first_dt0", 2, "first0", YAML, False, 0.1),
    ("n10_coarse", 10, 0.1, YAML, True, 0.1), ("n20_coarse_header", 20, 0.1, HEADER, False, 0.1),
    ("n100_rotating", 100, 0.01, YAML, True, 2.0), ("n160_rotating_jitter", 160, "jitter", YAML, False, 2.0),
    ("n3_header_bias", 3, 0.01, HEADER, True, 0.1), ("n1_header_bias", 1, 0.0025, HEADER, True, 0.1),
]


def make_case(rng, n, rule, bias, wnorm):
    if rule == "jitter":
        dt = rng.uniform(0.002, 0.012, n)
    elif rule == "first0":
        dt = np.full(n, 0.01); dt[0] = 0.0
    else:
        dt = np.full(n, float(rule))
    acc = np.array([0.0, 0.0, 9.8]) + rng.normal(0, 0.6, (n + 1, 3))
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    gyr = wnorm * axis + rng.normal(0, 0.05 * max(wnorm, 0.1), (n + 1, 3))
    ba = rng.normal(0, 0.05, 3) if bias else np.zeros(3)
    bg = rng.normal(0, 0.01, 3) if bias else np.zeros(3)
    return dt, acc, gyr, ba, bg


def main():
    assert os.path.isdir(os.path.join(pyref.REFERENCE, "GLIO", "include", "factors")), "needs the reference tree"
    rng = np.random.default_rng(20261016)
    offs, dts, accs, gyrs, starts, noises, outs, names = [0], [], [], [], [], [], [], []
    for name, n, rule, noise, bias, wnorm in CASES:
        dt, acc, gyr, ba, bg = make_case(rng, n, rule, bias, wnorm)
        for key, v in zip(("/IMU/acc_n", "/IMU/gyr_n", "/IMU/acc_w", "/IMU/gyr_w"), noise):
            pyref.set_param(key, v)
        got = pyref.preintegrate(acc[0], gyr[0], ba, bg, dt, acc[1:].reshape(-1, 3), gyr[1:].reshape(-1, 3))
        offs.append(offs[-1] + n); dts.append(dt); accs.append(acc[1:]); gyrs.append(gyr[1:])
        starts.append(np.concatenate([acc[0], gyr[0], ba, bg])); noises.append(noise); names.append(name)
        outs.append(np.frombuffer(bytes(got), np.uint8).copy())
    path = os.path.join(HERE, "preint_cases.npz")
    np.savez_compressed(path, names=np.array(names), offsets=np.array(offs, np.int32), dt=np.concatenate(dts), acc=np.concatenate(accs).reshape(-1, 3),
                        gyr=np.concatenate(gyrs).reshape(-1, 3), start=np.array(starts), noise=np.array(noises), preint=np.array(outs))
    print(path, os.path.getsize(path), "bytes,", len(names), "cases,", offs[-1], "samples, sizeof(glio_preint) =", C.sizeof(T.GlioPreint))


if __name__ == "__main__":
    main()

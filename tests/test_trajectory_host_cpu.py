"""The host's share of the every-frame trajectory: trajectory.frame_samples (Estimator.cpp:4287-4375, :4399-4481) on hand-made cases and against its C++ twin
glio::frameImuSamples through a small host program: identical doubles, bit for bit.  CPU only."""
import os
import subprocess

import numpy as np

from glio_amd import trajectory


def _buffer(n=60, seed=3):
    rng = np.random.default_rng(seed)
    stamps = 10.0 + np.arange(n) / 100.0
    acc = np.array([0.3, -0.2, 9.8]) + rng.normal(0, 0.3, (n, 3))
    gyr = rng.normal(0, 0.1, (n, 3))
    return stamps, acc, gyr


def test_start_rows_the_clamps_and_the_index():
    stamps, acc, gyr = _buffer()
    acc[2] = [40.0, 0.0, 0.0]; acc[3] = [40.0, 0.0, 0.0]          # around the first frame stamp: an in-between start row, NOT clamped
    acc[5] = [20.0, -20.0, -25.0]                                 # a whole sample: clamped
    acc[20] = [40.0, 0.0, 30.0]; acc[21] = [40.0, 0.0, 30.0]      # around the last segment's first stamp: clamped
    fs = [stamps[2] + 0.004, stamps[20] + 0.005, stamps[30] + 0.002]
    offs, smp, ii = trajectory.frame_samples(stamps, acc, gyr, fs, 2)
    assert list(offs) == [0, 1 + 18 + 1, 20 + 1 + 10 + 1]
    assert abs(smp[0, 1] - 40.0) < 1e-12 and smp[0, 0] == 0.0                      # :4295-4301
    assert list(smp[3, 1:4]) == [15.0, -15.0, -18.0]                              # sample 5
    assert list(smp[20, 1:4]) == [15.0, acc[20][1] * 0 + smp[20, 2], 18.0]        # :4413-4419
    assert ii == 31                                                               # not stepped back after the last segment
    # the closing row of segment 0 interpolates from the CLAMPED acc of the last whole sample (:4348): make that sample exceed the clamp
    acc[20] = [40.0, 0.0, 9.8]; acc[21] = [0.0, 0.0, 9.8]
    offs, smp, _ = trajectory.frame_samples(stamps, acc, gyr, fs, 2)
    dt1, dt2 = fs[1] - stamps[20], stamps[21] - fs[1]
    w1, w2 = dt2 / (dt1 + dt2), dt1 / (dt1 + dt2)
    assert smp[19, 1] == w1 * 15.0 + w2 * 0.0 and smp[19, 0] == dt1
    # ... and the next segment's start row comes from the raw samples 20, 21 again (ii-- at :4375), clamped because it is the last segment's
    assert smp[20, 1] == min(15.0, w1 * 40.0 + w2 * 0.0)


def test_frame_stamp_equal_to_an_imu_stamp():
    """the loop's `<` is strict: the sample AT the frame stamp is not taken whole; it is the closing row's partner with dt2 = 0, w2 = 1"""
    stamps, acc, gyr = _buffer()
    fs = [stamps[4] + 0.003, stamps[9], stamps[15] + 0.001]
    offs, smp, _ = trajectory.frame_samples(stamps, acc, gyr, fs, 4)
    assert list(offs) == [0, 1 + 4 + 1, 6 + 1 + 7 + 1]          # samples 5-8; then 9-15, sample 9 whole with dt 0
    assert smp[5, 0] == stamps[9] - stamps[8] and np.array_equal(smp[5, 4:7], 0.0 * gyr[8] + 1.0 * gyr[9])
    # the next segment starts between samples 8 and 9 with dt1 = the whole interval: w1 = 0, the start row is sample 9, and sample 9 is then taken whole
    assert np.array_equal(smp[6, 4:7], 0.0 * gyr[8] + 1.0 * gyr[9]) and smp[7, 0] == 0.0 and np.array_equal(smp[7, 4:7], gyr[9])


def test_cpp_twin_gives_the_same_doubles(tmp_path):
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glio_amd", "host")
    exe = str(tmp_path / "frame_samples")
    subprocess.check_call(["g++", "-std=c++14", "-O1", os.path.join(here, "host_frame_samples_test.cpp"), "-I" + os.path.join(here, "..", "..", "include"), "-o", exe])
    rng = np.random.default_rng(21)
    for trial in range(8):
        n = 400
        stamps = 50.0 + np.cumsum(rng.uniform(0.002, 0.012, n))
        acc = np.array([0.0, 0.0, 9.8]) + rng.normal(0, 8.0 if trial % 2 == 0 else 0.5, (n, 3))          # every second trial reaches the clamps
        gyr = rng.normal(0, 0.3, (n, 3))
        gaps = []
        for g in range(6):
            idx = int(rng.integers(0, 100))
            m = int(rng.integers(2, 7))
            fs = np.sort(rng.uniform(stamps[idx], stamps[idx + 1], 1).tolist() + rng.uniform(stamps[idx + 1], stamps[idx + 250], m - 1).tolist())
            if g == 1:
                k = int(np.searchsorted(stamps, fs[1])) + 1
                fs[1] = stamps[k]                         # a frame stamp exactly on a sample
                fs = np.sort(fs)
            if g == 2 and m > 2:
                fs[2] = fs[1] + 1e-4                      # a segment without a whole sample
                fs = np.sort(fs)
            gaps.append((idx, fs))
        text = [f"{n} {len(gaps)}"] + [" ".join(repr(float(v)) for v in np.r_[stamps[i], acc[i], gyr[i]]) for i in range(n)]
        for idx, fs in gaps:
            text += [f"{len(fs)} {idx}", " ".join(repr(float(t)) for t in fs)]
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        ln = 0
        for idx, fs in gaps:
            offs, smp, ii = trajectory.frame_samples(stamps, acc, gyr, fs, idx)
            head = out[ln].split(); ln += 1
            assert head[0] == "gap" and [int(v) for v in head[1:]] == [len(offs), len(smp), ii], (trial, idx)
            w = out[ln].split(); ln += 1
            assert w[0] == "o" and [int(v) for v in w[1:]] == list(offs)
            for s in smp:
                w = out[ln].split(); ln += 1
                assert w[0] == "s" and [float.fromhex(v) for v in w[1:]] == [float(v) for v in s], (trial, idx)
        assert ln == len(out)

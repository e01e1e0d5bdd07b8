"""The host's share of the raw IMU input: imu.keyframe_samples (the sample preparation of saveKeyFramesAndFactors, Estimator.cpp:4162-4229) and
imu.propagate_state (Rs / Ps / Vs of processIMU, :1592-1598) on hand-made cases, and against their C++ twins glio::keyframeImuSamples /
glio::propagateImuState through a small host program: identical doubles, bit for bit.  CPU only."""
import os
import subprocess

import numpy as np

from glio_amd import imu, synth


def _buffer(n=30, rate=100.0, t0=10.0, seed=3):
    rng = np.random.default_rng(seed)
    stamps = t0 + np.arange(n) / rate
    acc = np.array([0.3, -0.2, 9.8]) + rng.normal(0, 0.3, (n, 3))
    gyr = rng.normal(0, 0.1, (n, 3))
    return stamps, acc, gyr


def test_acceleration_clamps():
    stamps, acc, gyr = _buffer()
    acc[2] = [20.0, -20.0, -25.0]
    acc[3] = [14.0, 16.0, 17.5]
    acc[4] = [-15.5, 3.0, 18.5]
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, stamps[6] + 0.004)
    assert list(smp[2, 1:4]) == [15.0, -15.0, -18.0] and list(smp[3, 1:4]) == [14.0, 15.0, 17.5] and list(smp[4, 1:4]) == [-15.0, 3.0, 18.0]
    assert np.array_equal(smp[:7, 4:7], gyr[:7])          # the angular rate is not clamped
    # the closing sample is clamped AFTER the interpolation (:4216-4222)
    acc[7] = [40.0, 0.0, 0.0]; acc[6] = [14.0, 0.0, 0.0]
    smp, _, _ = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, stamps[6] + 0.004)
    assert smp[-1, 1] == 15.0


def test_first_call_and_dt_bookkeeping():
    stamps, acc, gyr = _buffer()
    kf = stamps[5] + 0.003
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, kf)
    assert len(smp) == 7 and idx == 6 and cur == kf
    assert smp[0, 0] == 0.0          # cur_time_imu < 0: the very first sample's dt is 0 (:4169-4171)
    assert all(smp[k, 0] == stamps[k] - stamps[k - 1] for k in range(1, 6))
    assert smp[6, 0] == kf - stamps[5]
    # the next keyframe: the first dt runs from the previous keyframe's time, sample 6 is taken whole
    kf2 = stamps[9] + 0.001
    smp2, idx2, cur2 = imu.keyframe_samples(stamps, acc, gyr, idx, cur, kf2)
    assert len(smp2) == 5 and idx2 == 10 and cur2 == kf2 and smp2[0, 0] == stamps[6] - kf and np.array_equal(smp2[0, 1:4], acc[6])


def test_closing_sample_weights():
    """dt1 = 1 ms, dt2 = 3 ms: w1 = dt2 / (dt1 + dt2) = 0.75 on the last sample taken, w2 = 0.25 on the next"""
    stamps = np.array([0.0, 0.010, 0.014, 0.020])
    acc = np.array([[0, 0, 9.0], [1.0, 2.0, 10.0], [5.0, -2.0, 6.0], [0, 0, 0]])
    gyr = np.array([[0, 0, 0], [0.4, 0.0, -0.8], [0.0, 0.4, 0.8], [0, 0, 0]])
    kf = 0.011
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, kf)
    assert len(smp) == 3 and idx == 2 and cur == kf
    dt1, dt2 = kf - stamps[1], stamps[2] - kf
    w1, w2 = dt2 / (dt1 + dt2), dt1 / (dt1 + dt2)
    assert abs(w1 - 0.75) < 1e-12 and abs(w2 - 0.25) < 1e-12
    assert smp[2, 0] == dt1
    assert list(smp[2, 1:4]) == [w1 * 1.0 + w2 * 5.0, w1 * 2.0 + w2 * -2.0, w1 * 10.0 + w2 * 6.0]
    assert list(smp[2, 4:7]) == [w1 * 0.4 + w2 * 0.0, w1 * 0.0 + w2 * 0.4, w1 * -0.8 + w2 * 0.8]


def test_keyframe_exactly_on_a_sample():
    """the loop's `<` is strict (:4167): the sample AT the keyframe time is not taken whole; it is the closing sample's partner with dt2 = 0, w2 = 1"""
    stamps, acc, gyr = _buffer()
    kf = stamps[4]
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, kf)
    assert len(smp) == 5 and idx == 4 and cur == kf
    assert smp[4, 0] == stamps[4] - stamps[3] and np.array_equal(smp[4, 1:4], 0.0 * acc[3] + 1.0 * acc[4]) and np.array_equal(smp[4, 4:7], 0.0 * gyr[3] + 1.0 * gyr[4])
    # and the next call takes that sample whole, with dt = 0
    smp2, idx2, _ = imu.keyframe_samples(stamps, acc, gyr, idx, cur, stamps[6] + 0.002)
    assert smp2[0, 0] == 0.0 and np.array_equal(smp2[0, 1:4], acc[4]) and idx2 == 7


def test_buffer_ends_before_the_keyframe():
    """the early break (:4194-4195): no closing sample, idx_imu = the buffer's size"""
    stamps, acc, gyr = _buffer(n=8)
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, 2, stamps[1], stamps[-1] + 0.5)
    assert len(smp) == 6 and idx == 8 and cur == stamps[-1] + 0.5
    assert smp[-1, 0] == stamps[7] - stamps[6] and np.array_equal(smp[-1, 1:4], acc[7])
    smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, idx, cur, stamps[-1] + 0.9)          # nothing left: an edge without samples
    assert smp.shape == (0, 7) and idx == 8


def test_propagate_state_against_a_numpy_restatement():
    """processIMU's Rs / Ps / Vs (:1592-1598) restated with numpy and synth.q2R_eigen (toRotationMatrix of the non-normalised deltaQ)"""
    rng = np.random.default_rng(8)
    stamps, acc, gyr = _buffer(n=60, seed=9)
    smp, _, _ = imu.keyframe_samples(stamps, acc, gyr, 0, -1.0, stamps[50] + 0.002)
    R0 = synth.q2R(synth.rotvec_q(rng.normal(0, 0.3, 3)))
    P0, V0, ba, bg = rng.normal(0, 5, 3), rng.normal(0, 2, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)
    a0, w0, g = acc[0] * 1.01, gyr[0] * 0.9, np.array([0, 0, synth.GRAVITY])
    R, P, V, a_end, w_end = imu.propagate_state(R0, P0, V0, ba, bg, a0, w0, smp, g)
    Rn, Pn, Vn, an, wn = R0.copy(), P0.copy(), V0.copy(), a0.copy(), w0.copy()
    for s in smp:
        dt, a1, w1 = s[0], s[1:4], s[4:7]
        un0 = Rn @ (an - ba) - g
        ug = 0.5 * (wn + w1) - bg
        Rn = Rn @ synth.q2R_eigen(np.r_[1.0, ug * dt / 2])
        un1 = Rn @ (a1 - ba) - g
        un = 0.5 * (un0 + un1)
        Pn = Pn + dt * Vn + 0.5 * dt * dt * un
        Vn = Vn + dt * un
        an, wn = a1, w1
    assert np.abs(R - Rn).max() < 1e-13 and np.abs(P - Pn).max() < 1e-12 and np.abs(V - Vn).max() < 1e-12
    assert np.array_equal(a_end, smp[-1, 1:4]) and np.array_equal(w_end, smp[-1, 4:7])
    assert abs(np.linalg.det(R) - 1) < 1e-4          # not renormalised, as in the reference: the drift over 51 samples is what it is


def test_cpp_twins_give_the_same_doubles(tmp_path):
    here = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glio_amd", "host")
    exe = str(tmp_path / "imu_samples")
    subprocess.check_call(["g++", "-std=c++14", "-O1", os.path.join(here, "host_imu_samples_test.cpp"), "-I" + os.path.join(here, "..", "..", "include"), "-o", exe])
    rng = np.random.default_rng(21)
    for trial in range(12):
        n = int(rng.integers(5, 200))
        stamps = 50.0 + np.cumsum(rng.uniform(0.002, 0.012, n))
        acc = np.array([0.0, 0.0, 9.8]) + rng.normal(0, 6.0 if trial % 3 == 0 else 0.5, (n, 3))          # every third trial reaches the clamps
        gyr = rng.normal(0, 0.3, (n, 3))
        kfs = np.sort(rng.uniform(stamps[0] - 0.01, stamps[-1] + 0.05, int(rng.integers(1, 8))))
        if trial % 4 == 1:
            kfs[0] = stamps[min(3, n - 1)]          # a keyframe exactly on a sample
        idx0, cur0 = (0, -1.0) if trial % 2 == 0 else (1, float(stamps[0]))
        R0 = synth.q2R(synth.rotvec_q(rng.normal(0, 0.5, 3)))
        st = np.concatenate([R0.ravel(), rng.normal(0, 5, 3), rng.normal(0, 2, 3), rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3), acc[0], gyr[0], [0, 0, synth.GRAVITY]])
        text = [f"{n} {len(kfs)} {idx0} {cur0!r}"] + [" ".join(repr(float(v)) for v in np.r_[stamps[i], acc[i], gyr[i]]) for i in range(n)]
        text += [" ".join(repr(float(t)) for t in kfs), " ".join(repr(float(v)) for v in st)]
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        idx, cur = idx0, cur0
        R, P, V, ba, bg, a0, w0, g = R0, st[9:12], st[12:15], st[15:18], st[18:21], st[21:24], st[24:27], st[27:30]
        ln = 0
        for t in kfs:
            smp, idx, cur = imu.keyframe_samples(stamps, acc, gyr, idx, cur, t)
            head = out[ln].split(); ln += 1
            assert head[0] == "kf" and int(head[1]) == len(smp) and int(head[2]) == idx and float.fromhex(head[3]) == cur, (trial, t)
            for s in smp:
                w = out[ln].split(); ln += 1
                assert w[0] == "s" and [float.fromhex(v) for v in w[1:]] == [float(v) for v in s], (trial, t)
            R, P, V, a0, w0 = imu.propagate_state(R, P, V, ba, bg, a0, w0, smp, g)
            w = out[ln].split(); ln += 1
            assert w[0] == "x" and [float.fromhex(v) for v in w[1:]] == [float(v) for v in np.r_[R.ravel(), P, V, a0, w0]], (trial, t)
        assert ln == len(out)

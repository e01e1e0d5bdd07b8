"""tests/golden/preint_cases.npz -- raw IMU edges and the reference's own class Preintegration on them -- held to the numpy restatement
synth.preintegrate (the second witness, on every machine) and, where the reference tree exists, to oracle.pyref.preintegrate again."""
import numpy as np
import pytest

import preint_cases
from glio_amd import synth
from oracle import pyref

CASES = preint_cases.load()


def test_the_fixture_covers_what_it_should():
    counts = sorted({len(c["dt"]) for c in CASES})
    assert len(CASES) >= 24 and {0, 1, 2, 3, 40, 100, 160, 400, 1000} <= set(counts)
    assert any(len(c["dt"]) and c["dt"][0] == 0.0 for c in CASES) and any(len(c["dt"]) and c["dt"][0] == 0.1 for c in CASES)
    assert len({c["noise"] for c in CASES}) == 2
    assert any(np.any(c["start"][6:] != 0) for c in CASES) and any(np.all(c["start"][6:] == 0) for c in CASES)
    assert any(len(c["gyr"]) and np.linalg.norm(c["gyr"], axis=1).mean() > 1.5 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_numpy_restatement_meets_the_fixture(case):
    st = case["start"]
    acc, gyr = np.vstack([st[0:3], case["acc"].reshape(-1, 3)]), np.vstack([st[3:6], case["gyr"].reshape(-1, 3)])
    got = synth.preintegrate(acc, gyr, case["dt"], st[6:9], st[9:12], noise=case["noise"])
    preint_cases.check(got, case["want"], case["name"])
    assert list(case["want"].linearized_ba) == list(st[6:9]) and list(case["want"].linearized_bg) == list(st[9:12])
    if len(case["dt"]) == 0:          # the constructor's state, exactly
        w = case["want"]
        assert list(w.delta_q) == [1, 0, 0, 0] and w.sum_dt == 0 and np.array_equal(np.array(w.jacobian).reshape(15, 15), np.eye(15))
        assert np.array_equal(np.array(w.covariance).reshape(15, 15), 0.001 * np.eye(15))


@pytest.mark.skipif(not pyref.available(), reason="no reference tree and no prebuilt oracle/_ref/libglio_ref.so")
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_reproduces_the_fixture(case):
    pyref.build()
    for key, v in zip(("/IMU/acc_n", "/IMU/gyr_n", "/IMU/acc_w", "/IMU/gyr_w"), case["noise"]):
        pyref.set_param(key, v)
    st = case["start"]
    got = pyref.preintegrate(st[0:3], st[3:6], st[6:9], st[9:12], case["dt"], case["acc"].reshape(-1, 3), case["gyr"].reshape(-1, 3))
    preint_cases.check(got, case["want"], case["name"])

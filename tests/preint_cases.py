"""tests/golden/preint_cases.npz (recorded by tests/golden/make_golden_preint.py from the reference's own class Preintegration) and the
project's pre-integration tolerances: close(a, b, tol) := max|a - b| <= tol * max(1, max|b|) with tol = 1e-12 for delta_p, delta_q, delta_v,
sum_dt and 1e-11 for jacobian and covariance (tests/test_oracle_ref.py::test_preintegration_propagation), plus the covariance against
max|covariance| alone at 1e-11 (its entries are ~1e-3, so the max(1, .) form alone would be an absolute check)."""
import os

import numpy as np

from glio_amd import ctypes_types as T

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preint_cases.npz")
FIELDS = (("delta_p", 1e-12), ("delta_q", 1e-12), ("delta_v", 1e-12), ("sum_dt", 1e-12), ("jacobian", 1e-11), ("covariance", 1e-11))


def load():
    z = np.load(PATH)
    cases = []
    for k, name in enumerate(z["names"]):
        lo, hi = int(z["offsets"][k]), int(z["offsets"][k + 1])
        want = T.GlioPreint.from_buffer_copy(z["preint"][k].tobytes())
        cases.append(dict(name=str(name), dt=z["dt"][lo:hi].copy(), acc=z["acc"][lo:hi].copy(), gyr=z["gyr"][lo:hi].copy(), start=z["start"][k].copy(),
                          noise=tuple(float(v) for v in z["noise"][k]), want=want))
    return cases


def as_arrays(p):
    """dict of synth.preintegrate / GlioPreint -> {field: flat array}"""
    get = (lambda k: p[k]) if isinstance(p, dict) else (lambda k: getattr(p, k))
    return {k: np.atleast_1d(np.asarray(get(k) if not hasattr(get(k), "_length_") else list(get(k)), float)).ravel() for k, _ in FIELDS}


def deviations(got, want):
    """per field max|a - b| / max(1, max|b|), and the covariance relative to max|covariance| alone"""
    g, w = as_arrays(got), as_arrays(want)
    dev = {k: float(np.abs(g[k] - w[k]).max() / max(1.0, np.abs(w[k]).max())) if np.all(np.isfinite(g[k])) else float("inf") for k, _ in FIELDS}
    dev["covariance_rel"] = float(np.abs(g["covariance"] - w["covariance"]).max() / np.abs(w["covariance"]).max()) if np.all(np.isfinite(g["covariance"])) else float("inf")
    return dev


def check(got, want, label=""):
    dev = deviations(got, want)
    print(label, " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    for k, tol in FIELDS:
        assert dev[k] <= tol, (label, k, dev[k], tol)
    assert dev["covariance_rel"] <= 1e-11, (label, "covariance relative to its own scale", dev["covariance_rel"])
    return dev

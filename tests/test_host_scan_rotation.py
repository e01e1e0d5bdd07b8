"""glio::ScanRotation (C++, glio_backend.hpp) == features.ScanRotation (Python) == a constant-yaw-rate case worked by hand: Preprocessing's
processIMU / solveRotation (Preprocessing.cpp:202-259) with the first sample's dt = 0, the interpolated last step, idx_imu, the reset after each cloud."""
import os
import subprocess

import numpy as np

from glio_amd import features

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DRIVER = r'''
#include <cstdio>
#include <cstring>
#include "glio_backend.hpp"
int main() {
    glio::ScanRotation r;
    char op[8];
    double t, g[3];
    while (scanf("%7s %lf", op, &t) == 2) {
        if (!strcmp(op, "imu")) { if (scanf("%lf %lf %lf", &g[0], &g[1], &g[2]) != 3) return 2; r.addImu(t, g); }
        else { double q[4]; if (r.forScan(t, q)) printf("%.17g %.17g %.17g %.17g\n", q[0], q[1], q[2], q[3]); else printf("none\n"); }
    }
    return 0;
}
'''


def _events(rate=0.8, t_end=0.5):
    ev = [("scan", 0.0)]                                             # before any IMU sample: dropped ("Waiting for IMU data")
    ts = np.round(np.arange(0, t_end, 0.01), 10)
    scans = [0.105, 0.205, 0.305]
    for t in ts:
        ev.append(("imu", float(t), (0.0, 0.0, rate)))
        while scans and ts[ts <= t][-1] >= scans[0] + 0.02:
            ev.append(("scan", scans.pop(0)))
    return ev


def _python(ev):
    r = features.ScanRotation()
    out = []
    for e in ev:
        if e[0] == "imu":
            r.add_imu(e[1], e[2])
        else:
            q = r.for_scan(e[1])
            out.append(None if q is None else tuple(q))
    return out


def test_constant_yaw_rate_by_hand():
    rate = 0.8
    got = _python(_events(rate))
    assert got[0] is None and len(got) == 4
    # scan 1 at 0.105: samples 0.00 (dt = 0: the identity factor), 0.01 .. 0.10 (dt 0.01 each), then the interpolated step of 0.005 at the same
    # rate; every deltaQ is (1, 0, 0, rate dt / 2) -- NOT normalised -- and they commute (one axis): a product of complex numbers 1 + i rate dt / 2
    z = np.prod([1 + 0.5j * rate * 0.01] * 10 + [1 + 0.5j * rate * 0.005])
    assert np.allclose(got[1], (z.real, 0, 0, z.imag), rtol=0, atol=1e-15)
    # scan 2 at 0.205 after the reset: the step 0.105 -> 0.11 (the last sample time is t_cur), 0.11 .. 0.20, the interpolated 0.005
    z2 = np.prod([1 + 0.5j * rate * 0.005] + [1 + 0.5j * rate * 0.01] * 9 + [1 + 0.5j * rate * 0.005])
    assert np.allclose(got[2], (z2.real, 0, 0, z2.imag), rtol=0, atol=1e-15)
    assert abs(got[2][0] ** 2 + got[2][3] ** 2 - 1) > 1e-6        # the product drifts off the unit sphere, as the reference's does


def test_cpp_twin_equals_python(tmp_path):
    src = tmp_path / "scan_rotation.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "scan_rotation")
    subprocess.check_call(["g++", "-std=c++14", "-O2", str(src), "-I" + os.path.join(ROOT, "glio_amd", "host"), "-I" + os.path.join(ROOT, "include"), "-o", exe])
    ev = _events(rate=-1.3) + [("imu", 0.5, (0.2, -0.1, 0.4)), ("imu", 0.51, (0.3, 0.0, 0.1)), ("scan", 0.505)]
    lines = []
    for e in ev:
        lines.append("imu %.17g %.17g %.17g %.17g" % ((e[1],) + tuple(e[2])) if e[0] == "imu" else "scan %.17g" % e[1])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    cpp = [None if ln == "none" else tuple(float(x) for x in ln.split()) for ln in r.stdout.split("\n") if ln]
    py = _python(ev)
    assert cpp == py

// host_keyframe_gate_test.cpp -- CPU-only check program of glio::KeyframeGate (LidarOdometry.cpp:566-578): reads the frames from stdin as text -- per line the
// size the scan is judged with, then q (w x y z) and t as hexadecimal or decimal doubles -- and prints the decision and kf_num after every frame.
// Driven by tests/test_keyframe_cloud_abi.py against the Python twin (glio_amd/odometry.py::KeyframeGate) and a hand-made sequence.
#include <cstdio>

#include "glio_backend.hpp"

int main() {
    glio::KeyframeGate gate;
    int size = 0;
    double q[4], t[3];
    while (scanf("%d %lf %lf %lf %lf %lf %lf %lf", &size, &q[0], &q[1], &q[2], &q[3], &t[0], &t[1], &t[2]) == 8) {
        const bool kf = gate.update(q, t, size);
        printf("%d %d\n", kf ? 1 : 0, gate.keyframeNumber());
    }
    return 0;
}

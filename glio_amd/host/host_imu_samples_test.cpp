// host_imu_samples_test.cpp -- CPU-only check program of glio::keyframeImuSamples / glio::propagateImuState (Estimator.cpp:4162-4229, :1592-1598): reads an IMU
// buffer, the running values and a list of keyframe times from stdin as text, prints every sample list and the propagated state as hexadecimal doubles.
// Driven by tests/test_imu_host_cpu.py against the Python twins (glio_amd/imu.py): identical doubles, bit for bit.
#include <array>
#include <cstdio>
#include <vector>

#include "glio_backend.hpp"

int main() {
    int n = 0, n_kf = 0;
    long long idx0 = 0;
    double cur = -1;
    if (scanf("%d %d %lld %lf", &n, &n_kf, &idx0, &cur) != 4) return 2;
    std::vector<double> stamps(n), kf(n_kf);
    std::vector<std::array<double, 3>> acc(n), gyr(n);
    for (int i = 0; i < n; ++i)
        if (scanf("%lf %lf %lf %lf %lf %lf %lf", &stamps[i], &acc[i][0], &acc[i][1], &acc[i][2], &gyr[i][0], &gyr[i][1], &gyr[i][2]) != 7) return 2;
    for (double& t : kf) if (scanf("%lf", &t) != 1) return 2;
    double st[9 + 3 + 3 + 3 + 3 + 3 + 3 + 3];          // R, P, V, ba, bg, acc0, gyr0, g
    for (double& x : st) if (scanf("%lf", &x) != 1) return 2;
    double* R = st; double* P = st + 9; double* V = st + 12; double* ba = st + 15; double* bg = st + 18; double* a0 = st + 21; double* w0 = st + 24; double* g = st + 27;
    size_t idx = (size_t)idx0;
    for (double t : kf) {
        const std::vector<glio_imu_sample> s = glio::keyframeImuSamples(stamps, acc, gyr, idx, cur, t);
        printf("kf %zu %zu %a\n", s.size(), idx, cur);
        for (const glio_imu_sample& x : s) printf("s %a %a %a %a %a %a %a\n", x.dt, x.acc[0], x.acc[1], x.acc[2], x.gyr[0], x.gyr[1], x.gyr[2]);
        glio::propagateImuState(R, P, V, ba, bg, a0, w0, s, g);
        printf("x");
        for (int k = 0; k < 15; ++k) printf(" %a", st[k]);
        for (int k = 21; k < 27; ++k) printf(" %a", st[k]);
        printf("\n");
    }
    return 0;
}

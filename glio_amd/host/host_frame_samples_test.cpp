// host_frame_samples_test.cpp -- CPU-only check program of glio::frameImuSamples (Estimator.cpp:4287-4375, :4399-4481): reads an IMU buffer and a list of gaps
// (the frame stamps and the IMU index) from stdin as text, prints every gap's segment offsets and sample rows as hexadecimal doubles.
// Driven by tests/test_trajectory_host_cpu.py against the Python twin (glio_amd/trajectory.py): identical doubles, bit for bit.
#include <array>
#include <cstdio>
#include <vector>

#include "glio_trajectory_backend.hpp"

int main() {
    int n = 0, n_gaps = 0;
    if (scanf("%d %d", &n, &n_gaps) != 2) return 2;
    std::vector<double> stamps(n);
    std::vector<std::array<double, 3>> acc(n), gyr(n);
    for (int i = 0; i < n; ++i)
        if (scanf("%lf %lf %lf %lf %lf %lf %lf", &stamps[i], &acc[i][0], &acc[i][1], &acc[i][2], &gyr[i][0], &gyr[i][1], &gyr[i][2]) != 7) return 2;
    for (int g = 0; g < n_gaps; ++g) {
        int m = 0;
        long long idx = 0;
        if (scanf("%d %lld", &m, &idx) != 2) return 2;
        std::vector<double> fs(m);
        for (double& t : fs) if (scanf("%lf", &t) != 1) return 2;
        const glio::FrameSegments seg = glio::frameImuSamples(stamps, acc, gyr, fs, (size_t)idx);
        printf("gap %zu %zu %zu\n", seg.seg_offset.size(), seg.samples.size(), seg.imu_idx);
        printf("o");
        for (int32_t o : seg.seg_offset) printf(" %d", o);
        printf("\n");
        for (const glio_imu_sample& x : seg.samples) printf("s %a %a %a %a %a %a %a\n", x.dt, x.acc[0], x.acc[1], x.acc[2], x.gyr[0], x.gyr[1], x.gyr[2]);
    }
    return 0;
}

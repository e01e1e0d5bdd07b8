// host_demo_batch_cov -- the batch stage's per-keyframe marginal covariance in C++ over glio::BatchBackend::covariance (glio_batch_backend.hpp).
// Reads a case file written by glio_amd/host/window_io.py::write_batch_cov_case:
//   int32 K band anchor cross n_dq n_dd n_imu nc_width | int64 n_con | double poses [K][7] | double speed_bias [K][9] (n_imu > 0) |
//   int32 ci [n_con] cj [n_con] | float cp [n_con][4] | double nc [n_con][nc_width] score [n_con] | int32 dq_i [n_dq] dq_j [n_dq] | double dq_const [n_dq][4] |
//   glio_gnss_frame | glio_dd_psr [n_dd] | glio_preint [n_imu] | double gravity
// and prints the blocks' words in hex for tests/test_hip_batch_covariance_hosts.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_batch_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

static void hex(const char* name, const void* p, size_t bytes) {
    printf("%s ", name);
    for (size_t k = 0; k < bytes; ++k) printf("%02x", ((const unsigned char*)p)[k]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_batch_cov case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    int64_t n_con = 0;
    rd(f, head, 8); rd(f, &n_con, 1);
    const int K = head[0], band = head[1], anchor = head[2], cross = head[3], n_dq = head[4], n_dd = head[5], n_imu = head[6], ncw = head[7];
    std::vector<double> poses((size_t)K * 7), sb(n_imu > 0 ? (size_t)K * 9 : 0);
    rd(f, poses.data(), poses.size()); rd(f, sb.data(), sb.size());
    std::vector<int32_t> ci((size_t)n_con), cj((size_t)n_con);
    std::vector<float> cp((size_t)n_con * 4);
    std::vector<double> nc((size_t)n_con * ncw), score((size_t)n_con);
    rd(f, ci.data(), ci.size()); rd(f, cj.data(), cj.size()); rd(f, cp.data(), cp.size()); rd(f, nc.data(), nc.size()); rd(f, score.data(), score.size());
    glio::DeltaQPairs dq;
    dq.i.resize((size_t)n_dq); dq.j.resize((size_t)n_dq); dq.const_diff.resize((size_t)n_dq * 4);
    rd(f, dq.i.data(), dq.i.size()); rd(f, dq.j.data(), dq.j.size()); rd(f, dq.const_diff.data(), dq.const_diff.size());
    glio_gnss_frame frame;
    rd(f, &frame, 1);
    std::vector<glio_dd_psr> dd((size_t)n_dd);
    rd(f, dd.data(), dd.size());
    std::vector<glio_preint> imu((size_t)n_imu);
    rd(f, imu.data(), imu.size());
    double gravity = 0;
    rd(f, &gravity, 1);
    fclose(f);
    try {
        glio::BatchBackend stage(K, band, n_con > 0 ? n_con : 1, device);
        stage.setConstraints(n_con, ci.data(), cj.data(), cp.data(), nc.data(), score.data());
        const double thr = n_dd > 0 ? dd[0].threshold : 10.0;
        stage.setSmallFactors(&frame, dq, dd, thr);
        if (n_imu > 0) stage.setImu(imu, gravity);
        const glio::BatchBackend::Covariance c = stage.covariance(poses, n_imu > 0 ? &sb : nullptr, anchor, cross != 0);
        hex("diag", c.diag.data(), c.diag.size() * 8);
        if (cross) hex("next", c.next.data(), c.next.size() * 8);
        hex("info", &c.info, sizeof c.info);
        printf("B %d levels %d bad_keyframe %d\n", c.B, c.info.levels, c.info.bad_keyframe);
        printf("{\"covariance_device_ms\": %.4f}\n", stage.covarianceLastDeviceMs());
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

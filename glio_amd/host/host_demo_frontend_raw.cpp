// host_demo_frontend_raw.cpp -- the front end from RAW scans, driven from C++: Preprocessing::cloudHandler on the device (glio_features_extract)
// feeding LidarOdometry::run() (glio::ScanToMapOdometry::runRaw, glio_backend.hpp).  Input: a flat file written by
// glio_amd/host/window_io.py::write_frontend_raw_stream (glio_opts | glio_feat_opts | n_scans scan_match_cnt stride intensity_offset | per scan: n,
// q_imu[4] doubles, n raw records of `stride` bytes).  Output: one text line per scan (`pose i  q[4] t[3]  rounds  kept  iterations  final_cost
// map_points  surf`) and a JSON line with the time per scan -- tests/test_hip_frontend_raw.py compares the poses with the Python twin
// (glio_amd/odometry.py::ScanToMapOdometry.run_raw) bit for bit.
// Build: g++ -std=c++14 -O2 host_demo_frontend_raw.cpp -I../../include -L../lib -lglio_hip -Wl,-rpath,'$ORIGIN/../lib'
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_backend.hpp"

template <typename T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_frontend_raw stream.bin [device]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    glio_opts opts;
    glio_feat_opts fopts;
    rd(f, &opts, 1);
    rd(f, &fopts, 1);
    int32_t hdr[4];
    rd(f, hdr, 4);
    const int n_scans = hdr[0], match_cnt = hdr[1] > 0 ? hdr[1] : 1;
    const glio::PointLayout layout = {hdr[2], hdr[3]};
    std::vector<std::vector<unsigned char>> scans(n_scans);
    std::vector<std::array<double, 4>> qs(n_scans);
    std::vector<int> ns(n_scans);
    for (int i = 0; i < n_scans; ++i) {
        int32_t n; rd(f, &n, 1); ns[i] = n;
        rd(f, qs[i].data(), 4);
        scans[i].resize((size_t)n * layout.stride_bytes); rd(f, scans[i].data(), scans[i].size());
    }
    fclose(f);
    try {
        glio::ScanToMapOdometry odo(opts, device, match_cnt);
        odo.featuresConfig(fopts);
        std::vector<glio::ScanToMapOdometry::Round> rounds;
        double t_steady = 0; int n_steady = 0;
        for (int i = 0; i < n_scans; ++i) {
            glio_feat_counts cnt;
            const double t0 = now_s();
            const std::array<double, 7> p = odo.runRaw(scans[i].data(), ns[i], layout, qs[i].data(), &rounds, &cnt);
            const double dt = now_s() - t0;
            if (i >= 3) { t_steady += dt; ++n_steady; }
            long kept = 0; int iters = 0; double cost = 0;
            for (const auto& r : rounds) { kept += r.kept; iters += r.summary.iterations; cost = r.summary.final_cost; }
            printf("pose %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %zu %ld %d %.17g %d %d\n", i, p[0], p[1], p[2], p[3], p[4], p[5], p[6], rounds.size(), kept, iters,
                   cost, odo.mapPoints(), cnt.surf);
        }
        printf("{\"scans\": %d, \"steady_scans\": %d, \"ms_per_scan\": %.4f}\n", n_scans, n_steady, n_steady ? 1e3 * t_steady / n_steady : 0.0);
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

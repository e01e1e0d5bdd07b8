// host_map_schedule_mirror_test.cpp -- host-only (no device, no library): glio::localMapPlan (glio_backend.hpp) and glio::correctWindowPoses
// (glio_loop_backend.hpp) on numbers read from standard input, results printed with every double as a hex float, for tests/test_map_schedule_host_cpu.py
// to hold against sliding.local_map_plan and loop.correct_window_poses bit for bit.  One command per line:
//   plan recent_size n_keyframes width latest_frame_idx                 -> "plan action recent_size latest_frame_idx n frames..."
//   correct N W abs_poses[N * 7] corrected[(N - W) * 7]                 -> "ok 0|1", then N lines "row q t | R | P"
// Build: g++ -std=c++14 -O1 host_map_schedule_mirror_test.cpp -I../../include
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "glio_backend.hpp"
#include "glio_loop_backend.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<double> v;
        for (double x; in >> x;) v.push_back(x);
        if (cmd == "plan" && v.size() == 4) {
            const glio::LocalMapPlan p = glio::localMapPlan((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
            printf("plan %d %d %d %d", p.action, p.recent_size, p.latest_frame_idx, (int)p.frames.size());
            for (int32_t f : p.frames) printf(" %d", (int)f);
            printf("\n");
        } else if (cmd == "correct" && v.size() >= 2) {
            const int N = (int)v[0], W = (int)v[1];
            const int nc = N - W > 0 ? N - W : 0;
            if (N < 1 || v.size() != (size_t)(2 + 7 * N + 7 * nc)) { printf("ok 0\n"); continue; }
            std::vector<double> a(v.begin() + 2, v.begin() + 2 + 7 * N), c(v.begin() + 2 + 7 * N, v.end()), Rs((size_t)9 * N, 0.0), Ps((size_t)3 * N, 0.0);
            const bool ok = glio::correctWindowPoses(a.data(), N, c.data(), nc, W, Rs.data(), Ps.data());
            printf("ok %d\n", ok ? 1 : 0);
            if (!ok) continue;
            for (int i = 0; i < N; ++i) {
                printf("row");
                for (int k = 0; k < 7; ++k) printf(" %a", a[7 * i + k]);
                for (int k = 0; k < 9; ++k) printf(" %a", Rs[9 * i + k]);
                for (int k = 0; k < 3; ++k) printf(" %a", Ps[3 * i + k]);
                printf("\n");
            }
        } else { printf("bad command\n"); return 2; }
    }
    return 0;
}

// host_posegraph_mirror_test.cpp -- the host-only half of glio_posegraph_backend.hpp driven from stdin, for tests/test_pose_graph_host_cpu.py: no device, no
// library.  Commands, one per line (numbers as C hex floats or decimals):
//   frames n_keyframes W k id...                       -> the frame ids of glio::globalGraphFrames
//   edge latest closest k id...                        -> i j of glio::loopEdgeFrames
//   gate timeshift gnss_cov_threshold pose_cov_threshold   a fresh glio::GnssGate
//   push stamp x y z cx cy cz
//   select n_keyframes W x y z time cov33 cov44        -> "none <queued>" or "gps node x y z vx vy vz <queued>" (hex floats)
//   dist32 ax ay az bx by bz / dist64 ...              -> the distance as a hex float
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#include "glio_posegraph_backend.hpp"

static double num(std::istringstream& in) { std::string s; in >> s; return std::strtod(s.c_str(), nullptr); }

int main() {
    std::unique_ptr<glio::GnssGate> gate(new glio::GnssGate());
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "frames" || cmd == "edge") {
            int a, b, k;
            in >> a >> b >> k;
            std::vector<int32_t> ids(k);
            for (int q = 0; q < k; ++q) in >> ids[q];
            if (cmd == "frames") {
                const std::vector<int32_t> out = glio::globalGraphFrames(ids, a, b);
                std::printf("frames");
                for (int32_t v : out) std::printf(" %d", v);
                std::printf("\n");
            } else {
                int i, j;
                glio::loopEdgeFrames(ids, a, b, &i, &j);
                std::printf("edge %d %d\n", i, j);
            }
        } else if (cmd == "gate") {
            const double ts = num(in), g = num(in), p = num(in);
            gate.reset(new glio::GnssGate(ts, g, p));
        } else if (cmd == "push") {
            glio::GnssFix f;
            f.stamp = num(in);
            for (int k = 0; k < 3; ++k) f.xyz[k] = num(in);
            for (int k = 0; k < 3; ++k) f.cov[k] = num(in);
            gate->push(f);
        } else if (cmd == "select") {
            int n, W;
            in >> n >> W;
            double xyz[3];
            for (int k = 0; k < 3; ++k) xyz[k] = num(in);
            const double t = num(in), c33 = num(in), c44 = num(in);
            glio::GnssFactor f;
            if (gate->select(n, W, xyz, t, c33, c44, &f)) std::printf("gps %d %a %a %a %a %a %a %zu\n", f.node, f.xyz[0], f.xyz[1], f.xyz[2], f.var[0], f.var[1], f.var[2], gate->queued());
            else std::printf("none %zu\n", gate->queued());
        } else if (cmd == "dist32") {
            float a[3], b[3];
            for (int k = 0; k < 3; ++k) a[k] = (float)num(in);
            for (int k = 0; k < 3; ++k) b[k] = (float)num(in);
            std::printf("dist %a\n", glio::pointDistanceF32(a, b));
        } else if (cmd == "dist64") {
            double a[3], b[3];
            for (int k = 0; k < 3; ++k) a[k] = num(in);
            for (int k = 0; k < 3; ++k) b[k] = num(in);
            std::printf("dist %a\n", glio::pointDistanceF64(a, b));
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}

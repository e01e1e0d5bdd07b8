// host_demo_pose_graph.cpp -- a drive that revisits its start, through glio::GlobalGraph / glio::PoseGraph (glio_posegraph_backend.hpp): every keyframe call
// feeds the frames between two keyframes into the global graph (Estimator.cpp:4586-4652), some GPS fixes are attached, the loop edge is added and the graph
// solved (:5251-5261); the corrected poses are printed as hex floats.  The case file is written by glio_amd/host/window_io.py::write_pose_graph_case:
//   int32 F NK W n_gps latest_kf closest_kf 0 0 | pose_each_frame [F][7] = t, q | keyframe_id_in_frame [NK] int32 (padded to a multiple of 2) |
//   rel [7] var [6] | n_gps x (frame, xyz[3], var[3]) doubles
// usage: host_demo_pose_graph case.bin [device] [damped=1]
// damped=1: the loop is closed with glio_pgraph_solve_damped (GlobalGraph::loopClosed(..., true)); one more line, `damped accepted rejected invalid trials
// final_radius`, and one `trial k E radius m verdict` per trial are printed.  Without it the output is what it always was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

#include "glio_posegraph_backend.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s case.bin [device] [damped=1]\n", argv[0]); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const bool damped = argc > 2 && std::strcmp(argv[argc - 1], "damped=1") == 0;
    const int device = argc > (damped ? 3 : 2) ? std::atoi(argv[2]) : 0;
    int32_t h[8];
    in.read((char*)h, sizeof h);
    const int F = h[0], NK = h[1], W = h[2], n_gps = h[3], latest = h[4], closest = h[5];
    std::vector<double> frames((size_t)7 * F);
    in.read((char*)frames.data(), (std::streamsize)(frames.size() * 8));
    std::vector<int32_t> kf((size_t)NK + (NK & 1));
    in.read((char*)kf.data(), (std::streamsize)(kf.size() * 4));
    kf.resize(NK);
    double rel[7], var[6];
    in.read((char*)rel, sizeof rel); in.read((char*)var, sizeof var);
    std::vector<double> gps((size_t)7 * n_gps);
    in.read((char*)gps.data(), (std::streamsize)(gps.size() * 8));
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    try {
        glio_pgraph_opts o;
        glio_pgraph_opts_default(&o);
        o.max_nodes = F; o.max_loops = 4; o.max_unary = n_gps > 0 ? n_gps : 1;
        glio::PoseGraph graph(&o, device);
        glio::GlobalGraph global(&graph, W);
        for (int n = 1; n <= NK; ++n) {
            // the frames the estimator holds when keyframe n - 1 is handled: up to that keyframe's own frame
            std::vector<double> so_far(frames.begin(), frames.begin() + (size_t)7 * (kf[n - 1] + 1));
            const std::vector<int32_t> ids = global.keyframeCall(so_far, kf, n);
            if (!ids.empty()) std::printf("call %d frames %d .. %d\n", n, ids.front(), ids.back());
        }
        for (int k = 0; k < n_gps; ++k) graph.addGps((int)gps[(size_t)7 * k], &gps[(size_t)7 * k + 1], &gps[(size_t)7 * k + 4]);
        const double before = graph.error();
        glio_pgraph_lm_info lm = {};
        const glio_pgraph_info info = global.loopClosed(kf, latest, closest, rel, var, damped, &lm);
        std::printf("solve %d %d %a %a %a %d %d\n", info.iterations, info.termination, before, info.initial_error, info.final_error, info.separators, info.segments);
        if (damped) {
            std::printf("damped %d %d %d %d %a\n", lm.accepted, lm.rejected, lm.invalid, lm.trials, lm.final_radius);
            std::vector<double> hist((size_t)4 * lm.trials);
            if (glio_pgraph_lm_history(graph.handle(), 0, lm.trials, hist.data()) != GLIO_OK) throw std::runtime_error(glio_last_error());
            for (int k = 0; k < lm.trials; ++k) std::printf("trial %d %a %a %a %d\n", k, hist[(size_t)4 * k], hist[(size_t)4 * k + 1], hist[(size_t)4 * k + 2], (int)hist[(size_t)4 * k + 3]);
        }
        const std::vector<double> x = graph.readPoses();
        for (int i = 0; i < graph.size(); ++i) {
            std::printf("pose %d", i);
            for (int c = 0; c < 7; ++c) std::printf(" %a", x[(size_t)7 * i + c]);
            std::printf("\n");
        }
        const std::vector<double> kp = global.keyframePoses(kf, NK - W + 1);
        std::printf("keyframes %zu\n", kp.size() / 7);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "host_demo_pose_graph: %s\n", e.what());
        return 1;
    }
    return 0;
}

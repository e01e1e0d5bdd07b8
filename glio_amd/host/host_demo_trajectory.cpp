// host_demo_trajectory.cpp -- a synthetic drive through glio::Trajectory (glio_trajectory_backend.hpp) into glio::GlobalGraph (glio_posegraph_backend.hpp): every
// keyframe call fills the frames between two keyframes (Estimator.cpp:4273-4557) on the device and hands pose_each_frame to the global graph (:4586-4652); then
// every stored gap is solved again between a corrected keyframe table (Trajectory::resolveAll).  All rows are printed as hex floats.  The case file is written
// by glio_amd/host/window_io.py::write_trajectory_case:
//   int32 n_imu F NK W 0 0 0 0 | imu [n_imu][7] = stamp, acc, gyr | frame_stamps [F] | keyframe_id_in_frame [NK] int32 (padded to a multiple of 2) |
//   imu_idx_in_kf [NK] int32 (padded) | keyframe_poses [NK][7] | start_states [NK][15] (row n - 1: the state passed at call n) | corrected [NK][7]
// usage: host_demo_trajectory case.bin [device]
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "glio_posegraph_backend.hpp"
#include "glio_trajectory_backend.hpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s case.bin [device]\n", argv[0]); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const int device = argc > 2 ? std::atoi(argv[2]) : 0;
    int32_t h[8];
    in.read((char*)h, sizeof h);
    const int n_imu = h[0], F = h[1], NK = h[2], W = h[3];
    std::vector<double> imu((size_t)7 * n_imu), frame_stamps((size_t)F);
    in.read((char*)imu.data(), (std::streamsize)(imu.size() * 8));
    in.read((char*)frame_stamps.data(), (std::streamsize)(frame_stamps.size() * 8));
    std::vector<int32_t> kf((size_t)NK + (NK & 1)), idx32((size_t)NK + (NK & 1));
    in.read((char*)kf.data(), (std::streamsize)(kf.size() * 4));
    in.read((char*)idx32.data(), (std::streamsize)(idx32.size() * 4));
    std::vector<double> kposes((size_t)7 * NK), starts((size_t)15 * NK), corrected((size_t)7 * NK);
    in.read((char*)kposes.data(), (std::streamsize)(kposes.size() * 8));
    in.read((char*)starts.data(), (std::streamsize)(starts.size() * 8));
    in.read((char*)corrected.data(), (std::streamsize)(corrected.size() * 8));
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    std::vector<double> stamps((size_t)n_imu);
    std::vector<std::array<double, 3>> acc((size_t)n_imu), gyr((size_t)n_imu);
    for (int i = 0; i < n_imu; ++i) {
        stamps[i] = imu[(size_t)7 * i];
        for (int k = 0; k < 3; ++k) { acc[i][k] = imu[(size_t)7 * i + 1 + k]; gyr[i][k] = imu[(size_t)7 * i + 4 + k]; }
    }
    std::vector<size_t> imu_idx(idx32.begin(), idx32.begin() + NK);
    try {
        glio_traj_opts to;
        glio_traj_opts_default(&to);
        to.max_gaps = NK;
        glio::TrajectoryStore store(&to, device);
        glio::Trajectory traj(&store, W);
        glio_pgraph_opts o;
        glio_pgraph_opts_default(&o);
        o.max_nodes = F; o.max_loops = 1; o.max_unary = 1;
        glio::PoseGraph graph(&o, device);
        glio::GlobalGraph global(&graph, W);
        for (int n = 1; n <= NK; ++n) {
            const std::vector<double> table(kposes.begin(), kposes.begin() + (size_t)7 * n);
            const std::vector<double> fs(frame_stamps.begin(), frame_stamps.begin() + kf[n - 1] + 1);
            const int gap = traj.keyframeCall(kf[n - 1], table, fs, stamps, acc, gyr, imu_idx, &starts[(size_t)15 * (n - 1)]);
            const std::vector<int32_t> ids = global.keyframeCall(traj.poses(), traj.keyframeIdInFrame(), n);
            if (gap >= 0) {
                glio_traj_summary s;
                store.readSolved(gap, &s);
                std::printf("call %d gap %d frames %d termination %d iterations %d\n", n, gap, s.n_frames, s.termination, s.iterations);
            }
            if (!ids.empty()) std::printf("graph %d frames %d .. %d\n", n, ids.front(), ids.back());
        }
        const std::vector<double> rows = traj.poses();
        for (size_t i = 0; i < rows.size() / 7; ++i) {
            std::printf("frame %zu", i);
            for (int c = 0; c < 7; ++c) std::printf(" %a", rows[7 * i + c]);
            std::printf("\n");
        }
        const std::vector<double> x = graph.readPoses();
        for (int i = 0; i < graph.size(); ++i) {
            std::printf("node %d", i);
            for (int c = 0; c < 7; ++c) std::printf(" %a", x[(size_t)7 * i + c]);
            std::printf("\n");
        }
        const std::vector<glio_traj_summary> summ = traj.resolveAll(corrected);
        for (size_t k = 0; k < summ.size(); ++k) std::printf("resolve %zu termination %d iterations %d\n", k, summ[k].termination, summ[k].iterations);
        const std::vector<double> again = traj.poses();
        for (size_t i = 0; i < again.size() / 7; ++i) {
            std::printf("resolved %zu", i);
            for (int c = 0; c < 7; ++c) std::printf(" %a", again[7 * i + c]);
            std::printf("\n");
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "host_demo_trajectory: %s\n", e.what());
        return 1;
    }
    return 0;
}

// host_demo_map_schedule.cpp -- the reference's local-map schedule (buildLocalMapWithLandMark, Estimator.cpp:3545-3616, with correctPoses' clear of the deque,
// :4660) driven from C++ through glio::SlidingWindowBackend: per keyframe call the new scan enters window slot W - 1 and the batch association's store, then the
// backend asks glio::localMapPlan and either rebuilds the ring from the resident keyframes at the poses pose_info_keyframe holds in THAT call
// (glio_localmap_rebuild_from_frames) or pushes the newest scan.  Input: a flat file written by window_io.write_map_schedule; output: a flat file of the map
// after every call (action, frame list, points) -- tests/test_hip_localmap_rebuild.py holds it against the Python driver and the oracle.
// A fifth argument `arm` makes the loop closure also arm the speed-bias priors of the next window (armSpeedBiasPriors, correctPoses' marg = false); the
// fourth word of every call's record then says whether they are armed (this program solves nothing: host_demo's `arm` runs such a window).
// Build: g++ -std=c++14 -O2 host_demo_map_schedule.cpp -I../../include -L../lib -lglio_hip -Wl,-rpath,'$ORIGIN/../lib'
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "glio_backend.hpp"
#include "glio_batch_backend.hpp"

template <typename T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
template <typename T> static void wr(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short write\n"); exit(2); } }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: host_demo_map_schedule schedule.bin maps.bin [device [arm]]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    const int device = argc > 3 ? atoi(argv[3]) : 0;
    const bool arm = argc > 4 && std::string(argv[4]) == "arm";
    glio_opts opts;
    rd(f, &opts, 1);
    int32_t hdr[8];            // n_keyframes, points per scan (capacity), local-map width, keyframe after whose call the loop closes (-1: never), accumulation, 0 0 0
    rd(f, hdr, 8);
    float leaf, tlb[3];
    double q_bl[4], t_bl[3];
    rd(f, &leaf, 1); rd(f, tlb, 3); rd(f, q_bl, 4); rd(f, t_bl, 3);
    const int W = opts.window, NK = hdr[0], cap = hdr[1], width = hdr[2], loop_after = hdr[3];
    std::vector<std::vector<float>> scans(NK);
    for (int j = 0; j < NK; ++j) { int32_t n; rd(f, &n, 1); scans[j].resize((size_t)n * 4); rd(f, scans[j].data(), scans[j].size()); }
    std::vector<double> pose_info((size_t)NK * NK * 7);      // [call][keyframe][7] = t_po, q_po: pose_info_keyframe as the call finds it
    rd(f, pose_info.data(), pose_info.size());
    fclose(f);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror("open output"); return 2; }
    try {
        glio::SlidingWindowBackend be(opts, device);
        be.configureLocalMap(width, leaf, cap);
        if (hdr[4]) glio::check(glio_localmap_set_accumulation(be.ctx(), hdr[4]), "glio_localmap_set_accumulation");
        be.enableReferenceMapSchedule(width, q_bl, t_bl);
        glio::BatchAssociationBackend ba(NK, cap, 16, device);
        std::vector<float> map;
        for (int j = 0; j < NK; ++j) {
            if (j > 0) be.slideWindow();
            be.setScan(W - 1, scans[j].data(), (int)(scans[j].size() / 4));
            ba.setFrameFromScan(j, be.ctx(), W - 1, tlb);
            const bool rebuilds = be.nextLocalMapCallRebuilds(j + 1);
            const int action = be.updateLocalMapByReferenceSchedule(ba.handle(), j + 1, &pose_info[(size_t)j * NK * 7], W - 1, tlb);
            if (rebuilds != (action == glio::MAP_REBUILD)) { fprintf(stderr, "plan changed between question and call\n"); return 1; }
            int n = 0;
            glio::check(glio_localmap_read(be.ctx(), nullptr, 0, &n), "glio_localmap_read");
            map.assign((size_t)(n > 0 ? n : 1) * 4, 0.f);
            glio::check(glio_localmap_read(be.ctx(), map.data(), n, &n), "glio_localmap_read");
            if (j == loop_after) { be.loopClosed(); if (arm) be.armSpeedBiasPriors(); }
            const int32_t rec[4] = {action, be.mapPoints(), n, be.speedBiasPriorsArmed() ? 1 : 0};
            wr(out, rec, 4); wr(out, map.data(), (size_t)n * 4);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    fclose(out);
    return 0;
}

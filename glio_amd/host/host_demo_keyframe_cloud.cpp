// host_demo_keyframe_cloud.cpp -- the hand-over of the keyframes' surf clouds from the front end to the sliding window, driven from C++: a raw-scan drive through
// glio::ScanToMapOdometry::runRaw, the keyframe rule (glio::KeyframeGate, LidarOdometry.cpp:566-578) and, for every keyframe, the cloud de-skewed and filtered on
// the device into a window slot twice -- from the front end's resident surf features (SlidingWindowBackend::setScanFromFrontEnd: no byte crosses PCIe) and
// from the same features read back and sent up again (setScanFiltered: the drop-in Estimator's route).  Input: the flat file of
// glio_amd/host/window_io.py::write_frontend_raw_stream.  Output: per scan `scan i kf surf` and per keyframe `kf i slot n_resident hash_resident n_host
// hash_host` (FNV-1a over the slot's bytes as glio_get_scan returns them) -- tests/test_hip_keyframe_cloud_hosts.py compares them with the Python twin.
// Build: g++ -std=c++14 -O2 host_demo_keyframe_cloud.cpp -I../../include -L../lib -lglio_hip -Wl,-rpath,'$ORIGIN/../lib'
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_backend.hpp"

template <typename T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
static unsigned long long fnv1a(const std::vector<float>& v) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_keyframe_cloud stream.bin [device] [leaf=0.9] [deskew=1] [window=3]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    float leaf = 0.9f;                   // surfDSRange (config_urban_hk.yaml:69)
    bool deskew = true;                  // if_to_deskew: the code's default (the released yaml sets false)
    int W = 3;
    for (int a = 3; a < argc; ++a) {
        if (!strncmp(argv[a], "leaf=", 5)) leaf = (float)atof(argv[a] + 5);
        else if (!strncmp(argv[a], "deskew=", 7)) deskew = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "window=", 7)) W = atoi(argv[a] + 7);
        else { fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
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
        glio_opts wopts;
        glio_opts_default(&wopts);
        wopts.window = W; wopts.max_points_per_scan = opts.max_points_per_scan; wopts.max_map_points = 64;
        glio::SlidingWindowBackend be(wopts, device), host(wopts, device);
        be.configureScanFilter(opts.max_points_per_scan);
        host.configureScanFilter(opts.max_points_per_scan);
        glio::KeyframeGate gate;
        int n_kf = 0;
        for (int i = 0; i < n_scans; ++i) {
            glio_feat_counts cnt;
            odo.runRaw(scans[i].data(), ns[i], layout, qs[i].data(), nullptr, &cnt);
            const bool kf = gate.update(odo);
            printf("scan %d %d %d\n", i, kf ? 1 : 0, cnt.surf);
            if (!kf) continue;
            const int slot = n_kf++ % W;
            // the resident route ...
            const int n_res = be.setScanFromFrontEnd(slot, odo, leaf, deskew);
            // ... and the host route: the features read back, de-skewed and filtered on their way up again
            std::vector<float> surf((size_t)cnt.surf * 4 + 4);
            int got = 0;
            glio::check(glio_features_read(odo.ctx(), GLIO_FEAT_SURF, surf.data(), cnt.surf, &got), "glio_features_read");
            const int n_host = host.setScanFiltered(slot, surf.data(), got, leaf, deskew ? &odo.rel_pose[4] : nullptr);
            printf("kf %d %d %d %llu %d %llu\n", i, slot, n_res, fnv1a(be.getScan(slot)), n_host, fnv1a(host.getScan(slot)));
        }
        printf("{\"scans\": %d, \"keyframes\": %d, \"leaf\": %.9g, \"deskew\": %d}\n", n_scans, n_kf, (double)leaf, deskew ? 1 : 0);
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

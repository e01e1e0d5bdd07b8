// host_demo_dense_map.cpp -- the dense map driven from C++: a raw-scan drive through glio::ScanToMapOdometry::runRaw, the keyframe rule (glio::KeyframeGate,
// LidarOdometry.cpp:566-578) and, for every keyframe, the front end's CUT cloud de-skewed by rel_pose's translation (LidarOdometry.cpp:626) and filtered at 0.4 m
// into a frame of glio::DenseClouds (full_clouds_ds, Estimator.cpp:3623-3626) -- on the store's own stream, no byte crosses PCIe -- then publishCompleteMap
// (:5275-5313): the frames at their keyframes' poses (glio::loopFramePoses, :5287-5288) added to a glio::GlobalMap on the store in chunks.  Input: the flat file
// of glio_amd/host/window_io.py::write_frontend_raw_stream.  Output: per scan `scan i kf cut`, per keyframe `kf i k n hash` (FNV-1a over the frame's bytes) and
// `map n_voxels hash n_points frames` -- tests/test_hip_dense_map_hosts.py compares them with the Python twin.
// Build: g++ -std=c++14 -O2 host_demo_dense_map.cpp -I../../include -L../lib -lglio_hip -Wl,-rpath,'$ORIGIN/../lib'
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_backend.hpp"
#include "glio_loop_backend.hpp"
#include "glio_map_backend.hpp"

template <typename T> static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }
static unsigned long long fnv1a(const std::vector<float>& v, unsigned long long h = 1469598103934665603ull) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_dense_map stream.bin [device] [leaf=0.4] [map_leaf=0.2] [chunk=2] [deskew=1]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    float leaf = 0.4f, map_leaf = 0.2f;          // ds_filter_surf_map (Estimator.cpp:854), ds_filter_global_map (:856)
    int chunk = 2;
    bool deskew = true;
    for (int a = 3; a < argc; ++a) {
        if (!strncmp(argv[a], "leaf=", 5)) leaf = (float)atof(argv[a] + 5);
        else if (!strncmp(argv[a], "map_leaf=", 9)) map_leaf = (float)atof(argv[a] + 9);
        else if (!strncmp(argv[a], "chunk=", 6)) chunk = atoi(argv[a] + 6);
        else if (!strncmp(argv[a], "deskew=", 7)) deskew = atoi(argv[a] + 7) != 0;
        else { fprintf(stderr, "unknown argument %s\n", argv[a]); return 2; }
    }
    if (chunk < 1) chunk = 1;
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
        glio::DenseClouds dense(n_scans > 0 ? n_scans : 1, fopts.max_raw_points, fopts.max_raw_points, device);
        glio::KeyframeGate gate;
        std::vector<double> pose_info;            // t_po, q_po of every keyframe
        int n_kf = 0;
        for (int i = 0; i < n_scans; ++i) {
            glio_feat_counts cnt;
            odo.runRaw(scans[i].data(), ns[i], layout, qs[i].data(), nullptr, &cnt);
            const bool kf = gate.update(odo);
            printf("scan %d %d %d\n", i, kf ? 1 : 0, cnt.cut);
            if (!kf) continue;
            const int k = n_kf++;
            const int n = dense.setFrameFromFeatures(k, odo.ctx(), leaf, deskew ? &odo.rel_pose[4] : nullptr);
            for (int c = 0; c < 3; ++c) pose_info.push_back(odo.abs_pose[4 + c]);
            for (int c = 0; c < 4; ++c) pose_info.push_back(odo.abs_pose[c]);
            printf("kf %d %d %d %llu\n", i, k, n, fnv1a(dense.readFrame(k)));
        }
        // publishCompleteMap: every keyframe, in chunks (extrinsics: the identity, as the front end's q_lb)
        glio_gmap_opts mo;
        glio_gmap_opts_default(&mo);
        mo.leaf = map_leaf;
        glio::GlobalMap gm(dense, &mo);
        const double qbl[4] = {1.0, 0.0, 0.0, 0.0}, tbl[3] = {0.0, 0.0, 0.0};
        glio_gmap_info last;
        memset(&last, 0, sizeof last);
        for (int a = 0; a < n_kf; a += chunk) {
            const int b = a + chunk < n_kf ? a + chunk : n_kf;
            std::vector<int32_t> part;
            for (int k = a; k < b; ++k) part.push_back(k);
            std::vector<double> poses((size_t)7 * part.size());
            glio::loopFramePoses(pose_info.data() + 7 * a, (int)part.size(), qbl, tbl, poses.data());
            last = gm.add(part, poses);
        }
        unsigned long long h = 1469598103934665603ull;
        const int nv = gm.size();
        for (int first = 0; first < nv; first += 1000) h = fnv1a(gm.read(first, nv - first < 1000 ? nv - first : 1000), h);
        printf("map %d %llu %lld %d\n", nv, h, (long long)last.n_points_total, n_kf);
        printf("{\"scans\": %d, \"keyframes\": %d, \"leaf\": %.9g, \"map_leaf\": %.9g, \"deskew\": %d}\n", n_scans, n_kf, (double)leaf, (double)map_leaf, deskew ? 1 : 0);
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

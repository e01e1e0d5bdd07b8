// host_demo_static_map -- the static map's call sequence in C++ over glio::StaticClouds (glio_static_backend.hpp): full clouds into a dense store, the views
// glio::staticViews picks, one classification of all frames, the map of the static store.  Reads a case file written by
// glio_amd/host/window_io.py::write_static_map_case:
//   int32 K cap half_window 0 | glio_static_opts | glio_gmap_opts | double min_baseline
//   | K x (int32 n, float [n][4])            the frames' clouds
//   | double poses[K][7]
// and prints the results' bytes in hex for tests/test_hip_static_map_hosts.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_static_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }
static void hex(const char* name, const void* p, size_t bytes) {
    printf("%s ", name);
    for (size_t i = 0; i < bytes; ++i) printf("%02x", ((const unsigned char*)p)[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_static_map case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    glio_static_opts opts;
    glio_gmap_opts gopts;
    double min_baseline;
    rd(f, head, 4); rd(f, &opts, 1); rd(f, &gopts, 1); rd(f, &min_baseline, 1);
    const int K = head[0], cap = head[1], half_window = head[2];
    try {
        glio::DenseClouds dense(K, cap, cap, device);
        std::vector<float> buf;
        for (int k = 0; k < K; ++k) {
            int32_t n; rd(f, &n, 1);
            buf.resize((size_t)n * 4); rd(f, buf.data(), buf.size());
            dense.setFrame(k, buf.data(), n, 16, 12, 0.f, nullptr, nullptr);            // (leaf 0: the cloud as it is)
        }
        std::vector<double> poses((size_t)7 * K);
        rd(f, poses.data(), poses.size());
        fclose(f);
        std::vector<int32_t> frames((size_t)K), off, views;
        for (int k = 0; k < K; ++k) frames[k] = k;
        glio::staticViews(poses, half_window, min_baseline, &off, &views);
        hex("view_offsets", off.data(), off.size() * 4);
        hex("views", views.data(), views.size() * 4);
        glio::StaticClouds st(dense, &opts);
        const glio_static_info info = st.classify(frames, poses, off, views);
        hex("info", &info, sizeof info);
        std::vector<uint8_t> th, te;
        std::vector<float> raw, fl;
        char name[32];
        for (int k = 0; k < K; ++k) {
            const std::vector<float> fr = st.readFrame(k);
            snprintf(name, sizeof name, "frame%d", k); hex(name, fr.data(), fr.size() * 4);
            st.readVotes(k, &th, &te);
            snprintf(name, sizeof name, "through%d", k); hex(name, th.data(), th.size());
            snprintf(name, sizeof name, "tested%d", k); hex(name, te.data(), te.size());
        }
        st.readImage(K - 1, &raw, &fl);
        hex("floor", fl.data(), fl.size() * 4);
        glio::GlobalMap gm(st.handle(), &gopts);
        const glio_gmap_info gi = gm.add(frames, poses);
        printf("voxels %08x\n", (unsigned)gi.n_voxels);
        const std::vector<float> vox = gm.read();
        hex("map", vox.data(), vox.size() * 4);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

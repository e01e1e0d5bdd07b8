// host_demo_place -- place recognition's call sequence in C++ over glio::PlaceRecognition (glio_place_backend.hpp): keyframe clouds into a batch association,
// their descriptors in one call (each with the levelling quaternion of its attitude), every place queried against the earlier ones, the appearance rule and
// the initial guess for the last place.  Reads a case file written by glio_amd/host/window_io.py::write_place_case:
//   int32 K cap top_k 0 | glio_place_opts | double min_time_gap
//   | K x (int32 n, float [n][4])            keyframe clouds
//   | double times[K] | double attitude[K][4] | double pose_closest[7]
// and prints the results' bytes in hex for tests/test_hip_place_hosts.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_place_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }
static void hex(const char* name, const void* p, size_t bytes) {
    printf("%s ", name);
    for (size_t i = 0; i < bytes; ++i) printf("%02x", ((const unsigned char*)p)[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_place case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    glio_place_opts opts;
    double gap;
    rd(f, head, 4); rd(f, &opts, 1); rd(f, &gap, 1);
    const int K = head[0], cap = head[1], top_k = head[2];
    try {
        glio_bassoc* ba = nullptr;
        if (glio_bassoc_create(device, K, cap, 1, &ba) != GLIO_OK) { fprintf(stderr, "glio_bassoc_create: %s\n", glio_last_error()); return 1; }
        std::vector<float> buf;
        for (int k = 0; k < K; ++k) {
            int32_t n; rd(f, &n, 1);
            buf.resize((size_t)n * 4); rd(f, buf.data(), buf.size());
            if (n > 0 && glio_bassoc_set_frame(ba, k, buf.data(), n) != GLIO_OK) { fprintf(stderr, "glio_bassoc_set_frame: %s\n", glio_last_error()); return 1; }
        }
        std::vector<double> times((size_t)K), att((size_t)4 * K), level((size_t)4 * K);
        double pose_closest[7];
        rd(f, times.data(), times.size()); rd(f, att.data(), att.size()); rd(f, pose_closest, 7);
        fclose(f);
        {
            glio::PlaceRecognition pr(ba, &opts);
            std::vector<int32_t> idx((size_t)K);
            for (int k = 0; k < K; ++k) { idx[k] = k; glio::levelingQuaternion(&att[4 * k], &level[4 * k]); }
            pr.addFrames(idx, idx, times, level);
            hex("level", level.data(), level.size() * 8);
            for (int k = 0; k < K; ++k) {
                const glio::PlaceRecognition::Descriptor d = pr.readDescriptor(k);
                char name[32]; snprintf(name, sizeof name, "heights%d", k);
                hex(name, d.heights.data(), d.heights.size() * 4);
                printf("mask%d %llx\n", k, (unsigned long long)d.mask);
            }
            std::vector<glio_place_match> many; std::vector<int32_t> nf;
            pr.queryMany(0, K, gap, true, top_k, &many, &nf);
            hex("many", many.data(), many.size() * sizeof(glio_place_match));
            hex("n_found", nf.data(), nf.size() * 4);
            const std::vector<glio_place_match> one = pr.query(K - 1, gap, top_k);
            hex("query", one.data(), one.size() * sizeof(glio_place_match));
            const glio::PlaceCandidate c = glio::detectCandidateByAppearance(pr, K - 1, gap, times[K - 1], -1.0);
            printf("candidate %d\n", c.closest);
            const double cy[2] = {c.yaw, c.distance};
            hex("candidate_yaw_distance", cy, 16);
            double guess[14];
            glio::placeInitialGuess(pose_closest, c.yaw, nullptr, guess);
            glio::placeInitialGuess(pose_closest, c.yaw, &att[4 * (K - 1)], guess + 7);
            hex("guess", guess, sizeof guess);
        }
        glio_bassoc_destroy(ba);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

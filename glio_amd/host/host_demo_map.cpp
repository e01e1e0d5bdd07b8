// host_demo_map -- the global map's call sequence in C++ over glio::GlobalMap (glio_map_backend.hpp): keyframe clouds into a batch association, the keyframes of
// glio::globalMapFrames at their composed poses added in chunks, the map read back in ranges.  Reads a case file written by
// glio_amd/host/window_io.py::write_map_case:
//   int32 K cap mapping_interval chunk_frames 0 0 0 0 | glio_gmap_opts
//   | K x (int32 n, float [n][4])            keyframe clouds
//   | double pose_info[K][7]                 t_po, q_po of every keyframe
//   | double q_bl[4], t_bl[3]
// and prints sizes and a checksum of the map's words for tests/test_hip_global_map.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_loop_backend.hpp"
#include "glio_map_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_map case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    glio_gmap_opts opts;
    rd(f, head, 8); rd(f, &opts, 1);
    const int K = head[0], cap = head[1], interval = head[2], chunk = head[3] > 0 ? head[3] : 1;
    try {
        glio_bassoc* ba = nullptr;
        if (glio_bassoc_create(device, K, cap, 1, &ba) != GLIO_OK) { fprintf(stderr, "glio_bassoc_create: %s\n", glio_last_error()); return 1; }
        std::vector<float> buf;
        for (int k = 0; k < K; ++k) {
            int32_t n; rd(f, &n, 1);
            buf.resize((size_t)n * 4); rd(f, buf.data(), buf.size());
            if (n > 0 && glio_bassoc_set_frame(ba, k, buf.data(), n) != GLIO_OK) { fprintf(stderr, "glio_bassoc_set_frame: %s\n", glio_last_error()); return 1; }
        }
        std::vector<double> info((size_t)7 * K);
        double qbl[4], tbl[3];
        rd(f, info.data(), info.size()); rd(f, qbl, 4); rd(f, tbl, 3);
        fclose(f);
        {
            glio::GlobalMap gm(ba, &opts);
            const std::vector<int32_t> frames = glio::globalMapFrames(K, interval);
            glio_gmap_info last;
            memset(&last, 0, sizeof last);
            double ms = 0.0;
            for (size_t a = 0; a < frames.size(); a += (size_t)chunk) {
                const size_t b = a + (size_t)chunk < frames.size() ? a + (size_t)chunk : frames.size();
                const std::vector<int32_t> part(frames.begin() + a, frames.begin() + b);
                std::vector<double> pinfo, poses((size_t)7 * part.size());
                for (int32_t k : part) pinfo.insert(pinfo.end(), info.begin() + 7 * k, info.begin() + 7 * k + 7);
                glio::loopFramePoses(pinfo.data(), (int)part.size(), qbl, tbl, poses.data());
                last = gm.add(part, poses);
                ms += gm.lastDeviceMs();
            }
            // read back in ranges of 1000 voxels, FNV-1a over the 32-bit words
            unsigned long long h = 1469598103934665603ull;
            const int nv = gm.size();
            for (int first = 0; first < nv; first += 1000) {
                const std::vector<float> part = gm.read(first, nv - first < 1000 ? nv - first : 1000);
                for (float x : part) { uint32_t u; memcpy(&u, &x, 4); h = (h ^ u) * 1099511628211ull; }
            }
            printf("map %d %llx %lld %d %d %zu\n", nv, h, (long long)last.n_points_total, last.radix_passes, last.pcl_index_overflow, frames.size());
            printf("{\"add_device_ms\": %.4f}\n", ms);
        }
        glio_bassoc_destroy(ba);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

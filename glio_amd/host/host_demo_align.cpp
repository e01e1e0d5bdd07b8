// host_demo_align -- the GNSS frame estimate's call sequence in C++ over glio::GnssAlignment (glio_align_backend.hpp).  Reads a case file written by
// glio_amd/host/window_io.py::write_align_case:
//   int32 n_dd n_pos stride 0 | glio_align_opts | glio_gnss_frame start | glio_dd_psr [n_dd] | double positions [n_pos][stride]
// and prints the result's words in hex for tests/test_hip_gnss_align_hosts.py: the frame, the info record, the search's costs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_align_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

static void hex(const char* name, const void* p, size_t bytes) {
    printf("%s ", name);
    for (size_t k = 0; k < bytes; ++k) printf("%02x", ((const unsigned char*)p)[k]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_align case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    glio_align_opts opts;
    glio_gnss_frame start;
    rd(f, head, 4); rd(f, &opts, 1); rd(f, &start, 1);
    const int n_dd = head[0], n_pos = head[1], stride = head[2];
    std::vector<glio_dd_psr> dd((size_t)n_dd);
    std::vector<double> pos((size_t)n_pos * stride);
    rd(f, dd.data(), dd.size()); rd(f, pos.data(), pos.size());
    fclose(f);
    try {
        glio::GnssAlignment al(n_dd, n_pos, device);
        al.setOpts(opts);
        al.setFactors(dd);
        al.setPositions(pos.data(), n_pos, stride);
        const glio::GnssAlignment::Result r = al.solve(start);
        hex("frame", &r.frame, sizeof r.frame);
        hex("info", &r.info, sizeof r.info);
        if (opts.n_hypotheses > 0) {
            const std::vector<double> c = al.readCoarse();
            hex("coarse", c.data(), c.size() * 8);
        }
        const float solve_ms = al.lastDeviceMs();
        int32_t nd = 0;
        const double c6 = al.cost(r.frame, opts.thresholds[opts.n_rounds - 1], &nd);
        hex("cost", &c6, 8);
        printf("status %d rows %d downweighted %d\n", r.info.status, r.info.n_rows, nd);
        printf("{\"solve_device_ms\": %.4f}\n", solve_ms);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

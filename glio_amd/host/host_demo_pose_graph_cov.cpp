// host_demo_pose_graph_cov -- the covariance of every node of a pose graph in C++ over glio::PoseGraph::marginalCovariances (glio_posegraph_backend.hpp).
// Reads a case file written by glio_amd/host/window_io.py::write_pose_graph_cov_case:
//   int32 N n_loops n_gps segment_nodes prior solve 0 0 | double poses [N][7] = t, q | n_loops x (i, j, rel [7], var [6]) doubles |
//   n_gps x (node, xyz [3], var [3]) doubles
// builds the graph (prior on node 0 when `prior`), solves it when `solve`, and prints the blocks' words in hex for tests/test_hip_pose_graph_cov_hosts.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "glio_posegraph_backend.hpp"

static void rd(FILE* f, void* p, size_t size, size_t n) { if (n && fread(p, size, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

static void hex(const char* name, const void* p, size_t bytes) {
    printf("%s ", name);
    for (size_t k = 0; k < bytes; ++k) printf("%02x", ((const unsigned char*)p)[k]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_pose_graph_cov case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    rd(f, head, 4, 8);
    const int N = head[0], n_loops = head[1], n_gps = head[2], segment_nodes = head[3], prior = head[4], solve = head[5];
    std::vector<double> poses((size_t)N * 7), loops((size_t)n_loops * 15), gps((size_t)n_gps * 7);
    rd(f, poses.data(), 8, poses.size()); rd(f, loops.data(), 8, loops.size()); rd(f, gps.data(), 8, gps.size());
    fclose(f);
    try {
        glio_pgraph_opts o;
        glio_pgraph_opts_default(&o);
        o.max_nodes = N; o.max_loops = n_loops > 0 ? n_loops : 1; o.max_unary = n_gps > 0 ? n_gps : 1; o.segment_nodes = segment_nodes;
        glio::PoseGraph pg(&o, device);
        if (prior) pg.setPrior(poses.data());
        pg.append(N, poses.data());
        for (int l = 0; l < n_loops; ++l) pg.addBetween((int)loops[(size_t)15 * l], (int)loops[(size_t)15 * l + 1], &loops[(size_t)15 * l + 2], &loops[(size_t)15 * l + 9]);
        for (int g = 0; g < n_gps; ++g) pg.addGps((int)gps[(size_t)7 * g], &gps[(size_t)7 * g + 1], &gps[(size_t)7 * g + 4]);
        if (solve) pg.solve();
        std::vector<double> next;
        glio_pgraph_cov_info info;
        const std::vector<double> diag = pg.marginalCovariances(&next, &info);
        hex("diag", diag.data(), diag.size() * 8);
        hex("next", next.data(), next.size() * 8);
        hex("info", &info, sizeof info);
        printf("nodes %d separators %d full_row_separators %d bad_node %d\n", info.n_nodes, info.separators, info.full_row_separators, info.bad_node);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

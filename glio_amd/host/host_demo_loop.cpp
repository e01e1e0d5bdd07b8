// host_demo_loop -- the loop-closure call sequence in C++ over glio::LoopClosure (glio_loop_backend.hpp): keyframe clouds into a batch association,
// the two submaps from them (or two ready clouds), the alignment, the constraint.  Reads a case file written by glio_amd/host/window_io.py::write_loop_case:
//   int32 K cap n_src_frames n_tgt_frames n_src_points n_tgt_points 0 0 | glio_loop_opts | icp_thres (double)
//   | K x (int32 n, float [n][4])                        keyframe clouds
//   | int32 src_frames[], double src_pose_info[][7]      t_po, q_po of the listed keyframes
//   | int32 tgt_frames[], double tgt_pose_info[][7]
//   | double q_bl[4], t_bl[3]
//   | float src_points[][4], tgt_points[][4]             ready submaps (used when the frame lists are empty)
// and prints everything with exact (hexadecimal / bit pattern) numbers for tests/test_hip_loop.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "glio_loop_backend.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) { if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }
static unsigned long long checksum(const std::vector<float>& v) {
    unsigned long long h = 1469598103934665603ull;
    for (float x : v) { uint32_t u; memcpy(&u, &x, 4); h = (h ^ u) * 1099511628211ull; }
    return h;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_demo_loop case.bin [device]\n"); return 2; }
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    glio_loop_opts opts;
    double icp_thres;
    rd(f, head, 8); rd(f, &opts, 1); rd(f, &icp_thres, 1);
    const int K = head[0], cap = head[1], nsf = head[2], ntf = head[3], nsp = head[4], ntp = head[5];
    try {
        glio_bassoc* ba = nullptr;
        if (glio_bassoc_create(device, K, cap, 1, &ba) != GLIO_OK) { fprintf(stderr, "glio_bassoc_create: %s\n", glio_last_error()); return 1; }
        std::vector<float> buf;
        for (int k = 0; k < K; ++k) {
            int32_t n; rd(f, &n, 1);
            buf.resize((size_t)n * 4); rd(f, buf.data(), buf.size());
            if (n > 0 && glio_bassoc_set_frame(ba, k, buf.data(), n) != GLIO_OK) { fprintf(stderr, "glio_bassoc_set_frame: %s\n", glio_last_error()); return 1; }
        }
        std::vector<int32_t> sf((size_t)nsf), tf((size_t)ntf);
        std::vector<double> sp((size_t)7 * nsf), tp((size_t)7 * ntf), sposes((size_t)7 * nsf), tposes((size_t)7 * ntf);
        double qbl[4], tbl[3];
        rd(f, sf.data(), sf.size()); rd(f, sp.data(), sp.size()); rd(f, tf.data(), tf.size()); rd(f, tp.data(), tp.size()); rd(f, qbl, 4); rd(f, tbl, 3);
        std::vector<float> spts((size_t)4 * nsp), tpts((size_t)4 * ntp);
        rd(f, spts.data(), spts.size()); rd(f, tpts.data(), tpts.size());
        fclose(f);
        {
            glio::LoopClosure lc(ba, &opts);
            if (nsf > 0) { glio::loopFramePoses(sp.data(), nsf, qbl, tbl, sposes.data()); lc.buildSubmap(GLIO_LOOP_SOURCE, sf, sposes); }
            else lc.setSubmap(GLIO_LOOP_SOURCE, spts.data(), nsp);
            if (ntf > 0) { glio::loopFramePoses(tp.data(), ntf, qbl, tbl, tposes.data()); lc.buildSubmap(GLIO_LOOP_TARGET, tf, tposes); }
            else lc.setSubmap(GLIO_LOOP_TARGET, tpts.data(), ntp);
            const std::vector<float> s = lc.readSubmap(GLIO_LOOP_SOURCE), t = lc.readSubmap(GLIO_LOOP_TARGET);
            printf("submap %zu %llx %zu %llx\n", s.size() / 4, checksum(s), t.size() / 4, checksum(t));
            const glio_loop_result r = lc.align();
            printf("result %d %d %d %d %d %a %a\n", r.converged, r.state, r.iterations, r.last_n_corr, r.rank_deficient, r.fitness, r.last_mse);
            printf("transform");
            for (float v : r.transform) { uint32_t u; memcpy(&u, &v, 4); printf(" %08x", u); }
            printf("\n");
            double rel[7], var[6];
            const double* pl = nsf > 0 ? sp.data() : nullptr;       // pose_info of the latest keyframe = the first of the source list
            const double* pc = ntf > 0 ? tp.data() + 7 * (ntf / 2) : nullptr;
            if (pl && pc && glio::loopConstraint(r, pl, pc, icp_thres, rel, var)) {
                printf("constraint");
                for (double v : rel) printf(" %a", v);
                printf(" %a\n", var[0]);
            } else printf("constraint none\n");
            printf("{\"align_device_ms\": %.4f}\n", (double)lc.lastDeviceMs());
        }
        glio_bassoc_destroy(ba);
    } catch (const std::exception& e) { fprintf(stderr, "%s\n", e.what()); return 1; }
    return 0;
}

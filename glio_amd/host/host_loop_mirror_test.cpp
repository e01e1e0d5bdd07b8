// Host-only check of glio_loop_backend.hpp's mirrors of the loop thread (no device, no library): reads one command from stdin, prints the result with
// hexadecimal floats; tests/test_loop_host_cpu.py compares it with glio_amd/loop.py bit for bit.
//   detect n radius time_thres time_new_odom time_last_loop sx sy sz, then n rows x y z time
//   frames n_keyframes slide_window_width closest lc_map_width
//   poses n q_bl[4] t_bl[3], then n rows t[3] q[4]
//   constraint converged fitness icp_thres transform[16] pose_latest[7] pose_closest[7]
#include <cstdio>
#include <cstring>
#include <vector>

#include "glio_loop_backend.hpp"

static double rd() { double v = 0; if (scanf("%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main() {
    char cmd[32];
    if (scanf("%31s", cmd) != 1) return 2;
    if (!strcmp(cmd, "detect")) {
        const int n = (int)rd();
        const double radius = rd(), time_thres = rd(), t_new = rd(), t_last = rd();
        const float sp[3] = {(float)rd(), (float)rd(), (float)rd()};
        std::vector<float> pos((size_t)3 * n); std::vector<double> times((size_t)n);
        for (int i = 0; i < n; ++i) { for (int c = 0; c < 3; ++c) pos[3 * i + c] = (float)rd(); times[i] = rd(); }
        printf("closest %d\n", glio::detectLoopCandidate(pos.data(), times.data(), n, sp, t_new, t_last, radius, time_thres));
    } else if (!strcmp(cmd, "frames")) {
        const int n = (int)rd(), W = (int)rd(), closest = (int)rd(), w = (int)rd();
        int latest = 0; std::vector<int32_t> s, t;
        glio::loopSubmapFrames(n, W, closest, w, &latest, s, t);
        printf("latest %d\nsrc", latest);
        for (int v : s) printf(" %d", v);
        printf("\ntgt");
        for (int v : t) printf(" %d", v);
        printf("\n");
    } else if (!strcmp(cmd, "poses")) {
        const int n = (int)rd();
        double qbl[4], tbl[3];
        for (double& v : qbl) v = rd();
        for (double& v : tbl) v = rd();
        std::vector<double> in((size_t)7 * n), out((size_t)7 * n);
        for (double& v : in) v = rd();
        glio::loopFramePoses(in.data(), n, qbl, tbl, out.data());
        for (int k = 0; k < n; ++k) { printf("pose"); for (int c = 0; c < 7; ++c) printf(" %a", out[7 * k + c]); printf("\n"); }
    } else if (!strcmp(cmd, "constraint")) {
        glio_loop_result r;
        memset(&r, 0, sizeof r);
        r.converged = (int)rd(); r.fitness = rd();
        const double thres = rd();
        for (float& v : r.transform) v = (float)rd();
        double pl[7], pc[7], rel[7], var[6];
        for (double& v : pl) v = rd();
        for (double& v : pc) v = rd();
        const bool ok = glio::loopConstraint(r, pl, pc, thres, rel, var);
        printf("ok %d\n", ok ? 1 : 0);
        if (ok) { printf("rel"); for (double v : rel) printf(" %a", v); printf("\nvar"); for (double v : var) printf(" %a", v); printf("\n"); }
    } else return 2;
    return 0;
}

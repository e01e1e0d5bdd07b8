// host_tr_math_test.cpp -- glio_amd/csrc/tr_math.h compiled by a plain host compiler (no HIP header) and driven over stdin by tests/test_tr_math_cpu.py.
// One call per line: a function's name, then its arguments as (hex) floats; the answer is one line of hex floats.  "consts" prints every named constant.
//   g++ -std=c++14 -O1 -ffp-contract=off host_tr_math_test.cpp -o host_tr_math_test
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/tr_math.h"

#ifdef __HIPCC__
#error "this program checks the host path of tr_math.h"
#endif

static void put(const std::vector<double>& v) {
    for (size_t i = 0; i < v.size(); ++i) printf("%s%a", i ? " " : "", v[i]);
    printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name, tok;
        if (!(in >> name)) continue;
        std::vector<double> a;
        while (in >> tok) a.push_back(strtod(tok.c_str(), nullptr));
        const size_t n = a.size();
        if (name == "consts" && n == 0)
            put({TR_INITIAL_RADIUS, TR_MAX_RADIUS, TR_MIN_RADIUS, TR_MIN_RELATIVE_DECREASE, TR_FUNCTION_TOLERANCE, TR_GRADIENT_TOLERANCE, TR_PARAMETER_TOLERANCE,
                 TR_MIN_MU, TR_MAX_MU, TR_MU_INCREASE, TR_MU_DECREASE_NUM, TR_MU_DECREASE_DEN, TR_SHRINK_BELOW, TR_SHRINK, TR_GROW_ABOVE, TR_GROW,
                 TR_MIN_DIAGONAL, TR_MAX_DIAGONAL, TR_LM_DECREASE_FACTOR, TR_LM_DECREASE_GROWTH, (double)TR_MAX_INVALID_STEPS, (double)TR_GO_ON, (double)TR_NO_CONVERGENCE,
                 (double)TR_FUNCTION_TOL, (double)TR_PARAMETER_TOL, (double)TR_GRADIENT_TOL, (double)TR_MIN_RADIUS_REACHED, (double)TR_FAILURE});
        else if (name == "dogleg" && n == 8) {          // lm gg nn gd gnorm gnn radius alpha
            double ca, cb, snorm;
            tr_dogleg_coeffs(a[0] != 0.0, a[1], a[2], a[3], a[4], a[5], a[6], a[7], ca, cb, snorm);
            put({ca, cb, snorm});
        } else if (name == "dogleg_roots" && n == 5) {  // gd gnorm gnn radius alpha: the trajectory's form, the squares of the rounded roots for the sums
            double ca, cb, snorm;
            tr_dogleg_coeffs(false, 0.0, 0.0, a[0], a[1], a[2], a[3], a[4], ca, cb, snorm, true);
            put({ca, cb, snorm});
        } else if (name == "step" && n == 10) {         // ca cb grad gn diag scale g t y mu
            double sv, step_s, w, lin, quad;
            tr_step_element(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], sv, step_s, w, lin, quad);
            put({sv, step_s, w, lin, quad});
        } else if (name == "pconv" && n == 3) put({(double)tr_parameter_converged(a[0], a[1], a[2])});
        else if (name == "fconv" && n == 3) put({(double)tr_function_converged(a[0], a[1], a[2])});
        else if (name == "quality" && n == 3) put({tr_step_quality(a[0], a[1], a[2])});
        else if (name == "accepted" && n == 2) put({(double)tr_step_accepted(a[0], a[1])});
        else if (name == "accept" && n == 4) put({tr_dogleg_accepted_radius(a[0], a[1], a[2]), tr_mu_accepted(a[3])});          // quality step_norm radius mu
        else if (name == "reject" && n == 1) put({tr_dogleg_rejected_radius(a[0])});
        else if (name == "lm_accept_pow" && n == 3) put({tr_lm_accepted_radius(a[1], tr_cube_pow(2.0 * a[0] - 1.0), a[2])});    // gain radius max_radius
        else if (name == "lm_accept_mul" && n == 3) put({tr_lm_accepted_radius(a[1], tr_cube_mul(2.0 * a[0] - 1.0), a[2])});
        else if (name == "lm_reject" && n == 2) { double r = a[0], f = a[1]; tr_lm_rejected(r, f); put({r, f}); }
        else if (name == "invalid" && n == 1) put({(double)tr_invalid_limit((int)a[0])});
        else if (name == "gate" && n == 7) put({(double)tr_iteration_gate((int)a[0], (int)a[1], a[2] != 0.0, a[3], a[4], a[5], a[6])});
        else if (name == "scale" && n == 1) put({tr_jacobi_scale(a[0])});
        else if (name == "clip" && n == 1) put({tr_clip_diagonal(a[0])});
        else if (name == "clip" && n == 3) put({tr_clip_diagonal(a[0], a[1], a[2])});
        else if (name == "clip_minmax" && n == 1) put({tr_clip_diagonal_minmax(a[0])});
        else { fprintf(stderr, "bad call: %s\n", line.c_str()); return 2; }
    }
    return 0;
}

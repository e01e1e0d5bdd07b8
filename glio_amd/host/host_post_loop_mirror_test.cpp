// host_post_loop_mirror_test.cpp -- host-only (no device, no library): the arm / install / disarm sequence of glio::SlidingWindowBackend's speed-bias
// priors (armSpeedBiasPriors, solve, marginalize, marginalizeAndKeep, marginalizeAndKeepAsync) over a recording stand-in for the C-ABI.  Every call the
// backend makes is printed, doubles as hex floats; tests/test_post_loop_host_cpu.py holds the log against sliding.py's drivers over a recording backend,
// line for line.  The stand-in's glio_solve moves the state (speed/bias += 1/8, translation += 1/4) so that the log shows WHICH values were installed.
// Commands on standard input, one per line:  arm | solve | marginalize | keep | keep_async | finish
// Build: g++ -std=c++14 -O1 host_post_loop_mirror_test.cpp -I../../include      (also run once under -fsanitize=address,undefined)
#include <cstdio>
#include <iostream>
#include <string>

#include "glio_backend.hpp"

struct glio_ctx { int W; int sbp_n; };

extern "C" {
const char* glio_last_error(void) { return "stand-in"; }
int glio_create(int, const glio_opts* o, glio_ctx** out) { *out = new glio_ctx{o->window, 0}; return GLIO_OK; }
void glio_destroy(glio_ctx* c) { delete c; }
int glio_set_speed_bias_priors(glio_ctx* c, int n_slots, const double* target) {
    printf("set_speed_bias_priors %d", n_slots);
    for (int k = 0; k < 9 * n_slots; ++k) printf(" %a", target[k]);
    printf("\n");
    c->sbp_n = n_slots;
    return GLIO_OK;
}
int glio_solve(glio_ctx* c, glio_state* s, glio_summary* sum) {
    printf("solve\n");
    for (int k = 0; k < 9 * c->W; ++k) s->speed_bias[k] += 0.125;
    for (int k = 0; k < 3 * c->W; ++k) s->trans[k] += 0.25;
    *sum = glio_summary();
    return GLIO_OK;
}
int glio_marginalize_size(glio_ctx* c, int32_t* n, int32_t* nb) {
    const int ne = c->sbp_n > 2 ? c->sbp_n - 2 : 0;
    *n = 6 * (c->W - 1) + 9 + 9 * ne; *nb = 2 * (c->W - 1) + 1 + ne;
    printf("marginalize_size %d %d\n", (int)*n, (int)*nb);
    return GLIO_OK;
}
int glio_marginalize(glio_ctx* c, const glio_state* s, double* lin_jac, double* lin_res, int32_t* blk_slot, int32_t* blk_kind, int32_t* blk_idx, double* blk_x0,
                     int32_t* out_n, int32_t* out_nb) {
    int32_t n, nb;
    const int ne = c->sbp_n > 2 ? c->sbp_n - 2 : 0;
    n = 6 * (c->W - 1) + 9 + 9 * ne; nb = 2 * (c->W - 1) + 1 + ne;
    printf("marginalize %a\n", s->speed_bias[0]);
    for (int k = 0; k < n * n; ++k) lin_jac[k] = 0.0;            // (the whole of what the caller was told to allocate is written: the sanitizer run checks the sizes)
    for (int k = 0; k < n; ++k) lin_res[k] = 0.0;
    for (int k = 0; k < nb; ++k) { blk_slot[k] = 0; blk_kind[k] = 0; blk_idx[k] = 0; }
    for (int k = 0; k < 9 * nb; ++k) blk_x0[k] = 0.0;
    *out_n = n; *out_nb = nb;
    return GLIO_OK;
}
int glio_marginalize_keep(glio_ctx* c, const glio_state* s) { printf("marginalize_keep %a\n", s->speed_bias[0]); c->sbp_n = 0; return GLIO_OK; }
int glio_marginalize_keep_async(glio_ctx* c, const glio_state* s) { printf("marginalize_keep_async %a\n", s->speed_bias[0]); c->sbp_n = 0; return GLIO_OK; }
int glio_marginalize_keep_finish(glio_ctx*) { printf("marginalize_keep_finish\n"); return GLIO_OK; }
}

int main(int argc, char** argv) {
    glio_opts opts = glio_opts();
    opts.window = argc > 1 ? atoi(argv[1]) : 4;
    glio::SlidingWindowBackend be(opts);
    for (int k = 0; k < 9 * opts.window; ++k) be.tmpSpeedBias[k] = 0.5 * k - 3.0;
    std::string cmd;
    while (std::getline(std::cin, cmd)) {
        if (cmd == "arm") be.armSpeedBiasPriors();
        else if (cmd == "solve") be.solve();
        else if (cmd == "marginalize") { const glio::MarginalizationPrior m = be.marginalize(); printf("prior %d %zu\n", m.n, m.keep_block_slot.size()); }
        else if (cmd == "keep") be.marginalizeAndKeep();
        else if (cmd == "keep_async") be.marginalizeAndKeepAsync();
        else if (cmd == "finish") be.marginalizeFinish();
        else if (!cmd.empty()) { printf("bad command\n"); return 2; }
        printf("armed %d\n", be.speedBiasPriorsArmed() ? 1 : 0);
    }
    return 0;
}

// host_window_tables_test.cpp -- glio_amd/csrc/window_tables.h (the host arithmetic of the window context) compiled by a plain host compiler, with and
// without the sanitizers, and run by tests/test_window_tables_cpu.py.  Reads commands from standard input, prints what the header's functions make of
// them; the expectations are stated in the test file, not here.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all host_window_tables_test.cpp -o host_window_tables_test
//
//   gnss W n_ddt_max n_dd n_dop, then n_dd x (slot_i slot_j n_sat master tag), n_dop x (slot_i slot_j epoch tag)      (tag: travels in `ratio`)
//   prior W np nb, then nb x (slot kind idx)
//   marg W sbp_n nb, then nb x (slot kind idx): the installed prior (nb = 0: none), np = what its blocks cover
//   chain np nb, then nb x (slot kind idx), then np * np doubles
//   stage cap early, then any of: up BYTES | d2d BYTES | word, ended by `end`
//   imu slot, then 225 doubles (the covariance)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <string>

#include "../csrc/window_tables.h"

#ifdef __HIPCC__
#error "this program checks host code"
#endif

template <class V> static void row(const char* name, const V& v) {
    printf("%s", name);
    for (auto x : v) printf(" %d", (int)x);
    printf("\n");
}
static bool refusal(const TabError& e) { printf("refused %d %s\n", e.code, e.msg); return true; }
struct Blocks { std::vector<int32_t> slot, kind, idx; int np = 0; };
static Blocks read_blocks(int nb) {
    Blocks b;
    b.slot.resize(nb); b.kind.resize(nb); b.idx.resize(nb);
    for (int k = 0; k < nb; ++k) {
        std::cin >> b.slot[k] >> b.kind[k] >> b.idx[k];
        b.np = std::max(b.np, b.idx[k] + (b.kind[k] == GLIO_BLK_SPEEDBIAS ? 9 : 3));
    }
    return b;
}

static void cmd_gnss() {
    int W, n_ddt_max, n_dd, n_dop;
    std::cin >> W >> n_ddt_max >> n_dd >> n_dop;
    std::vector<glio_dd_psr> dd(n_dd);
    std::vector<glio_doppler> dop(n_dop);
    for (auto& f : dd) { memset(&f, 0, sizeof f); std::cin >> f.slot_i >> f.slot_j >> f.n_sat >> f.master >> f.ratio; }
    for (auto& f : dop) { memset(&f, 0, sizeof f); std::cin >> f.slot_i >> f.slot_j >> f.epoch >> f.ratio; }
    GnssTables t;
    TabError e;
    if (gnss_build_tables(W, n_ddt_max, n_dd, dd.data(), n_dop, dop.data(), &t, &e)) { refusal(e); return; }
    // "copied": the result refers to a copy of the input, not to the caller's array
    printf("ok %d %d\n", (int)(t.dd != dd.data() || !t.dd_copy.empty()), (int)(t.dop != dop.data() || !t.dop_copy.empty()));
    printf("groups");
    for (auto& g : t.groups) printf(" %d %d %d %d %d %d %d %d", g.slot_i, g.slot_j, g.dd_begin, g.dd_end, g.dop_begin, g.dop_end, g.run_begin, g.run_end);
    printf("\nruns");
    for (auto& r : t.runs) printf(" %d %d %d %d", r.begin, r.end, r.epoch, r.group);
    printf("\nes");
    for (auto& s : t.es) printf(" %d %d", s.x, s.y);
    printf("\n");
    row("off", t.off); row("list", t.list);
    printf("flags %d %d %d\n", t.gnss_ok, t.gnss_chain, t.max_epoch);
    printf("ddorder");
    for (size_t k = 0; k < t.n_dd; ++k) printf(" %d", (int)t.dd[k].ratio);
    printf("\ndoporder");
    for (size_t k = 0; k < t.n_dop; ++k) printf(" %d", (int)t.dop[k].ratio);
    printf("\n");
}

static void cmd_prior() {
    int W, np, nb;
    std::cin >> W >> np >> nb;
    const Blocks b = read_blocks(nb);
    std::vector<int> index(15 * W), colblk(np);
    TabError e;
    if (prior_index_tables(W, np, nb, b.slot.data(), b.kind.data(), b.idx.data(), index.data(), colblk.data(), &e)) { refusal(e); return; }
    const PriorFlags f = prior_flags(nb, b.slot.data(), b.kind.data());
    printf("ok %d %d\n", f.prior_ok, f.ext_coupled);
    row("index", index); row("colblk", colblk);
}

static void cmd_marg() {
    int W, sbp_n, nb_in;
    std::cin >> W >> sbp_n >> nb_in;
    const Blocks in = read_blocks(nb_in);
    std::vector<int> h_index(15 * W, -1), cb(in.np);
    TabError e;
    if (nb_in && prior_index_tables(W, in.np, nb_in, in.slot.data(), in.kind.data(), in.idx.data(), h_index.data(), cb.data(), &e)) { refusal(e); return; }
    // a state whose every entry names itself: trans 1000 + 3 k + j, quat 2000 + 4 k + j, speed/bias 3000 + 9 k + j
    std::vector<double> tr(3 * W), qu(4 * W), sb(9 * W);
    for (int k = 0; k < 3 * W; ++k) tr[k] = 1000 + k;
    for (int k = 0; k < 4 * W; ++k) qu[k] = 2000 + k;
    for (int k = 0; k < 9 * W; ++k) sb[k] = 3000 + k;
    glio_state s{tr.data(), qu.data(), sb.data(), nullptr, 0};
    short extra[GLIO_MAX_WINDOW];
    const int ne = glio_marg_layout(W, sbp_n, in.np, h_index.data(), extra);
    const KeptSize want = marg_kept_size(W, ne);
    const int fits = want.n <= glio_prior_np_limit(W) && want.nb <= glio_prior_nb_limit(W);
    printf("size %d %d %d %d\n", want.n, want.nb, ne, fits);
    // (the library builds the tables only for a layout that fits; the buffers here hold every layout)
    std::vector<int32_t> slot(3 * W), kind(3 * W), idx(3 * W);
    std::vector<double> x0(27 * (size_t)W, -1.0);
    const KeptSize k = marg_block_tables(W, sbp_n, in.np, h_index.data(), &s, slot.data(), kind.data(), idx.data(), x0.data());
    if (k.n != want.n || k.nb != want.nb) { printf("size mismatch\n"); return; }
    slot.resize(k.nb); kind.resize(k.nb); idx.resize(k.nb); x0.resize(9 * (size_t)k.nb);
    row("slot", slot); row("kind", kind); row("idx", idx); row("x0", x0);
    std::vector<int> index(15 * W), colblk(k.n);
    if (prior_index_tables(W, k.n, k.nb, slot.data(), kind.data(), idx.data(), index.data(), colblk.data(), &e)) { refusal(e); return; }
    row("index", index); row("colblk", colblk);
}

static void cmd_chain() {
    int np, nb;
    std::cin >> np >> nb;
    const Blocks b = read_blocks(nb);
    std::vector<double> J((size_t)np * np);
    for (auto& v : J) std::cin >> v;
    int W = 1;
    for (int s : b.slot) W = std::max(W, s + 1);
    std::vector<int> index(15 * W), colblk(np);
    TabError e;
    if (prior_index_tables(W, np, nb, b.slot.data(), b.kind.data(), b.idx.data(), index.data(), colblk.data(), &e)) { refusal(e); return; }
    printf("chain %d\n", (int)prior_is_chain(np, J.data(), b.slot.data(), colblk.data()));
}

static void cmd_stage() {
    size_t cap; int early;
    std::cin >> cap >> early;
    std::vector<char> h(cap), d(cap);        // stand-ins for the pinned block and its mirror: only addresses are formed
    StageBatch b;
    stage_open(&b, h.data(), d.data(), cap, early);
    char dst[8];
    for (std::string op; std::cin >> op && op != "end";) {
        TabError e;
        if (op == "up") {
            size_t bytes; std::cin >> bytes;
            StagePlace p;
            if (stage_place(&b, dst, bytes, &p, &e)) { refusal(e); continue; }
            memset(p.at, 0x5a, bytes);          // what capi.hip's memcpy writes: the sanitizer sees every byte of it
            if (p.direct) printf("direct %zu\n", (size_t)(p.at - h.data()));
            else {
                const StageSegDev& sg = b.seg[b.n_seg - 1];
                printf("seg %zu %d %d\n", (size_t)(p.at - h.data()), (int)(sg.dst == dst && sg.bytes == bytes && (const char*)sg.src - d.data() == p.at - h.data()), b.n_seg);
            }
        } else if (op == "d2d") {
            size_t bytes; std::cin >> bytes;
            if (stage_place_d2d(&b, dst, dst + 4, bytes, &e)) { refusal(e); continue; }
            printf("d2d %d\n", b.n_seg);
        } else if (op == "word") {
            char* w = stage_result_word(&b);
            if (!w) { printf("word none\n"); continue; }
            memset(w, 0, 4);
            printf("word %zu\n", (size_t)(w - h.data()));
        } else exit(2);
    }
    printf("used %zu top %zu block %zu\n", b.used, b.top, stage_block_bytes(0));
}

static void cmd_imu() {
    int slot;
    std::cin >> slot;
    glio_preint p;
    for (int k = 0; k < 3; ++k) { p.delta_p[k] = 10 + k; p.delta_v[k] = 20 + k; p.linearized_ba[k] = 30 + k; p.linearized_bg[k] = 40 + k; }
    for (int k = 0; k < 4; ++k) p.delta_q[k] = 50 + k;
    p.sum_dt = 60;
    for (int k = 0; k < 225; ++k) p.jacobian[k] = 100 + k;
    for (int k = 0; k < 225; ++k) std::cin >> p.covariance[k];
    ImuEdgeDev e;
    if (!digest_edge(&p, slot, &e)) { printf("digest 0\n"); return; }
    printf("digest 1\n");
    std::vector<double> head(e.delta_p, e.delta_p + 17), jac(e.dp_dba, e.dp_dba + 45);
    row("head", head); row("jac", jac);
    int below = 0, diag_pos = 0;
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) { if (j < i && e.sqrt_info[i * 15 + j] != 0.0) ++below; if (i == j && e.sqrt_info[i * 15 + j] > 0.0) ++diag_pos; }
    printf("slot %d pad %d below %d diag %d\n", e.slot_i, e.pad_, below, diag_pos);
}

int main() {
    for (std::string cmd; std::cin >> cmd;) {
        if (cmd == "gnss") cmd_gnss();
        else if (cmd == "prior") cmd_prior();
        else if (cmd == "marg") cmd_marg();
        else if (cmd == "chain") cmd_chain();
        else if (cmd == "stage") cmd_stage();
        else if (cmd == "imu") cmd_imu();
        else return 2;
        printf("--\n");
    }
    return std::cin.eof() ? 0 : 3;
}

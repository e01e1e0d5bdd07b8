// host_linearize_entry_test.cpp -- the host arithmetic behind the prior's form by keyframe (csrc/window_tables.h: prior_span_tables,
// prior_jac_is_block_exact) as a program of its own: plain host compiler, no HIP.  tests/test_linearize_entry_cpu.py builds it with the address and
// undefined-behaviour sanitizers and compares what it prints.
//
// Layouts: the standard prior of a window of W keyframes ([T Q SB] of slot 0, [T Q] of slots 1 .. W-2), the same with its blocks listed in reverse
// order, and the layout after a loop closure (speed-bias blocks of further slots behind the poses), which cannot be walked by span.
#include <cstdio>
#include <vector>

#include "../csrc/window_tables.h"

struct Layout { int W, np; std::vector<int32_t> slot, kind, idx; };

static Layout standard(int W, int extra_sb) {
    Layout L;
    L.W = W;
    int at = 0;
    for (int s = 0; s + 1 < W; ++s)
        for (int k = 0; k < (s == 0 ? 3 : 2); ++k) { L.slot.push_back(s); L.kind.push_back(k); L.idx.push_back(at); at += k == 2 ? 9 : 3; }
    for (int j = 0; j < extra_sb; ++j) { L.slot.push_back(1 + j); L.kind.push_back(GLIO_BLK_SPEEDBIAS); L.idx.push_back(at); at += 9; }
    L.np = at;
    return L;
}

static int report(const char* name, const Layout& L) {
    const int nb = (int)L.slot.size();
    std::vector<int> index(15 * L.W), colblk(L.np), span(4 * (size_t)L.np);
    TabError e;
    if (prior_index_tables(L.W, L.np, nb, L.slot.data(), L.kind.data(), L.idx.data(), index.data(), colblk.data(), &e)) { printf("%s refused: %s\n", name, e.msg); return 1; }
    const int ok = prior_span_tables(L.W, L.np, nb, L.slot.data(), L.kind.data(), L.idx.data(), colblk.data(), span.data());
    printf("%s np %d ok %d:", name, L.np, ok);
    for (int j = 0; j < L.np; ++j)
        if (j == 0 || span[4 * j] != span[4 * j - 4]) printf(" [%d %d %d %d]", span[4 * j], span[4 * j + 1], span[4 * j + 2], span[4 * j + 3]);
    printf("\n");
    // a Jacobian that is block diagonal by keyframe, then one entry (a negative zero, a tiny number) outside the blocks
    std::vector<double> J((size_t)L.np * L.np, 0.0);
    for (int i = 0; i < L.np; ++i)
        for (int j = 0; j < L.np; ++j)
            if (L.slot[colblk[i]] == L.slot[colblk[j]]) J[(size_t)i * L.np + j] = 1.0 + i + 0.5 * j;
    const int a = prior_jac_is_block_exact(L.np, J.data(), L.slot.data(), colblk.data());
    J[(size_t)(L.np - 1)] = -0.0;
    const int b = prior_jac_is_block_exact(L.np, J.data(), L.slot.data(), colblk.data());
    J[(size_t)(L.np - 1)] = 1e-300;
    const int c = prior_jac_is_block_exact(L.np, J.data(), L.slot.data(), colblk.data());
    printf("%s exact %d %d %d\n", name, a, b, c);
    return 0;
}

int main() {
    int rc = 0;
    rc |= report("W3", standard(3, 0));
    rc |= report("W20", standard(20, 0));
    rc |= report("W64", standard(64, 0));
    Layout r = standard(4, 0);
    for (size_t k = 0; k < r.slot.size() / 2; ++k) {
        const size_t m = r.slot.size() - 1 - k;
        std::swap(r.slot[k], r.slot[m]); std::swap(r.kind[k], r.kind[m]); std::swap(r.idx[k], r.idx[m]);
    }
    rc |= report("W4 reversed", r);
    rc |= report("W5 loop", standard(5, 2));
    return rc;
}

// host_switches_test.cpp -- glio_amd/csrc/glio_switches.h and switches.hip (the table, the parse rule, the process snapshot) compiled by a plain host
// compiler, sanitizers on, and run by tests/test_switches_cpu.py.  Prints "parse NAME TEXT VALUE" for every named row and every argument ("-" stands for
// unset, "" for the empty string), then the snapshot before and after the environment changes under it.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all host_switches_test.cpp -o host_switches_test
#include <cstdio>

#include "../csrc/switches.hip"

#ifdef __HIPCC__
#error "this program checks the host code of the switch table"
#endif

int main(int argc, char** argv) {
    for (int i = 0; i < GLIO_SW_COUNT; ++i) {
        const char* name = glio_switch_rows[i].name;
        if (!name) continue;
        for (int a = 0; a < argc; ++a) {
            int v = 0;
            if (glio_debug_switch_parse(name, a ? argv[a] : nullptr, &v) != GLIO_OK) return 2;
            printf("parse %s %s %d\n", name, a ? argv[a] : "-", v);
        }
    }
    int v = 0;
    if (glio_debug_switch_value("GLIO_nonexistent", &v) != GLIO_E_ARG || glio_debug_switch_parse(nullptr, "1", &v) != GLIO_E_ARG) return 3;
    setenv("GLIO_CHAIN_FAST", "1", 1); setenv("GLIO_BCR_ELIM", "0", 1); setenv("GLIO_LM_SORT", "1", 1);
    printf("first %d %d %d\n", glio_switch<GLIO_SW_CHAIN_FAST>(), glio_switch<GLIO_SW_BCR_ELIM>(), glio_switch_at_create<GLIO_SW_LM_SORT>());
    setenv("GLIO_CHAIN_FAST", "2", 1); unsetenv("GLIO_BCR_ELIM"); setenv("GLIO_LM_SORT", "0", 1);
    printf("later %d %d %d\n", glio_switch<GLIO_SW_CHAIN_FAST>(), glio_switch<GLIO_SW_BCR_ELIM>(), glio_switch_at_create<GLIO_SW_LM_SORT>());
    const int old = glio_switch_set<GLIO_SW_CHAIN_FAST>(0);
    printf("set %d %d\n", old, glio_switch<GLIO_SW_CHAIN_FAST>());
    return 0;
}

// host_map_mirror_test -- host-only: glio::globalMapFrames (glio_map_backend.hpp) for tests/test_global_map_cpu.py.  Reads "n_keyframes mapping_interval" pairs
// from stdin, prints one line of frame indices per pair.  Links nothing of the library.
#include <cstdio>

#include "glio_map_backend.hpp"

int main() {
    int n, m;
    while (scanf("%d %d", &n, &m) == 2) {
        const std::vector<int32_t> fr = glio::globalMapFrames(n, m);
        printf("frames");
        for (int32_t i : fr) printf(" %d", (int)i);
        printf("\n");
    }
    return 0;
}

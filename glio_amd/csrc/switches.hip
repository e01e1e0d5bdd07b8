// switches.hip -- the definitions behind glio_switches.h: the table's rows, the one place of the library that looks at the environment, and the
// read-only hooks of the tests.  Host code only (plain C++: glio_amd/host/host_switches_test.cpp compiles this file without HIP).
#include "glio_switches.h"

#include "../../include/glio_hip.h"

const GlioSwitchRow glio_switch_rows[GLIO_SW_COUNT] = {
#define GLIO_SWITCH_ROW(id, name, dflt, norm, arg, scope, doc) {name, dflt, GLIO_SW_##norm, arg, GLIO_SW_##scope, doc},
    GLIO_SWITCH_TABLE(GLIO_SWITCH_ROW)
#undef GLIO_SWITCH_ROW
};

static int read_row(const GlioSwitchRow& r) { return glio_switch_parse(r, r.name ? getenv(r.name) : nullptr); }
GlioSwitchValues glio_switch_read_all() {
    GlioSwitchValues s;
    for (int i = 0; i < GLIO_SW_COUNT; ++i) s.v[i] = read_row(glio_switch_rows[i]);
    return s;
}
int glio_switch_read(GlioSwitchId id) { return read_row(glio_switch_rows[id]); }

static int find_row(const char* name) {
    for (int i = 0; name && i < GLIO_SW_COUNT; ++i)
        if (glio_switch_rows[i].name && strcmp(glio_switch_rows[i].name, name) == 0) return i;
    return -1;
}

extern "C" {

// the value the library works with: a PROCESS row from the snapshot (taken here if this is the first query), a CREATE row as an object created now would read it
int glio_debug_switch_value(const char* name, int* value) {
    const int i = find_row(name);
    if (i < 0 || !value) return GLIO_E_ARG;
    *value = glio_switch_rows[i].scope == GLIO_SW_PROCESS ? glio_switch_snapshot().v[i] : read_row(glio_switch_rows[i]);
    return GLIO_OK;
}
// the row's parse of a string (null: unset); the environment is not looked at
int glio_debug_switch_parse(const char* name, const char* text_or_null, int* value) {
    const int i = find_row(name);
    if (i < 0 || !value) return GLIO_E_ARG;
    *value = glio_switch_parse(glio_switch_rows[i], text_or_null);
    return GLIO_OK;
}
// row `index` of the named rows (capi.switches() walks them until GLIO_E_ARG); scope: 0 PROCESS, 1 CREATE
int glio_debug_switch_row(int index, const char** name, int* dflt, int* scope, const char** doc) {
    if (index < 0 || index >= GLIO_SW_COUNT || !glio_switch_rows[index].name || !name || !dflt || !scope || !doc) return GLIO_E_ARG;
    const GlioSwitchRow& r = glio_switch_rows[index];
    *name = r.name; *dflt = r.dflt; *scope = r.scope; *doc = r.doc;
    return GLIO_OK;
}

}  // extern "C"

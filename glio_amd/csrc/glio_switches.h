// glio_switches.h -- every GLIO_* environment switch of libglio_hip.so: one table, one parse rule, two read rules.  Host only (no HIP).
// The switches are lab switches (A/B runs, cross-checks, development aids), not API: INTEGRATION.md, "Environment switches".
//
// Parse rule: unset gives the row's default; otherwise atoi(text) goes through the row's normalisation ("" counts as 0):
//   RAW    the number itself                        MASK   number & arg
//   RANGE  the number if 0 <= number <= arg, else the default           BOOL   number != 0
// Read rules:
//   PROCESS  all such rows are read together, at the first query of any of them in the process (glio_switch / glio_switch_set): one
//            snapshot, and the environment is not looked at again.  The glio_debug_* setters write the snapshot.
//   CREATE   read when the object it configures is created or configured (glio_switch_at_create): glio_create, glio_bassoc_create,
//            glio_dense_create, glio_scan_filter_config, a local map's or voxel grid's creation, a ring's first rebuild.
// The last rows have no environment name: knobs that only their setters write (tests and A/B scripts).
#pragma once
#include <cstdlib>
#include <cstring>

//  id, environment name, default, normalisation, arg, scope, meaning
#define GLIO_SWITCH_TABLE(X) \
    X(KNN_MODE,            "GLIO_KNN_MODE",            0,   RANGE, 3, PROCESS, "nearest-neighbour search: 0 window queries grouped by cell, near block first; 1 one 16-lane group per query; 2 the 27-cell tiled search; 3 near block first, every row by itself") \
    X(BATCH_MOMENTS,       "GLIO_BATCH_MOMENTS",       1,   RAW,   0, PROCESS, "batch stage: 0 every linearisation streams the constraints instead of the per-pair moments") \
    X(BCR_ELIM,            "GLIO_BCR_ELIM",            -1,  RAW,   0, PROCESS, "batch solve elimination: -1 by block size, 1 the blocked form, 0 one register step per pivot") \
    X(DEBUG_FILL,          "GLIO_DEBUG_FILL",          -1,  RAW,   0, PROCESS, "development aid: fill every allocation of a context with this byte (-1: no fill)") \
    X(DEBUG_LDS_POISON,    "GLIO_DEBUG_LDS_POISON",    0,   RAW,   0, PROCESS, "development aid: a kernel that fills the LDS with NaN patterns runs in front of the solves") \
    X(DEBUG_POISON_ALLOC,  "GLIO_DEBUG_POISON_ALLOC",  0,   RAW,   0, PROCESS, "development aid: every device allocation of the library is handed out filled with 0xFF bytes") \
    X(ROCTX,               "GLIO_ROCTX",               0,   BOOL,  0, PROCESS, "roctx ranges around the library's calls (needs libroctx64.so)") \
    X(CHAIN_FAST,          "GLIO_CHAIN_FAST",          3,   MASK,  3, PROCESS, "chain step from LDS: bit 0 its tail, bit 1 its front; 0 the generic bodies") \
    X(SOLVE_ENDS,          "GLIO_SOLVE_ENDS",          6,   MASK,  6, PROCESS, "ends of a solve: bit 1 the first launch reads the mapped host copy, bit 2 the result is published from LDS; 0 the staging launch and finalize()") \
    X(CHAIN_FRONTS,        "GLIO_CHAIN_FRONTS",        4,   RAW,   0, PROCESS, "2: the chain keeps the two-front elimination for every window") \
    X(CHAIN_HELPERS,       "GLIO_CHAIN_HELPERS",       1,   BOOL,  0, PROCESS, "0: no helper workgroups beside the chain step") \
    X(CHAIN_HELPER_POLLS,  "GLIO_CHAIN_HELPER_POLLS",  256, RAW,   0, PROCESS, "polls the chain step waits for its helpers; 0 gives them up at once") \
    X(CHAIN_FAT,           "GLIO_CHAIN_FAT",           1,   BOOL,  0, PROCESS, "0: the helpers only sum, no speculative build of the blocks") \
    X(MARG_SPLIT,          "GLIO_MARG_SPLIT",          1,   BOOL,  0, PROCESS, "0: the one-workgroup form of the marginalisation") \
    X(BASSOC_LOCAL_TABLES, "GLIO_BASSOC_LOCAL_TABLES", 1,   BOOL,  0, PROCESS, "0: the batch association hashes every search frame at its pose, never in its own frame") \
    X(BASSOC_LOCAL_RATIO,  "GLIO_BASSOC_LOCAL_RATIO",  16,  RAW,   0, PROCESS, "own-frame tables only below this many pairs per frame to hash") \
    X(BASSOC_SHARED_BINS,  "GLIO_BASSOC_SHARED_BINS",  1,   BOOL,  0, PROCESS, "0: every pair of the batch association bins its queries for itself") \
    X(EARLY_UPLOAD,        "GLIO_EARLY_UPLOAD",        1,   BOOL,  0, CREATE,  "glio_create: 0 glio_set_imu / glio_set_gnss copy on the context's stream and wait for it") \
    X(UNSTAGE_IN_STREAM,   "GLIO_UNSTAGE_IN_STREAM",   0,   BOOL,  0, CREATE,  "glio_create: 1 the early uploads are installed on the context's stream, behind the searches") \
    X(EARLY_UPLOAD_WAIT,   "GLIO_EARLY_UPLOAD_WAIT",   0,   BOOL,  0, CREATE,  "glio_create: 1 an early upload waits for its copy") \
    X(CTX_PRIORITY,        "GLIO_CTX_PRIORITY",        1,   BOOL,  0, CREATE,  "glio_create: 0 the context's stream has the default priority, not the highest") \
    X(BASSOC_PRIORITY,     "GLIO_BASSOC_PRIORITY",     1,   BOOL,  0, CREATE,  "glio_bassoc_create: 0 the store's stream has the default priority, not the lowest") \
    X(LM_SORT,             "GLIO_LM_SORT",             0,   BOOL,  0, CREATE,  "a local map's or voxel grid's creation: 1 the map is ordered by the radix sort only, no occupancy bitmap") \
    X(LM_REBUILD_TIMING,   "GLIO_LM_REBUILD_TIMING",   0,   BOOL,  0, CREATE,  "a ring's first rebuild: 1 rebuilds are timed with events") \
    X(KFCLOUD_TIMING,      "GLIO_KFCLOUD_TIMING",      0,   BOOL,  0, CREATE,  "glio_scan_filter_config: 1 the keyframe cloud's stages are timed with events") \
    X(DENSE_TIMING,        "GLIO_DENSE_TIMING",        0,   BOOL,  0, CREATE,  "glio_dense_create: 1 the dense store's stages are timed with events") \
    X(GBIN_CAP,            nullptr,                    0,   RAW,   0, PROCESS, "glio_debug_set_gbin_cap: cell-table size of the merged-window grouping, 0 = from the map") \
    X(LINEARIZE_ENTRY,     nullptr,                    7,   MASK,  7, PROCESS, "glio_debug_linearize_entry: the merged linearisation launch: bit 0 status, counts and records asked for at entry, bit 1 the prior by keyframe on the chain path, bit 2 K3 workgroups from the roles' own count; 0 the launch as it was")

enum GlioSwitchId {
#define GLIO_SWITCH_ID(id, name, dflt, norm, arg, scope, doc) GLIO_SW_##id,
    GLIO_SWITCH_TABLE(GLIO_SWITCH_ID)
#undef GLIO_SWITCH_ID
    GLIO_SW_COUNT
};
enum GlioSwitchNorm { GLIO_SW_RAW, GLIO_SW_MASK, GLIO_SW_RANGE, GLIO_SW_BOOL };
enum GlioSwitchScope { GLIO_SW_PROCESS, GLIO_SW_CREATE };
struct GlioSwitchRow { const char* name; int dflt; GlioSwitchNorm norm; int arg; GlioSwitchScope scope; const char* doc; };
struct GlioSwitchValues { int v[GLIO_SW_COUNT]; };

constexpr GlioSwitchScope glio_switch_scope[GLIO_SW_COUNT] = {
#define GLIO_SWITCH_SCOPE(id, name, dflt, norm, arg, scope, doc) GLIO_SW_##scope,
    GLIO_SWITCH_TABLE(GLIO_SWITCH_SCOPE)
#undef GLIO_SWITCH_SCOPE
};

// switches.hip (the one translation unit that looks at the environment)
extern const GlioSwitchRow glio_switch_rows[GLIO_SW_COUNT];
GlioSwitchValues glio_switch_read_all();             // every row as the environment has it now
int glio_switch_read(GlioSwitchId id);               // one row as the environment has it now

static inline int glio_switch_parse(const GlioSwitchRow& r, const char* text) {
    if (!text) return r.dflt;
    const int v = atoi(text);
    switch (r.norm) {
        case GLIO_SW_MASK: return v & r.arg;
        case GLIO_SW_RANGE: return v >= 0 && v <= r.arg ? v : r.dflt;
        case GLIO_SW_BOOL: return v != 0;
        default: return v;
    }
}
// the process's snapshot (one object for the whole library: an inline function's static)
inline GlioSwitchValues& glio_switch_snapshot() { static GlioSwitchValues s = glio_switch_read_all(); return s; }
// the accessors take the row as a template argument, so that the wrong read rule for a row does not compile
template <GlioSwitchId id> static inline int glio_switch() {
    static_assert(glio_switch_scope[id] == GLIO_SW_PROCESS, "a CREATE row is read with glio_switch_at_create");
    return glio_switch_snapshot().v[id];
}
template <GlioSwitchId id> static inline int glio_switch_set(int value) {          // returns the value it replaces
    static_assert(glio_switch_scope[id] == GLIO_SW_PROCESS, "only the snapshot can be written");
    int& v = glio_switch_snapshot().v[id];
    const int old = v;
    v = value;
    return old;
}
template <GlioSwitchId id> static inline int glio_switch_at_create() {
    static_assert(glio_switch_scope[id] == GLIO_SW_CREATE, "a PROCESS row is read with glio_switch");
    return glio_switch_read(id);
}

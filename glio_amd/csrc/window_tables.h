// window_tables.h -- the host arithmetic of the window context: every table a set_* call or a marginalization hands to the device, and the byte
// arithmetic of the pinned upload arena.  HOST ONLY: no HIP header, include/glio_types.h and the standard library, so that it compiles with a plain host
// compiler (glio_amd/host/host_window_tables_test.cpp runs it under the sanitizers) as well as inside capi.hip, which keeps every HIP call and every
// memcpy into pinned memory.  The plain structs the functions fill live here; glio_device.h includes this header.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/glio_types.h"

// A refusal: the code the entry point returns (the values of GLIO_E_ARG / GLIO_E_STATE, include/glio_hip.h; capi.hip asserts them) and the text of
// glio_last_error (empty: the entry point leaves the last error as it is)
#define TAB_E_ARG (-1)
#define TAB_E_STATE (-3)
struct TabError { int code = 0; char msg[320] = ""; };
static inline int tab_refuse(TabError* e, int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(e->msg, sizeof e->msg, fmt, ap); va_end(ap);
    return e->code = code;
}
// ---------------------------------------------------------------------------------------------- device-resident layouts the host fills
// IMU edge, device form (pre-digested on upload: sqrt_info is LLT(cov^-1).L^T, ImuFactor.h:44-45)
struct ImuEdgeDev {
    double delta_p[3], delta_q[4], delta_v[3], lin_ba[3], lin_bg[3];
    double sum_dt;
    double dp_dba[9], dp_dbg[9], dq_dbg[9], dv_dba[9], dv_dbg[9];
    double sqrt_info[225];
    int slot_i;
    int pad_;
};
// GNSS group = all DD / Doppler factors that share one (slot_i, slot_j) pair
struct GnssGroup {
    int slot_i, slot_j;
    int dd_begin, dd_end;      // range in the sorted glio_dd_psr array
    int dop_begin, dop_end;    // range in the sorted glio_doppler array (sorted by epoch inside)
    int run_begin, run_end;    // range in the DopRun array
};
// Doppler rows of one epoch inside a group (contiguous in the sorted glio_doppler array)
struct DopRun { int begin, end, epoch, group; };
// keyframe slots (lo, hi) coupled by one clock-drift epoch, (-1, -1) if unused: the layout of the int2 the kernels read (ArrowDev::d_ep_slots)
struct alignas(8) EpochSlots { int x, y; };
static_assert(sizeof(ImuEdgeDev) == 2304 && sizeof(GnssGroup) == 32 && sizeof(DopRun) == 16 && sizeof(EpochSlots) == 8 && alignof(EpochSlots) == 8, "device layouts");

// ---------------------------------------------------------------------------------------------- prior
// Limits of a prior: the LDS arrays of the prior's workgroups (factor_kernels.hip, PriorLds) are sized by them.  A standard prior has 6 W + 9 columns in
// 2 W + 1 blocks; the layouts of the windows after a loop closure (speed-bias blocks of several keyframes) up to 15 (W - 1) in 3 (W - 1): W <= 27.
#define PRIOR_MAX_NP (6 * GLIO_MAX_WINDOW + 9)
#define PRIOR_MAX_NB (2 * GLIO_MAX_WINDOW + 1)
static inline int glio_prior_np_limit(int W) { const int a = 6 * W + 9, b = 15 * (W - 1), m = a > b ? a : b; return m < PRIOR_MAX_NP ? m : PRIOR_MAX_NP; }
static inline int glio_prior_nb_limit(int W) { const int a = 2 * W + 1, b = 3 * (W - 1), m = a > b ? a : b; return m < PRIOR_MAX_NB ? m : PRIOR_MAX_NB; }

// index[15 W]: state index -> prior column or -1;  colblk[np]: prior column -> block.  Every block table goes through here: a caller's
// (glio_set_prior) and the library's own (glio_marginalize_keep_async, marg_block_tables below).
static inline int prior_index_tables(int W, int np, int nb, const int32_t* blk_slot, const int32_t* blk_kind, const int32_t* blk_idx, int* index, int* colblk, TabError* e) {
    std::fill_n(index, 15 * W, -1); std::fill_n(colblk, np, -1);
    for (int b = 0; b < nb; ++b) {
        const int s = blk_slot[b], k = blk_kind[b], idx = blk_idx[b];
        if (k != GLIO_BLK_TRANS && k != GLIO_BLK_QUAT && k != GLIO_BLK_SPEEDBIAS) return tab_refuse(e, TAB_E_ARG, "prior block %d: unknown kind %d", b, k);
        const int ls = k == GLIO_BLK_SPEEDBIAS ? 9 : 3;
        if (s < 0 || s >= W || idx < 0 || idx + ls > np) return tab_refuse(e, TAB_E_ARG, "prior block out of range");
        const int off = 15 * s + (k == GLIO_BLK_TRANS ? 0 : (k == GLIO_BLK_QUAT ? 3 : 6));
        for (int j = 0; j < ls; ++j) {
            if (index[off + j] >= 0) return tab_refuse(e, TAB_E_ARG, "prior: two blocks for slot %d kind %d", s, k);
            if (colblk[idx + j] >= 0) return tab_refuse(e, TAB_E_ARG, "prior: blocks %d and %d overlap at column %d", colblk[idx + j], b, idx + j);
            index[off + j] = idx + j; colblk[idx + j] = b;
        }
    }
    for (int j = 0; j < np; ++j) if (colblk[j] < 0) return tab_refuse(e, TAB_E_ARG, "prior column %d not covered by a block", j);
    return 0;
}
// Is J0^T J0 block diagonal by keyframe?  The reference's own marginalization always produces that (its LiDAR factors constrain every pose
// absolutely, quirk Q7, so eliminating the oldest keyframe never couples two kept ones); then the whole window is a keyframe chain and the solver
// needs no dense pose block.
static inline bool prior_is_chain(int np, const double* lin_jac, const int32_t* blk_slot, const int* colblk) {
    std::vector<double> cn(np, 0.0);
    for (int i = 0; i < np; ++i) for (int j = 0; j < np; ++j) cn[j] += lin_jac[(size_t)i * np + j] * lin_jac[(size_t)i * np + j];
    bool chain = true;
    for (int a = 0; a < np && chain; ++a)
        for (int b2 = a + 1; b2 < np; ++b2) {
            if (blk_slot[colblk[a]] == blk_slot[colblk[b2]]) continue;
            double sab = 0;
            for (int i = 0; i < np; ++i) sab += lin_jac[(size_t)i * np + a] * lin_jac[(size_t)i * np + b2];
            if (fabs(sab) > 1e-13 * sqrt(cn[a] * cn[b2])) { chain = false; break; }
        }
    return chain;
}
// prior_ok: at most one speed-bias block (two would couple the arrow factorisation's chain densely);  ext_coupled: a speed-bias block beyond slot 1
struct PriorFlags { int prior_ok, ext_coupled; };
static inline PriorFlags prior_flags(int nb, const int32_t* blk_slot, const int32_t* blk_kind) {
    int nsb = 0, ext = 0;
    for (int b = 0; b < nb; ++b) if (blk_kind[b] == GLIO_BLK_SPEEDBIAS) { ++nsb; ext |= blk_slot[b] >= 2; }
    return {nsb <= 1, ext};
}

// ---------------------------------------------------------------------------------------------- the prior by keyframe
// Column spans for the prior's workgroups on the keyframe-chain path (factor_kernels.hip, prior_chain_H_block / prior_rg_block): span[4 np], per prior
// column j four numbers -- [lo, hi) the columns of j's own keyframe, [plo, phi) those of the keyframe below it (0, 0 where the prior has none).
// Returns 1 when the layout can be walked by span: the columns of every keyframe are ONE run of at most PRIOR_SPAN_MAX (a pose and a speed/bias block
// side by side are 15).  The layouts after a loop closure, whose extra speed-bias blocks sit behind the poses, return 0: they keep the dense form.
#define PRIOR_SPAN_MAX 16
static inline int prior_span_tables(int W, int np, int nb, const int32_t* blk_slot, const int32_t* blk_kind, const int32_t* blk_idx, const int* colblk, int* span) {
    std::vector<int> lo(W, np), hi(W, 0), cols(W, 0);
    for (int b = 0; b < nb; ++b) {
        const int s = blk_slot[b], ls = blk_kind[b] == GLIO_BLK_SPEEDBIAS ? 9 : 3;
        if (s < 0 || s >= W) return 0;
        lo[s] = std::min(lo[s], blk_idx[b]); hi[s] = std::max(hi[s], blk_idx[b] + ls); cols[s] += ls;
    }
    int ok = 1;
    for (int s = 0; s < W; ++s) if (cols[s] > 0 && (hi[s] - lo[s] != cols[s] || cols[s] > PRIOR_SPAN_MAX)) ok = 0;
    for (int j = 0; j < np; ++j) {
        const int s = colblk[j] >= 0 && colblk[j] < nb ? blk_slot[colblk[j]] : -1;
        if (s < 0) { span[4 * j] = span[4 * j + 1] = span[4 * j + 2] = span[4 * j + 3] = 0; ok = 0; continue; }
        span[4 * j] = lo[s]; span[4 * j + 1] = hi[s];
        const bool below = s > 0 && cols[s - 1] > 0;
        span[4 * j + 2] = below ? lo[s - 1] : 0; span[4 * j + 3] = below ? hi[s - 1] : 0;
    }
    return ok;
}
// Is every entry of the prior's Jacobian outside its keyframe's diagonal block an EXACT zero (of either sign)?  Then r = r0 + J0 dx and v = J0^T r
// can skip those products: they add +-0 to sums that start at +0, which changes no bit for a finite state.  (prior_is_chain above holds J0^T J0 to a
// tolerance only, which is enough for the solver's path and not for this.)
static inline int prior_jac_is_block_exact(int np, const double* lin_jac, const int32_t* blk_slot, const int* colblk) {
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < np; ++j)
            if (lin_jac[(size_t)i * np + j] != 0.0 && blk_slot[colblk[i]] != blk_slot[colblk[j]]) return 0;
    return 1;
}

// ---------------------------------------------------------------------------------------------- kept layout of the next marginalization
// The poses of slots 1 .. W-1 and the speed/bias of slot 1 as ever ([T1 Q1 SB1 | T2 Q2 | ...], 6 (W - 1) + 9 columns), then the speed/bias of every
// slot s >= 2 that carries a speed-bias prior or has a speed-bias block in the installed prior, ascending, 9 columns each.  Returns their number;
// extra_slot[j] = s.
static inline int glio_marg_layout(int W, int sbp_n, int prior_n, const int* h_prior_index, short* extra_slot) {
    int ne = 0;
    for (int s = 2; s < W; ++s)
        if (s < sbp_n || (prior_n > 0 && h_prior_index[15 * s + 6] >= 0)) { if (extra_slot) extra_slot[ne] = (short)s; ++ne; }
    return ne;
}
struct KeptSize { int n, nb; };          // columns and blocks of a kept layout with ne such extra blocks
static inline KeptSize marg_kept_size(int W, int ne) { return {6 * (W - 1) + 9 + 9 * ne, 2 * (W - 1) + 1 + ne}; }
// the block tables of the next prior (GetParameterBlocks with addr_shift slot s -> s-1, Estimator.cpp:2584-2600) in that layout
static inline KeptSize marg_block_tables(int W, int sbp_n, int prior_n, const int* h_prior_index, const glio_state* s, int32_t* blk_slot, int32_t* blk_kind, int32_t* blk_idx, double* blk_x0) {
    const int ns = marg_kept_size(W, 0).n;
    short extra[GLIO_MAX_WINDOW];
    const int ne = glio_marg_layout(W, sbp_n, prior_n, h_prior_index, extra);
    int nb = 0;
    for (int k = 1; k < W; ++k) {
        const int kinds = k == 1 ? 3 : 2;
        for (int kind = 0; kind < kinds; ++kind) {
            blk_slot[nb] = k - 1; blk_kind[nb] = kind;
            blk_idx[nb] = k == 1 ? (kind == 0 ? 0 : (kind == 1 ? 3 : 6)) : 15 + 6 * (k - 2) + 3 * kind;
            const double* src = kind == 0 ? s->trans + 3 * k : (kind == 1 ? s->quat + 4 * k : s->speed_bias + 9 * k);
            const int gs = kind == 0 ? 3 : (kind == 1 ? 4 : 9);
            for (int j = 0; j < 9; ++j) blk_x0[9 * nb + j] = j < gs ? src[j] : 0.0;
            ++nb;
        }
    }
    for (int j = 0; j < ne; ++j, ++nb) {
        blk_slot[nb] = extra[j] - 1; blk_kind[nb] = GLIO_BLK_SPEEDBIAS; blk_idx[nb] = ns + 9 * j;
        for (int q = 0; q < 9; ++q) blk_x0[9 * nb + q] = s->speed_bias[9 * extra[j] + q];
    }
    return marg_kept_size(W, ne);
}

// ---------------------------------------------------------------------------------------------- GNSS
// Sort by (slot_i, slot_j), Doppler additionally by epoch; group = one slot pair.  A caller that builds the factors keyframe pair by keyframe pair
// (the reference's loop order, Estimator.cpp:2255-2421) hands them over sorted already: then nothing is copied or moved on the host, dd / dop are
// the caller's arrays and are staged for upload as they are (0.17 -> 0.06 ms per keyframe at 152 + 1520 factors).
struct GnssTables {
    const glio_dd_psr* dd = nullptr; const glio_doppler* dop = nullptr; size_t n_dd = 0, n_dop = 0;     // sorted: the caller's arrays, or the copies below
    std::vector<glio_dd_psr> dd_copy; std::vector<glio_doppler> dop_copy;                               // (empty unless the input was unsorted)
    std::vector<GnssGroup> groups; std::vector<DopRun> runs;
    // structure tables of the arrow solver: which keyframe slots each clock-drift epoch couples, and per slot (CSR off / list) the epochs touching it
    std::vector<EpochSlots> es; std::vector<int> off, list;
    int gnss_ok = 1;         // every Doppler run couples neighbouring keyframes (else: velocity coupling that is not tridiagonal)
    int gnss_chain = 1;      // every pair is (i, i + 1): one that skips a keyframe (or is listed upper keyframe first) breaks the chain
    int max_epoch = -1;      // largest clock-drift epoch a Doppler factor names
};
static inline int gnss_build_tables(int W, int n_ddt_max, int n_dd, const glio_dd_psr* dd, int n_dop, const glio_doppler* dop, GnssTables* t, TabError* e) {
    for (int k = 0; k < n_dd; ++k) if (const glio_dd_psr& f = dd[k]; f.slot_i < 0 || f.slot_i >= W || f.slot_j < 0 || f.slot_j >= W || f.slot_i == f.slot_j || f.n_sat < 2 || f.n_sat > GLIO_DD_MAX_SAT || f.master < 0 || f.master >= f.n_sat) return tab_refuse(e, TAB_E_ARG, "bad DD factor");
    for (int k = 0; k < n_dop; ++k) if (const glio_doppler& f = dop[k]; f.slot_i < 0 || f.slot_i >= W || f.slot_j < 0 || f.slot_j >= W || f.slot_i == f.slot_j || f.epoch < 0 || f.epoch >= n_ddt_max) return tab_refuse(e, TAB_E_ARG, "bad Doppler factor (epoch %d, max_ddt_epochs %d)", f.epoch, n_ddt_max);
    auto key = [W](int i, int j) { return i * W + j; };
    auto dd_less = [&](const glio_dd_psr& a, const glio_dd_psr& b) { return key(a.slot_i, a.slot_j) < key(b.slot_i, b.slot_j); };
    auto dop_less = [&](const glio_doppler& a, const glio_doppler& b) {
        const int ka = key(a.slot_i, a.slot_j), kb = key(b.slot_i, b.slot_j);
        return ka != kb ? ka < kb : a.epoch < b.epoch; };
    t->dd = dd; t->n_dd = (size_t)n_dd; t->dop = dop; t->n_dop = (size_t)n_dop;
    if (!std::is_sorted(dd, dd + n_dd, dd_less)) {
        t->dd_copy.assign(dd, dd + n_dd);
        std::stable_sort(t->dd_copy.begin(), t->dd_copy.end(), dd_less);
        t->dd = t->dd_copy.data();
    }
    if (!std::is_sorted(dop, dop + n_dop, dop_less)) {
        t->dop_copy.assign(dop, dop + n_dop);
        std::stable_sort(t->dop_copy.begin(), t->dop_copy.end(), dop_less);
        t->dop = t->dop_copy.data();
    }
    const glio_dd_psr* sdd = t->dd; const glio_doppler* sdop = t->dop;
    std::vector<GnssGroup>& groups = t->groups; std::vector<DopRun>& runs = t->runs;
    size_t a = 0, b = 0;
    while (a < t->n_dd || b < t->n_dop) {
        int k = 1 << 30;
        if (a < t->n_dd) k = std::min(k, key(sdd[a].slot_i, sdd[a].slot_j));
        if (b < t->n_dop) k = std::min(k, key(sdop[b].slot_i, sdop[b].slot_j));
        GnssGroup g;
        g.slot_i = k / W; g.slot_j = k % W;
        g.dd_begin = (int)a;
        while (a < t->n_dd && key(sdd[a].slot_i, sdd[a].slot_j) == k) ++a;
        g.dd_end = (int)a;
        g.dop_begin = (int)b;
        g.run_begin = (int)runs.size();
        while (b < t->n_dop && key(sdop[b].slot_i, sdop[b].slot_j) == k) {
            DopRun r;
            r.begin = (int)b; r.epoch = sdop[b].epoch; r.group = (int)groups.size();
            while (b < t->n_dop && key(sdop[b].slot_i, sdop[b].slot_j) == k && sdop[b].epoch == r.epoch) ++b;
            r.end = (int)b;
            runs.push_back(r);
        }
        g.dop_end = (int)b;
        g.run_end = (int)runs.size();
        groups.push_back(g);
    }
    // an epoch must belong to exactly one group (one clock-drift unknown per epoch, one bracketing pair)
    const int ne = std::max(1, n_ddt_max);
    { std::vector<int> seen(ne, 0); for (auto& r : runs) if (seen[r.epoch]++) return tab_refuse(e, TAB_E_ARG, "epoch %d appears under two keyframe pairs", r.epoch); }
    if ((int)groups.size() > W * W) { e->code = TAB_E_ARG; return TAB_E_ARG; }
    t->es.assign(ne, EpochSlots{-1, -1});
    std::vector<std::vector<int>> per(W);
    for (auto& g : groups) if (g.slot_j - g.slot_i != 1) t->gnss_chain = 0;
    for (auto& r : runs) {
        t->max_epoch = std::max(t->max_epoch, r.epoch);
        const GnssGroup& g = groups[r.group];
        const int lo = std::min(g.slot_i, g.slot_j), hi = std::max(g.slot_i, g.slot_j);
        t->es[r.epoch] = EpochSlots{lo, hi};
        per[lo].push_back(r.epoch); per[hi].push_back(r.epoch);
        if (hi - lo != 1) t->gnss_ok = 0;
    }
    t->off.assign(W + 1, 0);
    for (int i = 0; i < W; ++i) { t->off[i + 1] = t->off[i] + (int)per[i].size(); t->list.insert(t->list.end(), per[i].begin(), per[i].end()); }
    return 0;
}

static inline void ecef2rotation_host(const double xyz[3], double R[9]) {   // gnss_utility.cpp:347-390,738-748
    const double e2 = 6.69437999014e-3, a = 6378137.0, R2D = 180.0 / M_PI, D2R = M_PI / 180.0;
    const double a2 = a * a, b2 = a2 * (1 - e2), b = sqrt(b2), ep2 = (a2 - b2) / b2;
    const double p = sqrt(xyz[0] * xyz[0] + xyz[1] * xyz[1]);
    double s1 = xyz[2] * a, s2 = p * b, h = sqrt(s1 * s1 + s2 * s2);
    const double st = s1 / h, ct = s2 / h;
    s1 = xyz[2] + ep2 * b * pow(st, 3);
    s2 = p - a * e2 * pow(ct, 3);
    const double lat = (atan(s1 / s2) * R2D) * D2R, lon = (atan2(xyz[1], xyz[0]) * R2D) * D2R;
    const double sl = sin(lat), cl = cos(lat), so = sin(lon), co = cos(lon);
    R[0] = -so; R[1] = -sl * co; R[2] = cl * co;
    R[3] = co;  R[4] = -sl * so; R[5] = cl * so;
    R[6] = 0;   R[7] = cl;       R[8] = sl;
}
// R_ecef_local = R_ecef_enu(anchor) * Rz(yaw)  (dd_psr_factor.hpp:33-45)
static inline void ecef_local_rotation(const double anc[3], double yaw, double R[9]) {
    double Ree[9];
    ecef2rotation_host(anc, Ree);
    const double s = sin(yaw), co = cos(yaw);
    const double Rel[9] = {co, -s, 0, s, co, 0, 0, 0, 1};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
        double a = 0;
        for (int k = 0; k < 3; ++k) a += Ree[i * 3 + k] * Rel[k * 3 + j];
        R[i * 3 + j] = a;
    }
}

// ---------------------------------------------------------------------------------------------- IMU
static inline bool inv15(const double* A_in, double* Ainv) {
    double A[225];
    memcpy(A, A_in, sizeof A);
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) Ainv[i * 15 + j] = i == j;
    for (int c = 0; c < 15; ++c) {
        int piv = c; double best = fabs(A[c * 15 + c]);
        for (int r = c + 1; r < 15; ++r) if (fabs(A[r * 15 + c]) > best) { best = fabs(A[r * 15 + c]); piv = r; }
        if (best == 0.0) return false;
        if (piv != c) for (int j = 0; j < 15; ++j) { std::swap(A[c * 15 + j], A[piv * 15 + j]); std::swap(Ainv[c * 15 + j], Ainv[piv * 15 + j]); }
        const double d = A[c * 15 + c];
        for (int j = 0; j < 15; ++j) { A[c * 15 + j] /= d; Ainv[c * 15 + j] /= d; }
        for (int r = 0; r < 15; ++r) {
            if (r == c) continue;
            const double f = A[r * 15 + c];
            if (f == 0.0) continue;
            for (int j = 0; j < 15; ++j) { A[r * 15 + j] -= f * A[c * 15 + j]; Ainv[r * 15 + j] -= f * Ainv[c * 15 + j]; }
        }
    }
    return true;
}
// sqrt_info = LLT(cov^-1).matrixL().transpose()  (ImuFactor.h:44-45) -- the reference recomputes this on
// the CPU in every Evaluate; it only depends on the pre-integration, so it is digested once at upload (Q5).
static inline bool digest_edge(const glio_preint* p, int slot, ImuEdgeDev* e) {
    memset(e, 0, sizeof *e);
    memcpy(e->delta_p, p->delta_p, 24); memcpy(e->delta_q, p->delta_q, 32); memcpy(e->delta_v, p->delta_v, 24);
    memcpy(e->lin_ba, p->linearized_ba, 24); memcpy(e->lin_bg, p->linearized_bg, 24);
    e->sum_dt = p->sum_dt; e->slot_i = slot;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            e->dp_dba[r * 3 + c] = p->jacobian[(0 + r) * 15 + 9 + c];
            e->dp_dbg[r * 3 + c] = p->jacobian[(0 + r) * 15 + 12 + c];
            e->dq_dbg[r * 3 + c] = p->jacobian[(3 + r) * 15 + 12 + c];
            e->dv_dba[r * 3 + c] = p->jacobian[(6 + r) * 15 + 9 + c];
            e->dv_dbg[r * 3 + c] = p->jacobian[(6 + r) * 15 + 12 + c];
        }
    double I[225];
    if (!inv15(p->covariance, I)) return false;
    for (int j = 0; j < 15; ++j) {           // lower Cholesky of the (lower triangle of the) inverse
        double d = I[j * 15 + j];
        for (int k = 0; k < j; ++k) d -= I[j * 15 + k] * I[j * 15 + k];
        if (!(d > 0.0)) return false;
        d = sqrt(d);
        I[j * 15 + j] = d;
        for (int i = j + 1; i < 15; ++i) {
            double s = I[i * 15 + j];
            for (int k = 0; k < j; ++k) s -= I[i * 15 + k] * I[j * 15 + k];
            I[i * 15 + j] = s / d;
        }
    }
    for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) e->sqrt_info[i * 15 + j] = j >= i ? I[j * 15 + i] : 0.0;
    return true;
}

// ---------------------------------------------------------------------------------------------- pinned upload arena
// A set_* call stages every table in ONE pinned block [segment descriptors (1 KB) | payloads, 64-byte aligned]; the block goes to its device mirror
// with ONE asynchronous copy and ONE kernel moves every segment to its destination (device-to-device segments -- results a kernel left in a
// workspace -- ride along): two operations per call instead of one copy per table.  A StageBatch is the state of one such call, a local of it; the
// functions below say where in the pinned block to memcpy a table and what to enqueue, capi.hip does both.
#define STAGE_HEADER 1024
#define STAGE_DIRECT_BYTES 16384
#define STAGE_MAX_SEGS 32
struct StageSegDev { void* dst; const void* src; size_t bytes; };          // what k_unstage reads, one per workgroup row
static_assert(sizeof(StageSegDev) * STAGE_MAX_SEGS <= STAGE_HEADER, "descriptor header");
struct StageBatch {
    char* h = nullptr; char* d = nullptr;          // the pinned block and its device mirror
    size_t cap = 0, used = 0, top = 0;             // payloads fill [STAGE_HEADER, used); tables sent on their own are taken top-down from [top, cap)
    int n_seg = 0, early = -1; StageSegDev seg[STAGE_MAX_SEGS];          // early: which of the two early arenas the block is, -1: the context's own
};
// the block a batch of `payload` bytes wants: header, payloads, the alignment of each of up to 34 pieces
static inline size_t stage_block_bytes(size_t payload) { return payload + STAGE_HEADER + 64 * 34; }
static inline void stage_open(StageBatch* b, char* h, char* d, size_t cap, int early) {
    b->h = h; b->d = d; b->cap = cap; b->used = STAGE_HEADER; b->top = cap & ~(size_t)63; b->n_seg = 0; b->early = early;
}
static inline int stage_overflow(TabError* e) { return tab_refuse(e, TAB_E_STATE, "upload arena overflow"); }
// Where a host table of `bytes` goes.  at: the place in the pinned block to memcpy it to.  direct: the caller enqueues a copy of its own from `at`
// to dst -- a large table goes straight to its destination (the copy engine beats a second pass over it), its pinned copy taken from the TOP of the
// block, outside the part the batch sends; an early batch has no such part (its block travels on another stream).  Else the table is a segment.
struct StagePlace { char* at; bool direct; };
static inline int stage_place(StageBatch* b, void* dst, size_t bytes, StagePlace* p, TabError* e) {
    if (bytes > STAGE_DIRECT_BYTES && b->early < 0) {
        const size_t need = (bytes + 63) & ~(size_t)63;
        if (b->top < need || b->top - need < b->used) return stage_overflow(e);
        b->top -= need;
        *p = {b->h + b->top, true};
        return 0;
    }
    const size_t off = (b->used + 63) & ~(size_t)63;
    if (off + bytes > b->top || b->n_seg >= STAGE_MAX_SEGS || (bytes & 3)) return stage_overflow(e);
    b->used = off + bytes;
    b->seg[b->n_seg++] = {dst, b->d + off, bytes};
    *p = {b->h + off, false};
    return 0;
}
// a device-to-device segment of the same batch
static inline int stage_place_d2d(StageBatch* b, void* dst, const void* src, size_t bytes, TabError* e) {
    if (b->n_seg >= STAGE_MAX_SEGS || (bytes & 3)) return stage_overflow(e);
    b->seg[b->n_seg++] = {dst, src, bytes};
    return 0;
}
// four pinned bytes behind the payloads for a result the device writes back (glio_marginalize_keep_async's "positive definite" flag), on a line of
// their own; null when the block has no room
static inline char* stage_result_word(StageBatch* b) {
    const size_t off = (b->used + 63) & ~(size_t)63;
    if (off + 4 > b->top) return nullptr;
    b->used = off + 4;
    return b->h + off;
}

// mdb_hnsw_route.h — which kernels an HNSW search call launches, decided in ONE place.
//
// hnsw_route(shape, call, opts) is a pure function: no mdb_ctx, no HIP call, no environment.  It returns the ordered list of
// launches of the call (kernel family, template arguments, grid, block, dynamic LDS), the scratch the call takes and the facts its
// callers need back.  HnswSet::search (mdb_hnsw.hip) and hnsw_upper_run (mdb_hnsw_upper.hip) only EXECUTE a route: they take the
// scratch it sizes, build the kernel arguments and walk the list.  mdb_hnsw_describe_search prints it; tests/host/hnsw_route_main.cpp
// runs this header alone under the host sanitizers.  Every condition of the dispatch is written once, here; DESIGN.md holds the
// table of forms against conditions.
//
// The LDS-size formulas that host and kernels share live here as constexpr functions (the kernel files include this header).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mdb_files.h"   // MDB_TILE, MDB_MAX_K, DistPlan / make_plan, the status / metric / quantizer constants

// ------------------------------------------------------------------------------------------ shared with the kernels
#define HNSW_BLOCK 256
#ifndef MDB_HNSW_L0_BLOCK
#define MDB_HNSW_L0_BLOCK 512
#endif
constexpr int beam_block(bool l0) { return l0 ? MDB_HNSW_L0_BLOCK : HNSW_BLOCK; }
// hnsw_beam_kernel: W (the sorted working set of the result: 64 NB keys rounded to 2 / 4 KB) | C 1024 keys | nb_id | nb_dist | misc | qs | vis
constexpr int beam_lds_c(int nb) { return nb <= 5 ? 2048 : 4096; }
constexpr int beam_lds_qs(int nb) { return beam_lds_c(nb) + 8192 + 1024 + 1024 + 64; }

#define UP_BLOCK 256             // hnsw_upper_kernel and the top launches
#define UP_LDS_VIS 6656          // their visited set sits behind the staging areas (mdb_hnsw_upper.hip)
#define T64_PPW 16               // hnsw_upper_table64_kernel: points per wave
#define PQ8_VQ 8                 // pq_quantize8_kernel: vectors per wave

// sorted positions (mdb_hnsw_rank.hip.h)
#define RK_MAX_POINTS 32768u     // 15-bit ranks / compact indices + the tie flag in one u16
#define RK_BLOCK 1024
#define RK_HIST_WORDS(NT) ((NT) / 64 * 256)
constexpr size_t rk_lds_bytes(uint32_t vis_words, uint32_t nu_pad, int nt, uint32_t extra_words) {
    return UP_LDS_VIS + (size_t)vis_words * 4 + (size_t)nu_pad * 4 + (size_t)RK_HIST_WORDS(nt) * 4 + 64 * 4 + (size_t)extra_words * 4;
}

// the frontier form (mdb_hnsw_closure.hip.h)
#define CL_FR_CAP 512u           // a frontier list: certain points are fewer than ef <= 448; theta = +inf only over <= max(ef, 64) points
#define CL_SUBHIST 4             // histograms of the select (waves spread over them)
#define CL_SH_WORDS 32           // shared words of the block (CL_SH_*)
constexpr size_t cl_lds_words(uint32_t vis_words, uint32_t out_words, uint32_t row_words) {
    return (size_t)CL_SH_WORDS + CL_SUBHIST * 256 + 2 * CL_FR_CAP + 3 * (size_t)vis_words + out_words + row_words;
}
// roles of a launch in the fallback protocol (HnswUpArgs::fb_role)
#define CL_ROLE_NONE 0
#define CL_ROLE_TOP 1            // closure, the split path's top launch: fb[q] = flagged (the counter words are being cleared by this very launch)
#define CL_ROLE_BOTTOM 2         // closure behind CL_ROLE_TOP / _TOP_LOCAL: a query left flagged above is skipped; counted when flagged here or above
#define CL_ROLE_SINGLE 3         // closure over every upper layer: fb[q] = flagged, counted
#define CL_ROLE_FALLBACK 4       // the sequential kernels: blocks of unflagged queries exit at once
#define CL_ROLE_TOP_LOCAL 5      // CL_ROLE_TOP whose block re-runs a flagged query itself, on sorted positions: every query is handed over,
                                 // fb[q] = CL_FB_COUNT marks the flagged ones for the launch below to count

// hnsw_closure_kernel (graphs no larger than ef): its dynamic LDS and what it stages there up front
struct ClosureStage {
    uint32_t dtab_off, rows0_off, rowsU_off;   // byte offsets into the block's LDS; 0 = not staged
};
constexpr size_t closure_lds_base(int wcap, int dpad, uint32_t max_n) {
    return (size_t)wcap * 16 + (size_t)dpad * 4 + 8 + 64 + (((size_t)max_n + 31) / 32 + 1) * 4;
}

// ------------------------------------------------------------------------------------------ LDS ceilings
constexpr size_t HNSW_LDS_ONE_BLOCK = 160 * 1024 - 512;   // a launch with one block per CU
constexpr size_t HNSW_LDS_TWO_BLOCKS = 80 * 1024 - 512;   // two blocks per CU: the table blocks of a top launch share the CU with its traversals
constexpr size_t HNSW_LDS_LAYER0 = 160 * 1024 - 256;      // the layer-0 kernels: visited set in LDS up to here, in global memory beyond
constexpr size_t HNSW_LDS_STAGE = 120 * 1024;             // hnsw_closure_kernel's 1024-thread block: what it may stage
constexpr size_t HNSW_TABLE_VIS_MAX = 96 * 1024;          // table path: the visited bitmap over the upper points
constexpr uint64_t HNSW_TABLE_MAX_BYTES = (uint64_t)2 << 30;

// ------------------------------------------------------------------------------------------ inputs
// what the dispatch reads of a loaded HnswSet / HnswUpper
struct HnswShape {
    int kind = MDB_QUANT_NONE, metric = MDB_METRIC_L2;
    uint32_t dimension = 0;
    int dpad = 0;
    uint32_t max_n = 0, max_stride = 0, max_rows0 = 0, max_rowsU = 0;
    bool all_dense = true;
    int pq_m = 0, pq_K = 0, pq_subdim = 0;
    uint32_t nu = 0, nu2 = 0, su = 0, layers = 0, small_layer = 0;
    uint64_t ntiles = 0, ntiles2 = 0;
    bool rows_nat = false, map21 = false;
};
struct HnswCall {
    uint64_t b = 0, k = 0;
    uint32_t ef = 0;
    int qstride = 0;            // floats between two query rows (a PQ call's decoded rows take the same stride)
    bool per_query_users = false;
    bool fuse = false;          // the caller offers a fused remap (HnswRemapOut with a doc array)
    bool filter = false;        // the caller offers a ratio filter (ClosureFilter with probes)
};
// the options the dispatch reads (mdb_options of the same names, same defaults: HnswSet::route_opts fills them)
#define HNSW_ROUTE_OPTS(X)                                                                                                       \
    X(hnsw_generic_dist, 0) X(closure_no_filter, 0) X(closure_no_stage, 0) X(hnsw_no_closure, 0) X(closure_block, 0)            \
    X(hnsw_no_beam, 0) X(hnsw_no_row64, 0) X(hnsw_no_table, 0) X(hnsw_table_qt, 4) X(hnsw_table_no_lds, 0)                      \
    X(hnsw_table64_min_b, 32) X(hnsw_no_wide, 0) X(hnsw_rank, 2) X(hnsw_closure, 1) X(hnsw_no_split, 0) X(hnsw_table_min_b, 1)  \
    X(hnsw_nb4_slack, 48) X(pq_no_quantize8, 0)
struct HnswRouteOpts {
#define X(field, dflt) long long field = dflt;
    HNSW_ROUTE_OPTS(X)
#undef X
};

// ------------------------------------------------------------------------------------------ the route
enum HnswRole { HR_PQ_QUANTIZE, HR_PQ_ROWS, HR_TABLE, HR_TOP, HR_LAYER1, HR_FALLBACK, HR_LAYER0, HR_CLOSURE };
enum HnswKernel {
    HK_PQ_QUANTIZE8, HK_PQ_QUANTIZE, HK_PQ_ROWS, HK_CLOSURE, HK_BEAM, HK_SEARCH, HK_TABLE64, HK_TABLE16, HK_TABLE, HK_TOP_RANK,
    HK_TOP, HK_UPPER_RANK, HK_UPPER
};
struct HnswKernelInfo {
    const char* name;
    int ntarg;
    unsigned bool_mask;   // bit i: template argument i is a bool
};
inline const HnswKernelInfo& hnsw_kernel_info(HnswKernel k) {
    static const HnswKernelInfo info[] = {
        {"pq_quantize8_kernel", 0, 0},          // HK_PQ_QUANTIZE8
        {"pq_quantize_kernel", 0, 0},           // HK_PQ_QUANTIZE
        {"pq_rows_kernel", 0, 0},               // HK_PQ_ROWS
        {"hnsw_closure_kernel", 3, 0},          // <METRIC, N16T, BLOCK>
        {"hnsw_beam_kernel", 6, 2 | 8 | 16},    // <METRIC, VIS_LDS, N16T, ROW64, L0, NB>
        {"hnsw_search_kernel", 3, 2},           // <METRIC, VIS_LDS, N16T>
        {"hnsw_upper_table64_kernel", 2, 0},    // <METRIC, N16>
        {"hnsw_upper_table16_kernel", 2, 0},    // <METRIC, QT>
        {"hnsw_upper_table_kernel", 2, 0},      // <METRIC, QT>
        {"hnsw_upper_top_rank_kernel", 3, 0},   // <METRIC, N16, NW>
        {"hnsw_upper_top_kernel", 3, 0},        // <METRIC, N16, NB>
        {"hnsw_upper_rank_kernel", 1, 0},       // <NW>
        {"hnsw_upper_kernel", 2, 1},            // <TLDS, NB>
    };
    return info[k];
}
inline const char* hnsw_role_name(HnswRole r) {
    static const char* const names[] = {"pq_quantize", "pq_rows", "table", "top", "layer1", "fallback", "layer0", "closure"};
    return names[r];
}

struct HnswLaunch {
    HnswRole role;
    HnswKernel kernel;
    int targ[6];             // template arguments in the kernel's order (bools as 0 / 1)
    uint32_t gx, gy, block;
    size_t lds;              // dynamic LDS bytes
    // what the executor's argument builder needs besides
    uint32_t q_first;        // table kernels: first query of this launch (the remainder launch)
    bool zero16;             // this launch clears the context's traversal counters on its way
    int layer_hi;            // traversal launches: the highest layer they traverse
    bool handover;           // they start from the state the launch above handed over
    int fb_role;             // CL_ROLE_*
    bool cl_tlds;            // frontier form behind the table: the query's row is copied into LDS
};
#define HNSW_ROUTE_MAX_LAUNCHES 8

struct HnswRoute {
    mdb_status status = MDB_OK;
    uint32_t ef = 0;         // as normalised (0 -> 1)
    int n = 0;
    HnswLaunch launch[HNSW_ROUTE_MAX_LAUNCHES];
    // ---- layer-0 kernels' sizes (HnswArgs)
    int ef_cap = 0, cand_cap = 0, smax = 0;
    uint32_t vis_words = 0;
    bool vis_lds = true;
    size_t vis_bytes = 0;    // the global visited set (0 when it is in LDS): b * vis_words words, cleared by a memset
    // ---- table path: scratch sizes in bytes and the word offsets of the fields inside them
    bool table = false;
    uint32_t nu_pad = 0, nu2_pad = 0;
    uint32_t up_words = 0, up_words2 = 0;   // visited bitmap over the upper points / the TOP set
    size_t table_bytes = 0;  // [b][nu_pad] distance images
    size_t out_bytes = 0;    // upper output state: ep [b] | ovf [b] | cnt [b][4] | vis [b][up_words]
    size_t hand_bytes = 0;   // hand-over between the upper launches: the same fields, then fb [b]
    size_t st_ovf = 0, st_cnt = 0, st_vis = 0, st_fb = 0;   // word offsets (ep at 0); st_fb in the hand-over state only
    bool local = false;      // frontier form: the top blocks re-run their flagged queries themselves
    // ---- what the callers get back
    bool fuse_done = false;  // the layer-0 launch writes the caller's (doc id, score) rows itself
    bool cf_done = false;    // the closure kernel applies the caller's ratio filter in its tail
    // ---- hnsw_closure_kernel
    int wcap = 0;
    ClosureStage stage{0u, 0u, 0u};
};

// registers of 64 beam slots on the table path: every count, selection and push of a step loops over them — four when ef leaves
// them enough slack (a compaction every ~slack accepted neighbours costs less than a fifth register in every step; the slack is also
// the exact ties with furthest a query may hold before it is re-run by the general kernel), five up to 256, eight beyond
inline int hnsw_route_nb(uint32_t ef, long long nb4_slack) {
    if (nb4_slack > 0 && (long long)ef + nb4_slack <= 256) return 4;
    return ef <= 256 ? 5 : 8;
}

inline HnswLaunch& hnsw_route_add(HnswRoute& r, HnswRole role, HnswKernel kernel, uint32_t gx, uint32_t gy, uint32_t block, size_t lds,
                                  int t0 = 0, int t1 = 0, int t2 = 0, int t3 = 0, int t4 = 0, int t5 = 0) {
    HnswLaunch& l = r.launch[r.n++];
    l = HnswLaunch{};
    l.role = role; l.kernel = kernel; l.gx = gx; l.gy = gy; l.block = block; l.lds = lds;
    l.targ[0] = t0; l.targ[1] = t1; l.targ[2] = t2; l.targ[3] = t3; l.targ[4] = t4; l.targ[5] = t5;
    l.fb_role = CL_ROLE_NONE;
    return l;
}

// quantization of n vectors (shared with the IVF-PQ paths: pq_quantize_device executes this launch)
inline void pq_quantize_route(HnswRoute& r, int m, int K, int subdim, uint64_t n, bool no_quantize8) {
    if (K == 256 && subdim == 8 && !no_quantize8) {
        const uint64_t groups = (n + PQ8_VQ - 1) / PQ8_VQ;
        hnsw_route_add(r, HR_PQ_QUANTIZE, HK_PQ_QUANTIZE8, (uint32_t)((groups + 3) / 4), (uint32_t)m, 256, 0);
    } else {
        hnsw_route_add(r, HR_PQ_QUANTIZE, HK_PQ_QUANTIZE, (uint32_t)((n * (uint64_t)m + 3) / 4), 1, 256, 0);
    }
}

// the distance table of every (query, upper point): lane = query for batches, thread = point below them
inline void hnsw_route_table(HnswRoute& r, const HnswShape& s, const HnswCall& c, const HnswRouteOpts& o, const DistPlan& p, int M,
                             bool table64) {
    const uint32_t b = (uint32_t)c.b;
    if (table64) {
        hnsw_route_add(r, HR_TABLE, HK_TABLE64, (s.nu + 4 * T64_PPW - 1) / (4 * T64_PPW), (b + 63) / 64, 256, 0, M, p.n16).zero16 = true;
        return;
    }
    const bool whole16 = p.n16 > 0 && p.n8 == 0 && p.n4 == 0 && p.ntail == 0;
    // whole 16-chunks: QF queries per pass of a tile; any other dimension: the cascade of exact_sums, two queries per pass
    const int qf = !whole16 ? 2 : o.hnsw_table_qt == 8 ? 8 : o.hnsw_table_qt == 2 ? 2 : 4;
    const HnswKernel kernel = whole16 ? HK_TABLE16 : HK_TABLE;
    const uint32_t gx = whole16 ? (uint32_t)((s.ntiles + 3) / 4) : (uint32_t)s.ntiles, block = whole16 ? 256 : 64;
    const uint32_t full = b / qf, rest = b % qf;
    if (full) hnsw_route_add(r, HR_TABLE, kernel, gx, full, block, 0, M, qf).zero16 = true;
    if (rest) {   // one query per pass for the remainder; the counters are cleared by whichever launch covers query 0
        HnswLaunch& l = hnsw_route_add(r, HR_TABLE, kernel, gx, rest, block, 0, M, 1);
        l.q_first = full * qf;
        l.zero16 = full == 0;
    }
}

// the launch over layers layer_hi .. 1, the last before layer 0: on sorted positions (the block sorts its table row and traverses by
// ranks: any ef, no beam registers), else the register beam on table lookups
inline void hnsw_route_bottom(HnswRoute& r, const HnswShape& s, const HnswCall& c, const HnswRouteOpts& o, HnswRole role, int layer_hi,
                              bool handover) {
    const uint32_t b = (uint32_t)c.b;
    const size_t rlds = rk_lds_bytes(r.up_words, r.nu_pad, RK_BLOCK, 0);
    HnswLaunch* l;
    if ((o.hnsw_rank & 1) && s.nu <= RK_MAX_POINTS && r.nu_pad <= RK_MAX_POINTS && rlds <= HNSW_LDS_ONE_BLOCK) {
        l = &hnsw_route_add(r, role, HK_UPPER_RANK, b, 1, RK_BLOCK, rlds, r.nu_pad <= 2048 ? 1 : r.nu_pad <= 8192 ? 4 : 16);
    } else {
        // TLDS: the query's table row is copied into LDS by the whole block first
        const size_t lds_base = UP_LDS_VIS + (size_t)r.up_words * 4;
        const bool tlds = lds_base + (size_t)r.nu_pad * 4 <= HNSW_LDS_ONE_BLOCK && !o.hnsw_table_no_lds;
        l = &hnsw_route_add(r, role, HK_UPPER, b, 1, UP_BLOCK, lds_base + (tlds ? (size_t)r.nu_pad * 4 : 0), tlds,
                            hnsw_route_nb(r.ef, o.hnsw_nb4_slack));
    }
    l->layer_hi = layer_hi;
    l->handover = handover;
    l->fb_role = role == HR_FALLBACK ? CL_ROLE_FALLBACK : CL_ROLE_NONE;
}

// the upper layers of a call on the table path (table, top, layer1 and fallback launches)
inline void hnsw_route_upper(HnswRoute& r, const HnswShape& s, const HnswCall& c, const HnswRouteOpts& o, const DistPlan& p, int M) {
    const uint32_t b = (uint32_t)c.b, words = r.up_words, words2 = r.up_words2, nu_pad = r.nu_pad, nu2_pad = r.nu2_pad;
    // lane = query table kernel: d = 16 n16 <= 128 with a row-major copy of the rows, batches from hnsw_table64_min_b on
    const bool table64 = s.rows_nat && p.n16 > 0 && p.n16 <= 8 && p.n8 == 0 && p.n4 == 0 && p.ntail == 0 && (long long)c.b >= o.hnsw_table64_min_b;
    // the split path: ONE top launch whose first b blocks traverse the layers >= 2 on a row they evaluate themselves while its other
    // blocks are that table pass; a bottom launch then takes layer 1 from the hand-over state
    const bool split = table64 && s.nu2 > 0 && s.layers >= 2 && !o.hnsw_no_split;
    const uint32_t top_grid = b + (s.nu + 4 * T64_PPW - 1) / (4 * T64_PPW) * ((b + 63) / 64);
    // top blocks on sorted positions: their LDS holds the row, its two rank tables and the sort's histograms
    const size_t lds_top_rank = rk_lds_bytes(words2, nu2_pad, 256, nu2_pad + words);
    const bool top_rank_fits = (o.hnsw_rank & 2) && lds_top_rank <= HNSW_LDS_TWO_BLOCKS;

    // ---- the frontier form (mdb_hnsw_closure.hip.h): table + top layers, layer 1, then the fallback launch for the flagged queries
    const size_t lds_row = cl_lds_words(words, 0, nu_pad) * 4, lds_norow = cl_lds_words(words, 0, 0) * 4;
    if (o.hnsw_closure && s.su <= 64 && s.layers >= 1 && lds_norow <= HNSW_LDS_ONE_BLOCK) {
        const bool tlds = lds_row <= HNSW_LDS_ONE_BLOCK && !o.hnsw_table_no_lds;
        const size_t lds_ctop = cl_lds_words(words2, words, nu2_pad) * 4;
        const bool csplit = split && lds_ctop <= HNSW_LDS_TWO_BLOCKS;
        // a top block re-runs its flagged query itself, on sorted positions (<= 2048 ranks), when its LDS holds that layout as well;
        // the fallback launch then has layer 1 alone to re-run, from the top launch's hand-over
        r.local = csplit && top_rank_fits && nu2_pad <= 2048;
        if (csplit) {
            HnswLaunch& t = hnsw_route_add(r, HR_TOP, HK_TOP_RANK, top_grid, 1, 256, r.local ? std::max(lds_top_rank, lds_ctop) : lds_ctop,
                                           M, p.n16, 1);
            t.zero16 = true;
            t.layer_hi = (int)s.layers;
            t.fb_role = r.local ? CL_ROLE_TOP_LOCAL : CL_ROLE_TOP;
        } else {
            hnsw_route_table(r, s, c, o, p, M, table64);
        }
        HnswLaunch& l1 = hnsw_route_add(r, HR_LAYER1, HK_UPPER_RANK, b, 1, RK_BLOCK, tlds ? lds_row : lds_norow, 1);
        l1.layer_hi = csplit ? 1 : (int)s.layers;
        l1.handover = csplit;
        l1.fb_role = csplit ? CL_ROLE_BOTTOM : CL_ROLE_SINGLE;
        l1.cl_tlds = tlds;
        // the sequential traversal for the flagged queries: of layer 1 alone when the top blocks resolve their own flags
        hnsw_route_bottom(r, s, c, o, HR_FALLBACK, r.local ? 1 : (int)s.layers, r.local);
        return;
    }
    // ---- the sequential kernels for every query
    const size_t lds_top = UP_LDS_VIS + (size_t)words2 * 4 + (size_t)nu2_pad * 4 + (size_t)words * 4;
    const bool top_beam = split && lds_top <= HNSW_LDS_ONE_BLOCK && r.ef <= 256;
    const bool top_rank = split && top_rank_fits && nu2_pad <= 8192;
    if (!top_beam && !top_rank) {
        hnsw_route_table(r, s, c, o, p, M, table64);
        hnsw_route_bottom(r, s, c, o, HR_LAYER1, (int)s.layers, false);
        return;
    }
    HnswLaunch& t = top_rank ? hnsw_route_add(r, HR_TOP, HK_TOP_RANK, top_grid, 1, 256, lds_top_rank, M, p.n16, nu2_pad <= 2048 ? 1 : 4)
                             : hnsw_route_add(r, HR_TOP, HK_TOP, top_grid, 1, 256, lds_top, M, p.n16, hnsw_route_nb(r.ef, o.hnsw_nb4_slack));
    t.zero16 = true;
    t.layer_hi = (int)s.layers;
    hnsw_route_bottom(r, s, c, o, HR_LAYER1, 1, true);
}

inline HnswRoute hnsw_route(const HnswShape& s, const HnswCall& c, const HnswRouteOpts& o) {
    HnswRoute r;
    r.ef = c.ef ? c.ef : 1;   // `len < ef` is never true and every push is followed by a pop: same as ef = 1
    if (c.b == 0) return r;
    if (r.ef > MDB_MAX_K * 2) { r.status = MDB_ERR_UNSUPPORTED; return r; }
    const uint32_t ef = r.ef, b = (uint32_t)c.b;
    const bool pq = s.kind == MDB_QUANT_PQ;
    if (pq) {
        // the query is quantized like a stored point and written out as its codebook rows
        pq_quantize_route(r, s.pq_m, s.pq_K, s.pq_subdim, c.b, o.pq_no_quantize8 != 0);
        hnsw_route_add(r, HR_PQ_ROWS, HK_PQ_ROWS, (uint32_t)((c.b * (uint64_t)c.qstride + 255) / 256), 1, 256, 0);
    }
    r.ef_cap = ((int)ef + 63) / 64 * 64;
    r.cand_cap = 1024;   // ring capacity (power of two): live candidates <= ef + ties; the beam kernel's sort / staging buffer fits as well
    while (r.cand_cap < r.ef_cap + 192) r.cand_cap <<= 1;
    r.smax = std::max<int>(64, ((int)s.max_stride + 63) / 64 * 64);
    size_t lds_base = (size_t)r.ef_cap * 8 + (size_t)r.cand_cap * 8 + (size_t)r.smax * 8 + (size_t)s.dpad * 4 + 64;
    if (ef <= 448) lds_base = std::max<size_t>(lds_base, (size_t)beam_lds_qs(ef <= 256 ? 5 : 8) + (size_t)s.dpad * 4);  // the beam kernel's fixed layout
    r.vis_words = (uint32_t)(((size_t)s.max_n + 31) / 32 + 1);
    r.vis_lds = lds_base + (size_t)r.vis_words * 4 <= HNSW_LDS_LAYER0;
    const size_t lds0 = lds_base + (r.vis_lds ? (size_t)r.vis_words * 4 : 0);
    if (!r.vis_lds) r.vis_bytes = (size_t)c.b * r.vis_words * 4;
    const DistPlan p = make_plan((int)s.dimension, s.metric);
    const int M = s.metric == MDB_METRIC_L2 ? MDB_METRIC_L2 : MDB_METRIC_DOT;
    // specialised distance when the whole vector is 16-lane chunks: instances for d = 128 and 768 (the configurations'), generic otherwise
    const int n16 = (!pq && p.n8 == 0 && p.n4 == 0 && p.ntail == 0 && !o.hnsw_generic_dist) ? p.n16 : 0;
    const int NF = n16 == 8 || n16 == 48 ? n16 : 0;

    // ---- graphs no larger than ef (SPANN centroid graphs): frontier-parallel closure, one launch
    if (s.max_n <= ef && s.max_n <= 4096 && !o.hnsw_no_closure) {
        r.wcap = 64;
        while ((uint32_t)r.wcap < s.max_n) r.wcap <<= 1;
        // small batches: 64 groups per query (latency); large ones: 256-thread blocks, four resident per CU
        const bool big = o.closure_block > 0 ? o.closure_block >= 1024 : c.b <= 256;
        size_t clds = closure_lds_base(r.wcap, s.dpad, s.max_n);
        // the SPANN ratio filter in the kernel's tail (k keys per query fit the frontier words: k <= wcap)
        r.cf_done = c.filter && !o.closure_no_filter && c.k <= (uint64_t)r.wcap;
        // staging: every point's distance up front + the rows in LDS, while the block keeps its residency.  Only the one-block-per-CU
        // form: with four 256-thread blocks per CU the rounds of one block already hide behind the others'
        if (!o.closure_no_stage && big) {
            clds = (clds + 15) & ~(size_t)15;
            if (clds + (size_t)s.max_n * 4 + 16 <= HNSW_LDS_STAGE) {
                r.stage.dtab_off = (uint32_t)clds;
                clds = (clds + (size_t)s.max_n * 4 + 15) & ~(size_t)15;
                if (s.max_rows0 && clds + (size_t)s.max_rows0 * 4 + 16 <= HNSW_LDS_STAGE) {
                    r.stage.rows0_off = (uint32_t)clds;
                    clds = (clds + (size_t)s.max_rows0 * 4 + 15) & ~(size_t)15;
                }
                if (s.max_rowsU && s.all_dense && clds + (size_t)s.max_rowsU * 4 + 16 <= HNSW_LDS_STAGE) {
                    r.stage.rowsU_off = (uint32_t)clds;
                    clds = (clds + (size_t)s.max_rowsU * 4 + 15) & ~(size_t)15;
                }
            }
        }
        hnsw_route_add(r, HR_CLOSURE, HK_CLOSURE, b, 1, big ? 1024 : 256, clds, M, NF, big ? 1024 : 256);
        return r;
    }
    // ef <= 256: register-resident beam; above: sorted LDS sets.  The table path's kernels exist with an 8-register beam as well
    // (512 slots): ef up to 448 stays off the general kernel there, which is 3x slower per expansion
    const bool beam = ef <= 256 && !o.hnsw_no_beam;
    const bool beam_wide = ef > 256 && ef <= 448 && !o.hnsw_no_beam && !o.hnsw_no_wide;
    const bool row64 = s.max_stride <= 64 && !o.hnsw_no_row64;   // hnsw_beam_kernel's one-chunk specialisation
    // upper layers on the distance table: one graph (no per-query user), f32 rows; the table is b * nu_pad words of scratch
    r.nu_pad = (uint32_t)s.ntiles * MDB_TILE;
    r.table = s.nu > 0 && !c.per_query_users && (beam || beam_wide) && row64 && !pq && !o.hnsw_no_table &&
              (long long)c.b >= o.hnsw_table_min_b && (uint64_t)c.b * r.nu_pad * 4 <= HNSW_TABLE_MAX_BYTES &&
              (size_t)(s.nu / 32 + 4) * 4 <= HNSW_TABLE_VIS_MAX;
    if (r.table) {
        r.nu2_pad = (uint32_t)s.ntiles2 * MDB_TILE;
        r.up_words = (s.nu / 32 + 4) & ~3u;   // a multiple of 4: hnsw_upper_kernel puts the table row's LDS copy (16-byte stores) behind the bitmap
        r.up_words2 = (s.nu2 / 32 + 4) & ~3u;
        r.table_bytes = (size_t)c.b * r.nu_pad * 4 + 64;
        r.out_bytes = (size_t)c.b * (r.up_words + 6) * 4 + 64;
        r.hand_bytes = ((size_t)c.b * (r.up_words + 8) + 64) * 4;
        r.st_ovf = c.b; r.st_cnt = 2 * c.b; r.st_vis = 6 * c.b; r.st_fb = c.b * (r.up_words + 6);
        hnsw_route_upper(r, s, c, o, p, M);
        r.fuse_done = c.fuse && c.k > 0;
        hnsw_route_add(r, HR_LAYER0, HK_BEAM, b, 1, beam_block(true), lds0, M, r.vis_lds, NF, true, true, hnsw_route_nb(ef, o.hnsw_nb4_slack));
    } else if (beam) {
        hnsw_route_add(r, HR_LAYER0, HK_BEAM, b, 1, HNSW_BLOCK, lds0, M, r.vis_lds, NF, row64, false, 5);
    } else {   // (a beam_wide call without the table lands here)
        hnsw_route_add(r, HR_LAYER0, HK_SEARCH, b, 1, HNSW_BLOCK, lds0, M, r.vis_lds, NF);
    }
    return r;
}

// ------------------------------------------------------------------------------------------ text
// `hnsw_beam_kernel<0, true, 8, true, true, 5>`: the key a code object's symbol and a profiler's kernel name reduce to
inline int hnsw_kernel_key(const HnswLaunch& l, char* buf, size_t len) {
    const HnswKernelInfo& ki = hnsw_kernel_info(l.kernel);
    int w = snprintf(buf, len, "%s", ki.name);
    for (int i = 0; i < ki.ntarg && w >= 0 && (size_t)w < len; ++i) {
        const char* sep = i == 0 ? "<" : ", ";
        if (ki.bool_mask >> i & 1) w += snprintf(buf + w, len - w, "%s%s", sep, l.targ[i] ? "true" : "false");
        else w += snprintf(buf + w, len - w, "%s%d", sep, l.targ[i]);
    }
    if (ki.ntarg && w >= 0 && (size_t)w < len) w += snprintf(buf + w, len - w, ">");
    return w;
}
// one launch per line: `role kernel_key gx,gy block lds`.  Returns the length of the whole text (as snprintf: it was cut when >= len)
inline size_t hnsw_route_text(const HnswRoute& r, char* buf, size_t len) {
    size_t w = 0;
    if (len) buf[0] = 0;
    for (int i = 0; i < r.n; ++i) {
        const HnswLaunch& l = r.launch[i];
        char key[96];
        hnsw_kernel_key(l, key, sizeof key);
        const int n = snprintf(w < len ? buf + w : nullptr, w < len ? len - w : 0, "%s %s %u,%u %u %zu\n", hnsw_role_name(l.role), key, l.gx,
                               l.gy, l.block, l.lds);
        if (n > 0) w += (size_t)n;
    }
    return w;
}
// the shape as the `key=value` words tests/host/hnsw_route_main.cpp reads
inline size_t hnsw_shape_text(const HnswShape& s, char* buf, size_t len) {
    const int n = snprintf(buf, len,
                           "kind=%d metric=%d dimension=%u dpad=%d max_n=%u max_stride=%u max_rows0=%u max_rowsU=%u all_dense=%d pq_m=%d pq_K=%d "
                           "pq_subdim=%d nu=%u nu2=%u su=%u layers=%u small_layer=%u ntiles=%llu ntiles2=%llu rows_nat=%d map21=%d",
                           s.kind, s.metric, s.dimension, s.dpad, s.max_n, s.max_stride, s.max_rows0, s.max_rowsU, (int)s.all_dense, s.pq_m,
                           s.pq_K, s.pq_subdim, s.nu, s.nu2, s.su, s.layers, s.small_layer, (unsigned long long)s.ntiles,
                           (unsigned long long)s.ntiles2, (int)s.rows_nat, (int)s.map21);
    return n > 0 ? (size_t)n : 0;
}

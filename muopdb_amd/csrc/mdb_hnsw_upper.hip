// mdb_hnsw_upper.hip — the UPPER layers of BlockBasedHnsw::ann_search (hnsw/block_based/index.rs:159-190) as a table pass
// plus a single-wave traversal.
//
// The reference runs search_layer with the full ef on EVERY layer (index.rs:174-186), so 60 % of a query's node expansions
// happen on layers >= 1 — which together hold only ~n/31 points (32 k of 1 M).  Instead of gathering neighbour vectors step by
// step there, one streaming pass evaluates every (query, upper point) distance with the exact lane association
// (hnsw_upper_table_kernel: the flat scan's thread-per-vector exact_sums over SoA tiles, queries as scalar operands; 16 MB read
// once per batch, QT queries per load) and the traversal of those layers becomes bookkeeping on table lookups:
//   * one WAVE per query, no block barrier, no distance waves, no LDS hand-off: the step's visited test-and-set (LDS atomics)
//     and its table lookups are issued together and land while the wave selects the runner-up and requests its row;
//   * the neighbours stay in their row lanes (lane = edge slot): no ordered compaction — the acceptance-by-counting lemma of
//     hnsw_beam_kernel only needs edge order = lane order;
//   * everything is indexed by COMPACT index (ascending point id, so tie-breaks are unchanged): 4 KB visited bitmap per query.
// The evaluation / expansion counters count lookups exactly where the reference evaluates a distance, the visited set (shared by
// the layers, index.rs:172) is handed to the layer-0 kernel as a bitmap over compact indices, and a query whose beam overflows
// (> ~120 exact ties with furthest) is flagged for the general traversal there.  Rows, score bits and both counters equal the
// all-in-one kernel's and the oracle's (tests/test_gpu_traversal.py, test_gpu_fullsize.py).
#include "mdb_hnsw.h"
#include "mdb_hnsw_dev.hip.h"
#include "mdb_kernels.h"
#include "mdb_launch.hip.h"

// ------------------------------------------------------------------------------------------ table
// grid (tiles, query groups of QT); one wave = one tile of 64 upper points, thread = point
template <int METRIC, int QT>
__global__ __launch_bounds__(64) void hnsw_upper_table_kernel(const float4* __restrict__ tiles, uint32_t nu, DistPlan p,
                                                              const float* __restrict__ q, int qstride, uint32_t q_first,
                                                              uint32_t* __restrict__ table, uint32_t nu_pad, unsigned long long* zero16) {
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    if (zero16 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 16) zero16[threadIdx.x] = 0ull;
    const uint32_t v = tile * MDB_TILE + lane;
    const uint32_t q0 = q_first + blockIdx.y * QT;
    float raw[QT];
#pragma unroll
    for (int i = 0; i < QT; ++i) raw[i] = 0.0f;
    if (v < nu) {
        TileLoader ld{tiles + (size_t)tile * p.d4 * MDB_TILE + lane};
        exact_sums<METRIC, QT, TileLoader, 0>(ld, q + (size_t)q0 * qstride, qstride, p, raw);
    }
#pragma unroll
    for (int i = 0; i < QT; ++i)
        table[(size_t)(q0 + i) * nu_pad + v] = v < nu ? f32_orderable(finish_distance<METRIC>(raw[i])) : SLOT_EMPTY;
}

// d = 16 * n16 (128, 768: the configurations' dimensions).  One wave = one tile, thread = point, QT queries per pass of the tile.
// The 16 lane accumulators of the reference per (query, point) stay in registers (QT * 16).  A query's 16-float chunk is ONE
// register (lane l holds element l % 16: a 64-byte load replicated over the four 16-lane rows) and reaches the arithmetic as the
// DPP operand of the subtract / multiply itself (row_newbcast:j = element j to every lane of the row): no scalar loads (exact_sums
// <QT = 8> takes 264-286 VGPRs and spills scalars; its s_load -> s_waitcnt lgkmcnt(0) per chunk left the SIMDs idle 80 % of the
// time), no LDS, 3 VALU per element and query.  Two register buffers of the tile's chunks: the next chunk's loads are in flight
// while the current one is accumulated.
#define MDB_T16_TERM(J)                                                                                                     \
    if (METRIC != MDB_METRIC_DOT) {                                                                                         \
        float df;                                                                                                           \
        asm("v_sub_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "=v"(df) : "v"(vq), "v"(xv[J]));     \
        ac[J] = __fadd_rn(ac[J], __fmul_rn(df, df));                                                                        \
    } else {                                                                                                                \
        float pr;                                                                                                           \
        asm("v_mul_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "=v"(pr) : "v"(vq), "v"(xv[J]));     \
        ac[J] = __fadd_rn(ac[J], pr);                                                                                       \
    }
template <int METRIC>
__device__ __forceinline__ void t16_accumulate(float (&ac)[16], const float vq, const float (&xv)[16]) {
    MDB_T16_TERM(0) MDB_T16_TERM(1) MDB_T16_TERM(2) MDB_T16_TERM(3) MDB_T16_TERM(4) MDB_T16_TERM(5) MDB_T16_TERM(6) MDB_T16_TERM(7)
    MDB_T16_TERM(8) MDB_T16_TERM(9) MDB_T16_TERM(10) MDB_T16_TERM(11) MDB_T16_TERM(12) MDB_T16_TERM(13) MDB_T16_TERM(14) MDB_T16_TERM(15)
}
#undef MDB_T16_TERM

template <int METRIC, int QT>
__global__ __launch_bounds__(256) void hnsw_upper_table16_kernel(const float4* __restrict__ tiles, uint32_t nu, uint32_t ntiles, int n16,
                                                                 const float* __restrict__ q, int qstride, uint32_t q_first,
                                                                 uint32_t* __restrict__ table, uint32_t nu_pad, unsigned long long* zero16) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (zero16 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 16) zero16[threadIdx.x] = 0ull;
    const uint32_t tile = blockIdx.x * 4 + wave;
    if (tile >= ntiles) return;
    const uint32_t v = tile * MDB_TILE + lane;
    const float4* tp = tiles + (size_t)tile * (4 * n16) * MDB_TILE + lane;
    const uint32_t q0 = q_first + blockIdx.y * QT;
    const float* __restrict__ ql = q + (size_t)q0 * qstride + (lane & 15);   // this lane's element of every chunk
    float acc[QT][16];
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;
    float4 xa[4], xb[4];
    float qa[QT], qb[QT];
    auto load = [&](float4 (&x)[4], float (&qv)[QT], int c) {
#pragma unroll
        for (int t = 0; t < 4; ++t) x[t] = tp[(size_t)(4 * c + t) * MDB_TILE];
#pragma unroll
        for (int i = 0; i < QT; ++i) qv[i] = ql[(size_t)i * qstride + 16 * c];
    };
    auto accumulate = [&](const float4 (&x)[4], const float (&qv)[QT]) {
        const float xv[16] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w,
                              x[2].x, x[2].y, x[2].z, x[2].w, x[3].x, x[3].y, x[3].z, x[3].w};
#pragma unroll
        for (int i = 0; i < QT; ++i) t16_accumulate<METRIC>(acc[i], qv[i], xv);
    };
    load(xa, qa, 0);
    int c = 0;
#pragma unroll 1
    for (; c + 2 <= n16; c += 2) {
        load(xb, qb, c + 1);
        accumulate(xa, qa);
        if (c + 2 < n16) load(xa, qa, c + 2);
        accumulate(xb, qb);
    }
    if (c < n16) accumulate(xa, qa);
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        const float raw = __fadd_rn(0.0f, reduce_ordered<16>(acc[i]));   // exact_sums: ret = 0 + (ordered sum of the 16 lanes)
        table[(size_t)(q0 + i) * nu_pad + v] = v < nu ? f32_orderable(finish_distance<METRIC>(raw)) : SLOT_EMPTY;
    }
}

// Batches of >= 32 queries, d = 16 * N16 <= 128: the roles swapped — LANE = QUERY (64 queries per wave, a query's d floats resident in
// registers), the POINT's 16-float chunk is the one register that reaches the arithmetic through the DPP operand (lane l of every 16-lane
// row loads element l % 16: a 64-byte load).  Every point is then read ONCE per 64 queries instead of once per QT (the thread = point
// kernel above re-reads the 16 MB of upper vectors b / QT times and ran at the L2's bandwidth, 38 us at batch 64); what is left is the
// arithmetic itself, 3 VALU per element and query.  A wave takes PPW consecutive points; four results per lane are stored together.
#define MDB_T64_TERM(J)                                                                                                       \
    if (METRIC != MDB_METRIC_DOT) {                                                                                           \
        float df;                                                                                                             \
        asm("v_sub_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "=v"(df) : "v"(xv), "v"(qr[16 * C + J])); \
        ac[J] = __fadd_rn(ac[J], __fmul_rn(df, df));                                                                          \
    } else {                                                                                                                  \
        float pr;                                                                                                             \
        asm("v_mul_f32_dpp %0, %1, %2 row_newbcast:" #J " row_mask:0xf bank_mask:0xf" : "=v"(pr) : "v"(xv), "v"(qr[16 * C + J])); \
        ac[J] = __fadd_rn(ac[J], pr);                                                                                         \
    }
template <int METRIC, int N16, int C>
__device__ __forceinline__ void t64_chunk(float (&ac)[16], const float xv, const float (&qr)[16 * N16]) {
    MDB_T64_TERM(0) MDB_T64_TERM(1) MDB_T64_TERM(2) MDB_T64_TERM(3) MDB_T64_TERM(4) MDB_T64_TERM(5) MDB_T64_TERM(6) MDB_T64_TERM(7)
    MDB_T64_TERM(8) MDB_T64_TERM(9) MDB_T64_TERM(10) MDB_T64_TERM(11) MDB_T64_TERM(12) MDB_T64_TERM(13) MDB_T64_TERM(14) MDB_T64_TERM(15)
}
#undef MDB_T64_TERM
template <int METRIC, int N16, int C>
struct T64Point {
    static __device__ __forceinline__ void run(float (&ac)[16], const float (&xc)[N16], const float (&qr)[16 * N16]) {
        t64_chunk<METRIC, N16, C>(ac, xc[C], qr);
        T64Point<METRIC, N16, C + 1>::run(ac, xc, qr);
    }
};
template <int METRIC, int N16>
struct T64Point<METRIC, N16, N16> {
    static __device__ __forceinline__ void run(float (&)[16], const float (&)[N16], const float (&)[16 * N16]) {}
};

// (T64_PPW points per wave: mdb_hnsw_route.h)
// (a block of 256 threads; bx = its slice of the points, by = its group of 64 queries)
template <int METRIC, int N16>
__device__ __forceinline__ void table64_block(const float* __restrict__ rows, uint32_t nu, const float* __restrict__ q, int qstride, uint32_t b,
                                              uint32_t* __restrict__ table, uint32_t nu_pad, const uint32_t bx, const uint32_t by) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t p0 = (bx * 4 + wave) * T64_PPW;
    if (p0 >= nu) return;
    const uint32_t qi = by * 64 + lane;
    const bool qok = qi < b;
    const float4* q4 = (const float4*)(q + (size_t)(qok ? qi : b - 1) * qstride);   // rows are 16-byte aligned (stage_queries)
    float qr[16 * N16];
#pragma unroll
    for (int t = 0; t < 4 * N16; ++t) {
        const float4 v = q4[t];
        qr[4 * t + 0] = v.x; qr[4 * t + 1] = v.y; qr[4 * t + 2] = v.z; qr[4 * t + 3] = v.w;
    }
    const float* xp = rows + (size_t)p0 * (16 * N16) + (lane & 15);
    float xa[N16], xb[N16];
#pragma unroll
    for (int c = 0; c < N16; ++c) xa[c] = xp[16 * c];
    uint32_t* const trow = table + (size_t)qi * nu_pad + p0;
    uint32_t img[4];
#pragma unroll 1
    for (uint32_t i = 0; i < T64_PPW; i += 2) {
        // two points per trip: the other buffer's loads are in flight while one is accumulated (points past nu: the last valid row again)
        {
            const uint32_t pn = p0 + i + 1 < nu ? i + 1 : i;
#pragma unroll
            for (int c = 0; c < N16; ++c) xb[c] = xp[(size_t)pn * (16 * N16) + 16 * c];
            float ac[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) ac[j] = 0.0f;
            T64Point<METRIC, N16, 0>::run(ac, xa, qr);
            img[i & 3] = f32_orderable(finish_distance<METRIC>(__fadd_rn(0.0f, reduce_ordered<16>(ac))));
        }
        {
            const uint32_t pn = p0 + i + 2 < nu ? i + 2 : i;
#pragma unroll
            for (int c = 0; c < N16; ++c) xa[c] = xp[(size_t)pn * (16 * N16) + 16 * c];
            float ac[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) ac[j] = 0.0f;
            T64Point<METRIC, N16, 0>::run(ac, xb, qr);
            img[(i + 1) & 3] = f32_orderable(finish_distance<METRIC>(__fadd_rn(0.0f, reduce_ordered<16>(ac))));
        }
        if ((i & 3) == 2 && qok) {   // p0 and nu_pad are multiples of 16 / 64: 16-byte aligned (slots past nu are never read)
            uint4 o; o.x = img[0]; o.y = img[1]; o.z = img[2]; o.w = img[3];
            *(uint4*)(trow + (i - 2)) = o;
        }
    }
}

template <int METRIC, int N16>
__global__ __launch_bounds__(256, 2) void hnsw_upper_table64_kernel(const float* __restrict__ rows, uint32_t nu, const float* __restrict__ q,
                                                                 int qstride, uint32_t b, uint32_t* __restrict__ table, uint32_t nu_pad,
                                                                 unsigned long long* zero16) {
    if (zero16 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 16) zero16[threadIdx.x] = 0ull;
    table64_block<METRIC, N16>(rows, nu, q, qstride, b, table, nu_pad, blockIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------------------------------ traversal
struct HnswUpArgs {
    const uint32_t* rows;     // [(layer - row_layer0) * nu + c] * su: adjacency rows of layers row_layer0 .. in this launch's compact numbering
    const uint32_t* table;    // [b][nu_pad] distance images (the top phase of the split path computes its row itself)
    uint32_t nu, nu_pad, su, small_layer, entry_c;
    int row_layer0;
    int layer_hi, layer_lo;   // this launch traverses layers layer_hi .. layer_lo (>= 1)
    int ef;
    uint32_t vis_words;
    // state handed over by the launch that traversed the layers above (nullptr: start at entry_c with an empty visited set)
    const uint32_t* in_ep;    // [b] entry point, this launch's numbering
    const uint32_t* in_ovf;   // [b]
    const uint32_t* in_vis;   // [b][vis_words]
    const uint32_t* in_cnt;   // [b][4] evaluations, expansions, NaN seen
    // state handed on
    const uint32_t* ep_map;   // index -> what out_ep holds: the point id (layer 0 follows) or the next launch's compact index
    const uint32_t* vis_map;  // nullptr: out_vis = the bitmap as is; else bit c of it -> bit vis_map[c] of a bitmap of out_words words
    uint32_t out_words;
    uint32_t* out_ep;
    uint32_t* out_ovf;
    uint32_t* out_vis;
    uint32_t* out_cnt;        // the counters go here ([b][4]), not to the context: the layer-0 block adds them with its own when the query
                              // ends inside the beam — a beam that overflows further down re-runs the WHOLE query, and nothing of it may
                              // have been counted (nullptr: a caller with nothing below it; counted here unless overflowed)
    uint32_t* flags;
    unsigned long long* counters;
    // top phase of the split path: the block evaluates its query against this compact set itself (tiles, d = 16 n16)
    const float4* self_tiles;
    uint32_t self_ntiles;
    int n16;
    const float* q;
    int qstride;
    int dbg_on;               // MDB_PIPE_DBG builds: this launch adds its cycle sums to counters[4..15] (MDB_HNSW_DBG bit 0: bottom launch, bit 1: top;
                              // bit 2 / 3: the same two launches in the frontier form, CL_DBG_*)
    // frontier form (mdb_hnsw_closure.hip.h): fb[q] (CL_FB_*) = what is left to do for a query the form flagged; fb_role: what this
    // launch does with the word (CL_ROLE_*; nullptr / 0: no closure launch in this call)
    uint32_t* fb;
    int fb_role;
    const uint32_t* top_map;  // a closure launch over every upper layer: the TOP set (layers >= 2) in this launch's numbering, for its own theta
    uint32_t top_n;
    int cl_tlds;              // closure launch behind the table: the query's row is copied into LDS
};
// (the CL_ROLE_* roles of a launch in the fallback protocol, HnswUpArgs::fb_role: mdb_hnsw_route.h)
// values of fb[q]; every call writes the word of each of its queries before it reads it (the scratch is reused from call to call)
#define CL_FB_CLEAN 0u
#define CL_FB_RERUN 1u           // the follow-up launch re-runs the query: from the top, or layer 1 alone behind CL_ROLE_TOP_LOCAL
#define CL_FB_COUNT 2u           // flagged in the top launch and resolved there: not yet counted


#define UP_LDS_STAGE 0                 // 512 keys (compaction staging)
#define UP_LDS_FLAG 4096               // 512 words
#define UP_LDS_FR 6144                 // two frontier lists of 64 (closure of tiny layers)
// UP_LDS_VIS 6656 (mdb_hnsw_route.h): the visited set, then what the launch's form puts behind it

// One wave per query.  The state is the Beam<NB> of mdb_hnsw_dev.hip.h and the step a sequence of its operations (over-full
// unsorted register beam B, acceptance and stop test by counting, runner-up + its row fetched ahead) — the step hnsw_beam_kernel's
// wave 0 runs, written out there; what is gone is everything between its P2 and P4.
// TLDS: the query's table row (nu_pad words, 129 KB at 1 M points / 32 k upper points) is copied into LDS by the whole block first —
// a lookup is then an LDS read (~100 cycles) instead of a first-touch miss of a line the table kernel wrote from another XCD
// (the L2s are not coherent: the row comes back from the Infinity Cache / HBM, ~1 k cycles, 40 % of the lookups).  Waves 1-3 only
// help with that copy.
// wave 0 of the block (64 lanes): layers a.layer_hi .. a.layer_lo on the table row `tq`, visited set `vis` (LDS, initialised by the
// caller), then the hand-over.  `vis_out`: LDS scratch of a.out_words words when a.vis_map is set.
template <int NB>
__device__ __forceinline__ void upper_traverse_wave0(const HnswUpArgs& a, const int qi_in, const int lane, char* lds, const uint32_t* tq,
                                                     uint32_t* vis, uint32_t* vis_out) {
    // Round 6 (found with `opt -passes=print<uniformity>` while the sorted-position kernels were built): the block index reaches
    // this function through phis behind the block's per-thread set-up loops, and the per-lane branches that were inside the step
    // (`lane < su` around the row load, `valid` around the LDS atomic and the table lookup, `lane == 0` around the entry point's
    // mark) joined in blocks that also carried the loop's scalars — so `stop`, `overflow`, `ru_valid`, the counters ... were all
    // per-lane values to the compiler, and the loop's control flow was exec-mask code with its state in VGPRs and lane masks.
    // The block index is named uniform again and those accesses are branch-free (idle lanes: a clamped address / a word of their own).
    const int qi = __builtin_amdgcn_readfirstlane(qi_in);
    uint32_t* const dummy = (uint32_t*)(lds + UP_LDS_FLAG);   // 64 words an OR of 0 leaves alone
    uint64_t* const C = (uint64_t*)(lds + UP_LDS_STAGE);
    uint32_t* const stage_flag = (uint32_t*)(lds + UP_LDS_FLAG);
    uint32_t* const fr = (uint32_t*)(lds + UP_LDS_FR);
    const int ef = a.ef;
    const uint32_t su = a.su;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    Beam<NB> B;   // the register beam (mdb_hnsw_dev.hip.h): seeded at every layer's entry point
    uint32_t rowv = 0xFFFFFFFFu, rowr = 0xFFFFFFFFu;
    BeamCand ru = {SLOT_EMPTY, 0, false};   // the runner-up: the best candidate already in B
    bool stop = false, overflow = a.in_ovf ? a.in_ovf[qi] != 0u : false, nan_lane = false;
    int ru_closer = 0;
    int nexp = 0;   // expanded slots of B: no stop count is taken while nexp < ef (see beam_pop)
    uint32_t evals = a.in_cnt ? a.in_cnt[4 * qi + 0] : 0u, expanded = a.in_cnt ? a.in_cnt[4 * qi + 1] : 0u;
    if (a.in_cnt && a.in_cnt[4 * qi + 2]) nan_lane = true;
    uint32_t ep = a.in_ep ? a.in_ep[qi] : a.entry_c;
#ifdef MDB_PIPE_DBG
    unsigned long long dbg_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif

    for (int layer = a.layer_hi; layer >= a.layer_lo && !overflow; --layer) {
        const uint32_t* const lrows = a.rows + (size_t)(layer - a.row_layer0) * a.nu * su;
        // (raw: lanes >= su repeat the row's last word and are masked where the row is consumed)
        const uint32_t lane_c = min((uint32_t)lane, su - 1u);
        auto load_row = [&](uint32_t node) -> uint32_t { return lrows[(size_t)node * su + lane_c]; };
        if ((uint32_t)layer >= a.small_layer && ef >= 64) {
            // ---- a layer with no more points than ef (<= 64, edges only among them): its result is the closure of the entry
            // point whatever the pop order (see hnsw_closure_kernel) — whole frontiers per round, 64 / sp points per pass
            uint32_t sp = 1;
            while (sp < su) sp <<= 1;
            const uint32_t per = 64u / sp;
            uint32_t* cur = fr;
            uint32_t* nxt = fr + 64;
            if (lane == 0) { atomicOr(&vis[ep >> 5], 1u << (ep & 31)); cur[0] = ep; }
            uint32_t ncur = 1;
            uint64_t best = MDB_KEY_MAX;
            while (ncur > 0) {
                uint32_t nnext = 0;
                for (uint32_t base = 0; base < ncur; base += per) {
                    const uint32_t pi = base + lane / sp, slot = lane % sp;
                    const bool act = pi < ncur;
                    const uint32_t f = act ? cur[pi] : 0u;
                    const uint32_t nbr = (act && slot < su) ? lrows[(size_t)f * su + slot] : 0xFFFFFFFFu;
                    if (act && slot == 0) {
                        const uint32_t od = tq[f];
                        const float fd = f32_from_orderable(od);
                        if (fd != fd) nan_lane = true;
                        const uint64_t key = ((uint64_t)od << 32) | f;
                        best = key < best ? key : best;
                    }
                    expanded += (uint32_t)__popcll(__ballot(act && slot == 0 && nbr != 0xFFFFFFFFu));  // rows are packed
                    bool isnew = false;
                    if (nbr != 0xFFFFFFFFu) {
                        const uint32_t bit = 1u << (nbr & 31);
                        isnew = !(atomicOr(&vis[nbr >> 5], bit) & bit);
                    }
                    const unsigned long long bal = __ballot(isnew);
                    if (isnew) nxt[nnext + __popcll(bal & lt_mask)] = nbr;
                    nnext += (uint32_t)__popcll(bal);
                }
                evals += ncur;
                ncur = nnext;
                uint32_t* t = cur; cur = nxt; nxt = t;
            }
            // smallest (distance, id) of the layer's points
            const uint32_t mo = wave_min_u32((uint32_t)(best >> 32));
            ep = wave_min_u32((uint32_t)(best >> 32) == mo ? (uint32_t)best : 0xFFFFFFFFu);
            continue;
        }
        // ---- entry point: mark visited, look its distance up, seed B (index.rs:219-231) and pop it at once
        {
            atomicOr(lane == 0 ? &vis[ep >> 5] : &dummy[lane], lane == 0 ? 1u << (ep & 31) : 0u);
            rowv = load_row(ep);
            const uint32_t od0 = tq[ep];
            const float f0 = f32_from_orderable(od0);
            if (f0 != f0) nan_lane = true;
            B = beam_seed<NB>(ep, od0, lane);
            nexp = 1;
            stop = false;
            ru.have = false;
            evals += 1;
        }
        while (!stop && !overflow) {
            // ---- visited test-and-set and table lookups of the popped node's row: issued together ...
            PIPE_T(t0);
            const uint32_t nbr = (uint32_t)lane < su ? rowv : 0xFFFFFFFFu;
            const bool valid = nbr != 0xFFFFFFFFu;
            const uint32_t bit = 1u << (nbr & 31);
            const uint32_t old = atomicOr(valid ? &vis[nbr >> 5] : &dummy[lane], valid ? bit : 0u);
            uint32_t od = tq[valid ? nbr : 0u];
            // ---- ... and in flight while the wave finds the best candidate already in B (the next pop unless a neighbour accepted
            // below beats it), requests its row and takes its stop count
            PIPE_T2L(s0);   // (debug 2: the LDS round trip of the visited set / table is retired here, not behind the selection)
            ru = beam_select(B);
            PIPE_T2L(s1);
            if (ru.have) {
                rowr = load_row(ru.id);
                ru_closer = nexp >= ef ? beam_count_closer(B, ru.o) : 0;
            }
            PIPE_T(t1);
            PIPE_ACC2(6, s0 - t0); PIPE_ACC2(7, s1 - s0);
            const bool have = valid && !(old & bit);
            const unsigned long long hm = __ballot(have);
            const uint32_t nnew = (uint32_t)__popcll(hm);
            expanded += __ballot(valid) != 0 ? 1u : 0u;
            evals += nnew;
            od = have ? od : SLOT_EMPTY;
            if (have) {
                const float fd = f32_from_orderable(od);
                if (fd != fd) nan_lane = true;   // the reference panics (NotNan::new(..).unwrap())
            }
            const uint32_t id = nbr;
            // ---- accept + push, then choose the next node
            BeamCand best = {SLOT_EMPTY, 0, false};   // best accepted neighbour in pop order
            PIPE_T(t2);
            PIPE_ACC(0, t1 - t0); PIPE_ACC(1, t2 - t1); PIPE_ACC(5, 1); PIPE_CNT(6, nnew);
            if (nnew) {
                PIPE_CNT(7, __popcll(__ballot(have && od < B.fbound)));   // the prefilter's survivors
                unsigned long long accepted;
                B = beam_accept(B, have, od, (int)nnew, ef, accepted);
                const int na = __popcll(accepted);
                PIPE_T(t3);
                PIPE_ACC(2, t3 - t2); PIPE_CNT(8, na); PIPE_CNT(9, na == 1 ? 1 : 0);
                if (na) {
                    if (B.n + na > (64 * NB)) {
                        bool by_bound;
                        B = beam_compact(B, ef, na, C, stage_flag, lane, by_bound);
                        PIPE_CNT(by_bound ? 10 : 11, 1);   // slot 10: by the bound, slot 11: by the exact select
                        nexp = 0;
#pragma unroll
                        for (int r = 0; r < NB; ++r) nexp += __popcll(__ballot(B.bd[r] != SLOT_EMPTY && B.cdv[r] == SLOT_EMPTY));
                        if (B.n + na > (64 * NB)) { overflow = true; break; }
                        ru = beam_select(B);  // may have been dropped
                        if (ru.have) rowr = load_row(ru.id);
                        ru_closer = nexp >= ef ? beam_count_closer(B, ru.o) : 0;
                    }
                    if (nexp >= ef) ru_closer += __popcll(accepted & __ballot(od < ru.o));   // this step's pushes
                    B = beam_push(B, accepted, od, id, lane, best);
                }
                PIPE_T(t4);
                PIPE_ACC(3, t4 - t3);
            }
            PIPE_T(t5);
            PIPE_T2(p0);   // (debug 2: every outstanding load — the runner-up's row — retired here)
            PIPE_ACC2(8, p0 - t5);
            // ---- candidates.pop()
            BeamPop pop;
            B = beam_pop(B, ru, nexp >= ef ? ru_closer : 0, best, nexp >= ef, ef, pop);
            if (pop == BEAM_POP_STOP) {
                stop = true;
            } else {
                rowv = pop == BEAM_POP_RUNNER_UP ? rowr : load_row(best.id);
                ++nexp;
            }
            PIPE_T(t6);
            PIPE_ACC(4, t6 - t5);
            PIPE_ACC2(9, t6 - p0);
        }
        if (overflow) break;
        // ---- a layer hands its nearest point down
        ep = beam_nearest_id(B);
    }
    const bool nan_seen = __ballot(nan_lane) != 0;
    // the hand-over fields are re-read from the kernarg segment (HnswUpArgs is the first kernel argument of both kernels) behind an opaque
    // barrier: kept in `a` they stay live — as spilled scalars, reloaded by v_readlane — through the whole traversal loop
    const HnswUpArgs* ap = (const HnswUpArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ap));
    const HnswUpArgs& e = *ap;
    if (e.vis_map) {
        // the next launch numbers the points differently (a superset): bit c -> bit vis_map[c]
        for (uint32_t i = lane; i < e.out_words; i += 64) vis_out[i] = 0;
        for (uint32_t w = lane; w < e.vis_words; w += 64) {
            uint32_t bits = vis[w];
            while (bits) {
                const uint32_t c = 32u * w + (uint32_t)__ffs((int)bits) - 1u;
                bits &= bits - 1u;
                const uint32_t t = e.vis_map[c];
                atomicOr(&vis_out[t >> 5], 1u << (t & 31));
            }
        }
        for (uint32_t i = lane; i < e.out_words; i += 64) e.out_vis[(size_t)qi * e.out_words + i] = vis_out[i];
    } else {
        for (uint32_t i = lane; i < e.vis_words; i += 64) e.out_vis[(size_t)qi * e.vis_words + i] = vis[i];
    }
#ifdef MDB_PIPE_DBG
    if (lane == 0)
        for (int i = 0; i < 12; ++i)
            if (dbg_acc[i]) atomicAdd(&e.counters[4 + i], dbg_acc[i]);
#endif
    if (lane == 0) {
        e.out_ep[qi] = overflow ? 0u : e.ep_map[ep];
        e.out_ovf[qi] = overflow ? 1u : 0u;
        if (e.out_cnt) {
            e.out_cnt[4 * qi + 0] = evals; e.out_cnt[4 * qi + 1] = expanded; e.out_cnt[4 * qi + 2] = nan_seen ? 1u : 0u;
        } else if (!overflow) {
            atomicAdd(&e.counters[0], (unsigned long long)evals);
            atomicAdd(&e.counters[1], (unsigned long long)expanded);
            if (nan_seen) atomicOr(e.flags, MDB_FLAG_NAN);
        }
    }
}

// TLDS: the query's table row (nu_pad words, 129 KB at 1 M points / 32 k upper points) is copied into LDS by the whole block first —
// a lookup is then an LDS read (~100 cycles) instead of a first-touch miss of a line the table kernel wrote from another XCD
// (the L2s are not coherent: the row comes back from the Infinity Cache / HBM, ~1 k cycles, 40 % of the lookups).  Waves 1-3 only
// help with that copy.
template <bool TLDS, int NB>
__global__ __launch_bounds__(UP_BLOCK) void hnsw_upper_kernel(HnswUpArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint32_t* const vis = (uint32_t*)(lds + UP_LDS_VIS);
    const int qi = blockIdx.x, lane = threadIdx.x & 63;
    if (a.fb && !a.fb[qi]) return;   // the fallback launch behind the frontier form: only the flagged queries run
    const uint32_t* const tg = a.table + (size_t)qi * a.nu_pad;
    uint32_t* const tl = vis + a.vis_words;   // TLDS: the row's copy (vis_words is a multiple of 4: 16-byte aligned; nu_pad is a multiple of 64)
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += UP_BLOCK) vis[i] = a.in_vis ? a.in_vis[(size_t)qi * a.vis_words + i] : 0u;
    if (TLDS) {
        const uint4* src = (const uint4*)tg;
        uint4* dst = (uint4*)tl;
        for (uint32_t i = threadIdx.x; i < a.nu_pad / 4; i += UP_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    upper_traverse_wave0<NB>(a, qi, lane, lds, TLDS ? tl : tg, vis, tl + (TLDS ? a.nu_pad : 0));
}

#include "mdb_hnsw_rank.hip.h"
#include "mdb_hnsw_closure.hip.h"

// a top block of the split path's first launch in the frontier form (a.fb_role CL_ROLE_TOP / CL_ROLE_TOP_LOCAL): it evaluates its query against the TOP
// set itself, as the sequential forms do, and traverses the layers >= 2 with all four waves.  Returns closure_traverse's flag; the row
// is still at `row` when it does.
template <int METRIC, int N16>
__device__ __forceinline__ bool closure_top_block(const HnswUpArgs& a, char* lds, const uint32_t*& row) {
    const ClLds L = cl_carve((uint32_t*)lds, a.vis_words, a.out_words);
    const int qi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long t_row = CL_DBG_NOW();
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += 256) L.vis[i] = 0u;
    // the block's own table row: one wave per tile of 64 points, thread = point (exact association, DPP-broadcast query chunks)
    const float* const ql = a.q + (size_t)qi * a.qstride + (lane & 15);
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;             // of the row's canonical images: the select's key range, taken where the row is made
    for (uint32_t tile = wave; tile < a.self_ntiles; tile += 4) {
        const float4* tp = a.self_tiles + (size_t)tile * (4 * N16) * MDB_TILE + lane;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < N16; ++c) {
            float4 x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = tp[(size_t)(4 * c + t) * MDB_TILE];
            const float xv[16] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w,
                                  x[2].x, x[2].y, x[2].z, x[2].w, x[3].x, x[3].y, x[3].z, x[3].w};
            t16_accumulate<METRIC>(acc, ql[16 * c], xv);
        }
        const uint32_t v = tile * MDB_TILE + lane;
        const uint32_t img = v < a.nu ? f32_orderable(finish_distance<METRIC>(__fadd_rn(0.0f, reduce_ordered<16>(acc)))) : SLOT_EMPTY;
        L.row[v] = img;
        if (v < a.nu) { mn = min(mn, rk_canon(img)); mx = max(mx, rk_canon(img)); }
    }
    __syncthreads();
    row = L.row;
    return closure_traverse<256>(a, qi, L, L.row, true, mn, mx, CL_DBG_NOW() - t_row);
}


// The split path (batches of >= 32 queries, d = 16 n16 <= 128): ONE launch whose first b blocks traverse the layers >= 2 — ~1 k points:
// each block evaluates its query against them itself (the thread = point arithmetic of hnsw_upper_table16_kernel, the row goes
// straight into LDS) — while the remaining blocks are the lane = query table pass over ALL upper points (hnsw_upper_table64_kernel's
// body) that layer 1 needs: the 35 us of that pass run on the 192 CUs the 64 traversals leave idle instead of in front of them.
// The layer-1 launch (hnsw_upper_kernel) picks the state up: entry point and visited set in ITS numbering, counters not yet counted.
template <int METRIC, int N16, int NB>
__global__ __launch_bounds__(256, 2) void hnsw_upper_top_kernel(HnswUpArgs a, uint32_t nq, const float* __restrict__ rows_nat, uint32_t nu_all,
                                                                uint32_t* __restrict__ table_all, uint32_t nu_all_pad, uint32_t tgx,
                                                                unsigned long long* zero16) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if (blockIdx.x >= nq) {
        const uint32_t t = blockIdx.x - nq;
        table64_block<METRIC, N16>(rows_nat, nu_all, a.q, a.qstride, nq, table_all, nu_all_pad, t % tgx, t / tgx);
        return;
    }
    if (zero16 && blockIdx.x == 0 && threadIdx.x < 16) zero16[threadIdx.x] = 0ull;
    uint32_t* const vis = (uint32_t*)(lds + UP_LDS_VIS);
    const int qi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* const tl = vis + a.vis_words;
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += UP_BLOCK) vis[i] = 0u;
    // the block's own table row: one wave per tile of 64 points, thread = point (exact association, DPP-broadcast query chunks)
    const float* const ql = a.q + (size_t)qi * a.qstride + (lane & 15);
    for (uint32_t tile = wave; tile < a.self_ntiles; tile += UP_BLOCK / 64) {
        const float4* tp = a.self_tiles + (size_t)tile * (4 * N16) * MDB_TILE + lane;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < N16; ++c) {
            float4 x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = tp[(size_t)(4 * c + t) * MDB_TILE];
            const float xv[16] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w,
                                  x[2].x, x[2].y, x[2].z, x[2].w, x[3].x, x[3].y, x[3].z, x[3].w};
            t16_accumulate<METRIC>(acc, ql[16 * c], xv);
        }
        const uint32_t v = tile * MDB_TILE + lane;
        tl[v] = v < a.nu ? f32_orderable(finish_distance<METRIC>(__fadd_rn(0.0f, reduce_ordered<16>(acc)))) : SLOT_EMPTY;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    upper_traverse_wave0<NB>(a, qi, lane, lds, tl, vis, tl + a.nu_pad);
}

// the same launch with the top blocks on sorted positions (mdb_hnsw_rank.hip.h): own table row -> LDS, sorted there, traversed by ranks
template <int METRIC, int N16, int NW>
__global__ __launch_bounds__(256, 2) void hnsw_upper_top_rank_kernel(HnswUpArgs a, uint32_t nq, const float* __restrict__ rows_nat, uint32_t nu_all,
                                                                     uint32_t* __restrict__ table_all, uint32_t nu_all_pad, uint32_t tgx,
                                                                     unsigned long long* zero16) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if (blockIdx.x >= nq) {
        const uint32_t t = blockIdx.x - nq;
        table64_block<METRIC, N16>(rows_nat, nu_all, a.q, a.qstride, nq, table_all, nu_all_pad, t % tgx, t / tgx);
        return;
    }
    if (zero16 && blockIdx.x == 0 && threadIdx.x < 16) zero16[threadIdx.x] = 0ull;
    uint32_t* const vis = (uint32_t*)(lds + UP_LDS_VIS);
    const int qi = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* const tl = vis + a.vis_words;
    uint16_t* const bufA = (uint16_t*)(tl + a.nu_pad);
    uint16_t* const bufB = bufA + a.nu_pad;
    uint32_t* const hist = (uint32_t*)(bufB + a.nu_pad);
    uint32_t* const red = hist + RK_HIST_WORDS(256);
    uint32_t* const vis_out = red + 64;
    const bool closure = a.fb_role == CL_ROLE_TOP || a.fb_role == CL_ROLE_TOP_LOCAL;
    if (closure) {   // the frontier form (mdb_hnsw_closure.hip.h) is a mode of this launch
        const uint32_t* row;
        const bool flagged = closure_top_block<METRIC, N16>(a, lds, row);
        if (NW != 1 || a.fb_role != CL_ROLE_TOP_LOCAL || !flagged) return;
        // flagged (an exact tie at the stop test, a NaN): nothing was published and the closure's LDS is dead.  The block re-runs the
        // query on sorted positions right here, as below; all that moves is the row (the layouts overlap: through registers,
        // nu_pad <= 2048 = 8 words per thread)
        uint32_t keep[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t i = threadIdx.x + 256u * j;
            keep[j] = i < a.nu_pad ? row[i] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t i = threadIdx.x + 256u * j;
            if (i < a.nu_pad) tl[i] = keep[j];
        }
        if (threadIdx.x == 0) a.fb[qi] = CL_FB_COUNT;
    }
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += UP_BLOCK) vis[i] = 0u;
    // the block's own table row: one wave per tile of 64 points, thread = point (exact association, DPP-broadcast query chunks)
    const float* const ql = a.q + (size_t)qi * a.qstride + (lane & 15);
    // (behind the frontier form the row is already there: no tile is left to do)
    for (uint32_t tile = closure ? a.self_ntiles : wave; tile < a.self_ntiles; tile += UP_BLOCK / 64) {
        const float4* tp = a.self_tiles + (size_t)tile * (4 * N16) * MDB_TILE + lane;
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < N16; ++c) {
            float4 x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = tp[(size_t)(4 * c + t) * MDB_TILE];
            const float xv[16] = {x[0].x, x[0].y, x[0].z, x[0].w, x[1].x, x[1].y, x[1].z, x[1].w,
                                  x[2].x, x[2].y, x[2].z, x[2].w, x[3].x, x[3].y, x[3].z, x[3].w};
            t16_accumulate<METRIC>(acc, ql[16 * c], xv);
        }
        const uint32_t v = tile * MDB_TILE + lane;
        tl[v] = v < a.nu ? f32_orderable(finish_distance<METRIC>(__fadd_rn(0.0f, reduce_ordered<16>(acc)))) : SLOT_EMPTY;
    }
    __syncthreads();
    uint16_t *P, *R;
    uint32_t nan_start;
    const unsigned long long ts0 = __builtin_readcyclecounter();
    rank_tables<256>(tl, a.nu, bufA, bufB, hist, red, P, R, nan_start);
    if (threadIdx.x >= 64) return;
    if constexpr (NW == 1) upper_traverse_rank1(a, qi, lane, lds, R, P, nan_start, vis, vis_out, __builtin_readcyclecounter() - ts0);
    else upper_traverse_rank<NW>(a, qi, lane, lds, R, P, nan_start, vis, vis_out, __builtin_readcyclecounter() - ts0);
}

// ------------------------------------------------------------------------------------------ executor
// The arguments of a traversal launch of the route, by its role.  HR_TOP: the TOP set (layers >= 2) on a row the block evaluates itself,
// handing entry point and visited set on in the layer-1 numbering, overflow flag and counters not yet counted (st: the hand-over
// state, fb behind it).  HR_LAYER1 / HR_FALLBACK: layers l.layer_hi .. 1 on the table rows, the last launch before layer 0 (out_ep
// holds point ids, the bitmap as is).
static HnswUpArgs upper_args(mdb_ctx* ctx, const HnswUpper& up, const DistPlan& p, const float* d_q, int qstride, const HnswRoute& r,
                             const HnswLaunch& l, const uint32_t* d_table, uint32_t* st, const HnswUpperOut& out) {
    const bool top = l.role == HR_TOP;
    uint32_t *const st_ep = st, *const st_ovf = st + r.st_ovf, *const st_cnt = st + r.st_cnt, *const st_vis = st + r.st_vis;
    HnswUpArgs a{};
    a.rows = top ? up.rows2.p : up.rows.p; a.table = top ? nullptr : d_table; a.row_layer0 = top ? 2 : 1;
    a.nu = top ? up.nu2 : up.nu; a.nu_pad = top ? r.nu2_pad : r.nu_pad; a.su = up.su; a.small_layer = up.small_layer;
    a.entry_c = top ? up.entry_c2 : up.entry_c;
    a.layer_hi = l.layer_hi; a.layer_lo = top ? 2 : 1;
    a.ef = (int)r.ef;
    a.vis_words = top ? r.up_words2 : r.up_words;
    if (l.handover) { a.in_ep = st_ep; a.in_ovf = st_ovf; a.in_vis = st_vis; a.in_cnt = st_cnt; }
    a.ep_map = top ? up.map21.p : up.ids.p; a.vis_map = top ? up.map21.p : nullptr; a.out_words = r.up_words;
    a.out_ep = top ? st_ep : out.ep; a.out_ovf = top ? st_ovf : out.ovf; a.out_vis = top ? st_vis : out.vis; a.out_cnt = top ? st_cnt : out.cnt;
    a.flags = ctx->d_flags; a.counters = ctx->d_counters;
    if (top) {
        a.self_tiles = (const float4*)up.tiles2.data.p; a.self_ntiles = (uint32_t)up.tiles2.ntiles; a.n16 = p.n16; a.q = d_q; a.qstride = qstride;
    }
    // MDB_PIPE_DBG builds (MDB_HNSW_DBG bit 0: the sequential bottom launch, bit 1: the sequential top launch)
    if (l.fb_role == CL_ROLE_NONE || l.fb_role == CL_ROLE_FALLBACK) a.dbg_on = (int)((ctx->opt.hnsw_dbg >> (top ? 1 : 0)) & 1);
    else a.dbg_on = (int)((ctx->opt.hnsw_dbg >> (top ? 3 : 2)) & 1);
    if (l.fb_role != CL_ROLE_NONE) { a.fb = st + r.st_fb; a.fb_role = l.fb_role; }
    if (l.fb_role == CL_ROLE_BOTTOM || l.fb_role == CL_ROLE_SINGLE) {   // the frontier form's own theta over the TOP set
        if (up.nu2 > 0 && up.map21.p) { a.top_map = up.map21.p; a.top_n = up.nu2; }
        a.cl_tlds = l.cl_tlds ? 1 : 0;
    }
    return a;
}

mdb_status hnsw_upper_run(mdb_ctx* ctx, const HnswUpper& up, const DistPlan& p, const float* d_q, int qstride, size_t b,
                          const HnswRoute& r, uint32_t* d_table, uint32_t* d_state, const HnswUpperOut& out, unsigned long long* zero16) {
    const float4* tiles = (const float4*)up.tiles.data.p;
    const uint32_t ntiles = (uint32_t)up.tiles.ntiles, tgx = (up.nu + 4 * T64_PPW - 1) / (4 * T64_PPW);
    for (int i = 0; i < r.n; ++i) {
        const HnswLaunch& l = r.launch[i];
        if (l.role != HR_TABLE && l.role != HR_TOP && l.role != HR_LAYER1 && l.role != HR_FALLBACK) continue;
        const dim3 grid(l.gx, l.gy);
        unsigned long long* const z16 = l.zero16 ? zero16 : nullptr;
        const HnswUpArgs a = l.role == HR_TABLE ? HnswUpArgs{} : upper_args(ctx, up, p, d_q, qstride, r, l, d_table, d_state, out);
        switch (l.kernel) {
        case HK_TABLE64:
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(l.targ[0], [&](auto M) {
                return mdb_pick<1, 2, 3, 4, 5, 6, 7, 8>(l.targ[1], [&](auto N) {
                    return mdb_launch(ctx, hnsw_upper_table64_kernel<M(), N()>, grid, l.block, l.lds, up.rows_nat.p, up.nu, d_q, qstride, (uint32_t)b,
                                      d_table, r.nu_pad, z16);
                });
            }));
            break;
        case HK_TABLE16:
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(l.targ[0], [&](auto M) {
                return mdb_pick<8, 4, 2, 1>(l.targ[1], [&](auto QF) {
                    return mdb_launch(ctx, hnsw_upper_table16_kernel<M(), QF()>, grid, l.block, l.lds, tiles, up.nu, ntiles, p.n16, d_q, qstride,
                                      l.q_first, d_table, r.nu_pad, z16);
                });
            }));
            break;
        case HK_TABLE:
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(l.targ[0], [&](auto M) {
                return mdb_pick<2, 1>(l.targ[1], [&](auto QT) {
                    return mdb_launch(ctx, hnsw_upper_table_kernel<M(), QT()>, grid, l.block, l.lds, tiles, up.nu, p, d_q, qstride, l.q_first, d_table,
                                      r.nu_pad, z16);
                });
            }));
            break;
        case HK_TOP_RANK:
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(l.targ[0], [&](auto M) {
                return mdb_pick<1, 2, 3, 4, 5, 6, 7, 8>(l.targ[1], [&](auto N) {
                    return mdb_pick<1, 4>(l.targ[2], [&](auto NW) {
                        return mdb_launch(ctx, hnsw_upper_top_rank_kernel<M(), N(), NW()>, grid, l.block, l.lds, a, (uint32_t)b, up.rows_nat.p, up.nu,
                                          d_table, r.nu_pad, tgx, z16);
                    });
                });
            }));
            break;
        case HK_TOP:
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(l.targ[0], [&](auto M) {
                return mdb_pick<1, 2, 3, 4, 5, 6, 7, 8>(l.targ[1], [&](auto N) {
                    return mdb_pick<4, 5>(l.targ[2], [&](auto NB) {
                        return mdb_launch(ctx, hnsw_upper_top_kernel<M(), N(), NB()>, grid, l.block, l.lds, a, (uint32_t)b, up.rows_nat.p, up.nu, d_table,
                                          r.nu_pad, tgx, z16);
                    });
                });
            }));
            break;
        case HK_UPPER_RANK:
            MDB_TRY(mdb_pick<1, 4, 16>(l.targ[0], [&](auto NW) { return mdb_launch(ctx, hnsw_upper_rank_kernel<NW()>, grid, l.block, l.lds, a); }));
            break;
        case HK_UPPER:
            MDB_TRY(mdb_pick<4, 5, 8>(l.targ[1], [&](auto NB) {
                return mdb_pick_bool(l.targ[0] != 0, [&](auto TL) { return mdb_launch(ctx, hnsw_upper_kernel<TL(), NB()>, grid, l.block, l.lds, a); });
            }));
            break;
        default:
            return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "hnsw_upper_run: a route with kernel %d among its upper launches", (int)l.kernel);
        }
        MDB_HIP(ctx, hipGetLastError());
    }
    return MDB_OK;
}

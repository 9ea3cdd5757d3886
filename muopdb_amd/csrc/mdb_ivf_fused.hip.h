// mdb_ivf_fused.hip.h — device code of mdb_ivf.hip, part 3: the fused small-batch IVF-PQ step (ivf_prep_kernel, ivf_pq_fused_kernel; the
// matrix-core coarse search of mdb_ivf_coarse.hip.h sits between them).  Included by mdb_ivf.hip only, after mdb_ivf_pq2.hip.h.
#pragma once

// ------------------------------------------------------------------------------------------
// The small-batch step of BASELINE config C3 — BlockBasedIvf::search (index.rs:396-413) over an L2 PQ index, a few thousand
// scanned vectors per query — in TWO launches instead of six (pad, flat scan, merge, quantize, table scan, remap):
//
//   ivf_prep_kernel       every (query, centroid) distance of find_nearest_centroids (:147-163) — 8 queries share each centroid
//                         load, nothing is selected here — and the queries' PQ codes (pq/mod.rs:152-177).
//   ivf_pq_fused_kernel   ONE 1024-thread block per query: the num_probes nearest centroids, the bound table, the scan, the exact
//                         distances of the candidates, the top-k by (distance, point id) (:250-286), doc ids + IdWithScore order
//                         (:298-332).
//
// The old step was latency, not work: its scan built a 128 KB table of every (subspace, code, element) term per query to
// evaluate ~4 000 vectors of which a few dozen can reach the top-k, and every selection went through a streaming selector
// with a block barrier (16 waves) and often a sort per round.  Here
//   * the block keeps ONE word per (subspace, code): a bf16 lower and upper bound of the row's sum (ivf_scan_pq3_kernel's
//     table).  The k-th smallest UPPER bound bounds the k-th exact distance from above; a vector whose LOWER bound exceeds it
//     is out, every other one is a CANDIDATE, evaluated exactly from the codebook rows in L2 with ivf_scan_pq2_kernel's
//     terms and association: identical keys.
//   * "k-th smallest of n" is never computed exactly: block_kth_bound() buckets the order-preserving images of the values
//     (a monotone map: min .. max onto 1024 bins, one LDS histogram, one scan) and returns the upper edge of the bin that
//     holds the k-th — a few barriers whatever n and k.  What passes is a small superset of the k smallest, ranked by
//     COUNTING (every element counts the smaller ones: no sort, one barrier).
//   * a wave fetches four tiles of the flattened list sequence at once (one load latency per 4 096 vectors).
// Thousands of exact ties (candidate lists beyond their capacity) take the streaming selector instead: slower, still exact.
// Requires: one index (no per-query user), L2, m == 4 MW, nbits == 8, k <= 64, probes <= 64 (<= 8 192 centroids when the
// coarse search runs here).
// 16 waves per query (four per SIMD): the heavy phases (bound lookups, table, exact rows) need the memory and LDS parallelism —
// with four waves the lookups alone took 12.5 k cycles instead of 3.4 k.  The price: every instruction of the short serial
// phases (reductions, scans, counting ranks) that all waves execute alike costs 16 cycles of its SIMD, so those phases are
// written for instruction count (LDS atomics instead of per-wave loops over the other waves' partial results).
#define PQF_NW (PQF_BLOCK / MDB_WAVE)
#ifndef PQF_TPW_MAX
#define PQF_TPW_MAX 6
#endif
                       // PQF_TPW_MAX: tiles per wave and chunk (6 with <= 4 code words per vector: a chunk = 96 tiles — C3's 16 probes are 64-75 tiles,
                       // and a second chunk of a handful of tiles cost a whole round of fetch + bound + append: 7 k of 63 k cycles)
#ifndef PQF_GROUP_BOUND
#define PQF_GROUP_BOUND 1   // the k-th bounds from 64 group minima (block_group_bound) instead of the histogram (block_kth_bound)
#endif
#define PQF_R1 8       // centroid distances per thread and chunk of the probe selection (8 192 centroids per chunk)
#define PQF_CAP 2048   // candidate slots kept in LDS
#define PQF_QT 4       // queries per block of the coarse part of ivf_prep_kernel (8: 232 VGPRs, two waves per SIMD, 24 us; 4: see DESIGN)
struct FusedArgs {
    const float* q;             // query rows [B][qstride], read with scalar loads (wave-uniform addresses)
    int qstride;
    const float4* cent_tiles;   // the centroid tiles, their count and the exact-distance plan of `num_features`
    uint32_t num_clusters, cent_ntiles;
    DistPlan cp, sp;            // sp = plan of one subvector (quantization)
    int num_probes;
    float* cdist;               // [B][cent_ntiles * 64] centroid distances (prep -> fused)
    uint8_t* qcodes;            // [B][m] (prep -> fused)
    const uint8_t* index_bytes; // remap (doc_out != nullptr): doc ids are read from the uploaded index file
    mdb_u128* doc_out;
    float* score_out;
    uint32_t* doc_counts_out;
    unsigned long long* zero4;  // four words cleared by block 0: the NEXT fused call's counters (no memset launch per call)
    unsigned long long* dbg;    // MDB_PQF_DBG: block 0 / thread 0 stores a cycle stamp after every phase
    uint32_t cap;               // candidate slots in use (<= PQF_CAP; tests shrink it to force the overflow pass)
    uint32_t cand_words;        // LDS words reserved for the candidate records (even)
    uint32_t b, m, coarse_blocks, quant_blocks, tile_groups;
    uint32_t no_masks;          // nothing was ever invalidated and the call has no planner filter: the scan reads neither tombstone nor allow words
    // COARSE == 2 (ivf_coarse_mfma_kernel ran): the query's candidate centroids, S segments of `cm_caps` slots, and the row-major centroids
    const uint2* cm_cand;
    const uint32_t* cm_cnt;
    const float* cent_rows;
    uint32_t cm_S, cm_caps;
    float cm_kappa, cm_xnmax;
    uint32_t cm_global;
};

// exact_sums<L2, QT> for vectors of whole 16-float chunks, written on float2: every subtract / multiply / add of the lane cascade
// is ONE v_pk_*_f32 on register pairs that are adjacent as loaded (the float4 halves of the centroid and of the LDS broadcast of the
// query; accumulator pairs (2p, 2p + 1)) — the generic form compiled to the same packed operations plus as many v_mov_b32 arranging
// their operands (502 moves beside 676 packed operations in ivf_prep_kernel).  Same operations in the same order per accumulator:
// (q - x) rounded, squared rounded, added rounded; chunk c before chunk c + 1; the ordered horizontal sum at the end.
typedef float mdb_f2 __attribute__((ext_vector_type(2)));
template <int QT>
__device__ __forceinline__ void l2_sums16_packed(const TileLoader& ld, const float* __restrict__ qs, int dpad, int n16, float (&out)[QT]) {
    mdb_f2 acc[QT][8];
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = mdb_f2{0.0f, 0.0f};
    auto add4 = [&](const float4 (&x)[4], int c) {
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            const float4* q4 = (const float4*)(qs + (size_t)i * dpad + 16 * c);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const float4 q = q4[kk];
                const mdb_f2 d0 = mdb_f2{q.x, q.y} - mdb_f2{x[kk].x, x[kk].y};
                const mdb_f2 d1 = mdb_f2{q.z, q.w} - mdb_f2{x[kk].z, x[kk].w};
                acc[i][2 * kk] = acc[i][2 * kk] + d0 * d0;
                acc[i][2 * kk + 1] = acc[i][2 * kk + 1] + d1 * d1;
            }
        }
    };
    int c = 0;
    for (; c + 2 <= n16; c += 2) {   // two chunks' loads in flight, as exact_sums issues them
        float4 xa[4], xb[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) { xa[kk] = ld.get4(4 * c + kk); xb[kk] = ld.get4(4 * c + 4 + kk); }
        add4(xa, c);
        add4(xb, c + 1);
    }
    if (c < n16) {
        float4 xa[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) xa[kk] = ld.get4(4 * c + kk);
        add4(xa, c);
    }
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        float s = 0.0f;   // simd_reduce_add_ordered
#pragma unroll
        for (int j = 0; j < 8; ++j) { s = __fadd_rn(s, acc[i][j].x); s = __fadd_rn(s, acc[i][j].y); }
        out[i] = __fadd_rn(0.0f, s);
    }
}

// The coarse part stages its PQF_QT query rows in LDS: every lane of a wave needs the same query element at the same time, an
// LDS broadcast read (one ds_read_b128 per four elements, in order, partially awaitable) delivers it straight into vector
// registers — per-lane vector loads of a uniform address cost an instruction per element (35 us for the kernel), scalar
// loads must all be awaited together and moved into vector registers for the packed math (56 us).
__global__ __launch_bounds__(256) void ivf_prep_kernel(FusedArgs f, const float* __restrict__ q, const float* __restrict__ cb,
                                                       float* __restrict__ cdist, uint8_t* __restrict__ qcodes, uint32_t* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) float qs[];   // [PQF_QT][dpad]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // the light, latency-bound quantize blocks come FIRST in dispatch order: they run in the shadow of the coarse blocks
    if (blockIdx.x >= f.quant_blocks) {
        // ---- distances to 4 tiles of centroids (one per wave) for PQF_QT queries: sqrt-L2 with the reference's lane cascade
        const uint32_t cbid = blockIdx.x - f.quant_blocks;
        const uint32_t g = cbid % f.tile_groups, qg = cbid / f.tile_groups;
        const uint32_t t = g * 4 + (uint32_t)wave;
        const uint32_t q0 = qg * PQF_QT;
        const uint32_t qn = min((uint32_t)PQF_QT, f.b - q0);
        const int d = f.cp.d, dpad = f.cp.d4 * 4 + 16;   // (+16: exact_sums forms, never dereferences, pointers past the row)
        for (int i = threadIdx.x; i < PQF_QT * dpad; i += 256) {
            const int qq = i / dpad, e = i % dpad;
            qs[i] = ((uint32_t)qq < qn && e < d) ? q[(size_t)(q0 + qq) * f.qstride + e] : 0.0f;   // a short last group: zero rows, not stored
        }
        __syncthreads();
        if (t >= f.cent_ntiles) return;
        TileLoader ld{f.cent_tiles + (size_t)t * f.cp.d4 * MDB_TILE + lane};
        float raw[PQF_QT];
        // (tried: the two-buffer form of exact_sums — 35 us instead of 24, registers; the centroid's whole vector in registers,
        // one load latency per tile — 29 us; 8 instead of 4 queries per block — 24 us: the kernel sits between its LDS
        // broadcast reads and its packed arithmetic, ~7 us each per CU, not on a latency chain)
#ifndef PQF_NO_PACKED_PREP
        if (f.cp.n8 == 0 && f.cp.n4 == 0 && f.cp.ntail == 0) l2_sums16_packed<PQF_QT>(ld, qs, dpad, f.cp.n16, raw);
        else
#endif
        exact_sums<MDB_METRIC_L2, PQF_QT, TileLoader, 0>(ld, qs, dpad, f.cp, raw);
        const size_t lpad = (size_t)f.cent_ntiles * MDB_TILE;
        bool nan_seen = false;
        const bool valid = t * MDB_TILE + (uint32_t)lane < f.num_clusters;
#pragma unroll
        for (int i = 0; i < PQF_QT; ++i) {
            if ((uint32_t)i < qn) {
                const float dist = finish_distance<MDB_METRIC_L2>(raw[i]);
                if (valid && dist != dist) nan_seen = true;
                cdist[(size_t)(q0 + i) * lpad + (size_t)t * MDB_TILE + lane] = dist;
            }
        }
        if (nan_seen) atomicOr(flags, MDB_FLAG_NAN);
        return;
    }
    // ---- the queries' codes (Q::QuantizedT::process_vector, index.rs:193): one wave per (query, subspace)
    const size_t task = (size_t)blockIdx.x * 4 + wave;
    if (task >= (size_t)f.b * f.m) return;
    const size_t qi = task / f.m;
    const int s = (int)(task % f.m);
    const int subdim = f.sp.d;
    const uint32_t code = pq_quantize_wave(q + qi * f.qstride + (size_t)s * subdim, cb + (size_t)s * 256 * subdim, 256, subdim, f.sp, lane);
    if (lane == 0) qcodes[task] = (uint8_t)code;
}

#include "mdb_ivf_coarse.hip.h"

// (block_kth_bound / kth_area_reset: mdb_device.hip.h — shared with the merge of many sorted partial lists, mdb_flat.hip)
static_assert(PQF_QT <= 4, "ivf_prep_kernel's query groups read the caller's rows in place: at most 4 rows per group (stage_queries)");
template <int SUBDIM, int MW, int COARSE>   // COARSE: 0 probes given, 1 the [B][L] distances of ivf_prep_kernel, 2 the candidates of ivf_coarse_mfma_kernel
__global__ __launch_bounds__(PQF_BLOCK) void ivf_pq_fused_kernel(ScanArgs a, FusedArgs f, const uint32_t* __restrict__ codes,
                                                                 const float* __restrict__ cb, const float* __restrict__ sdc) {
    constexpr int m = 4 * MW, nbits = 8, K = 256, S4 = SUBDIM / 4;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint32_t* red = (uint32_t*)lds;                        // [64]
    uint32_t* hist = red + 64;                             // 2 x [PQF_NB + 32]: block_kth_bound's alternating areas
    uint32_t* misc = hist + 2 * (PQF_NB + 32);             // [0] candidates [1] scored [2] coarse candidates
    uint32_t* gm = misc + 16;                              // [64 + 3 (+ pad to 80)] block_group_bound's minima and result words
    uint32_t* pstart = gm + 80;                            // [64]  first tile of probe j
    uint32_t* ppref = pstart + 64;                         // [65]  exclusive prefix of the probes' tile counts (+ pad to 80)
    uint32_t* probes_l = ppref + 80;                       // [64]
    uint32_t* qcode = probes_l + 64;                       // [m <= 32]
    float* qv = (float*)(qcode + 32);                      // the query's own codebook rows [m][SUBDIM]
    float* btab = qv + m * SUBDIM;                         // [m * 256]: the row's f32 sum (ivf_scan_pq3_kernel's table and bracket)
    uint32_t* cand = (uint32_t*)(btab + m * K);            // [PQF_CAP][1 + MW]: a candidate's point id and code words
    uint64_t* ck = (uint64_t*)(cand + f.cand_words);      // [PQF_CAP] keys: coarse candidates, then the candidates' exact keys
    uint64_t* wkey = ck + PQF_CAP;                         // [64] the winners, ascending
    uint64_t* rlo = wkey + 64;                             // remap: [64] doc id halves, scores
    uint64_t* rhi = rlo + 64;
    float* rsc = (float*)(rhi + 64);
    char* sel_lds = (char*)(rsc + 64);                     // the streaming selector of the overflow paths
    const int qi = blockIdx.x;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid / MDB_WAVE), lane = tid % MDB_WAVE;
    const IvfUserDev u = a.users[0];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    bool nan_seen = false, bad = false;
    unsigned scored = 0;
    if (f.zero4 && qi == 0 && tid < 4) f.zero4[tid] = 0ull;
    if (tid < 16) misc[tid] = 0;
    kth_area_reset(hist);
    int flip = 0, rot = 0;
    constexpr int TPW = MW <= 4 ? PQF_TPW_MAX : 4;
    __syncthreads();   // the first block_kth_bound call adds to the area's min / max / count words: they must be cleared by then
#define PQF_STAMP(i) do { if (f.dbg && qi == 0 && tid == 0) f.dbg[i] = __builtin_readcyclecounter(); } while (0)
#define PQF_SUB(i) do { if (f.dbg) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); PQF_STAMP(i); } } while (0)
    PQF_STAMP(0);
    // the first chunk of the query's centroid distances (ivf_prep_kernel's rows: written by another launch, so they come from the
    // Infinity Cache / HBM) is requested BEFORE the quantization below and used behind it
    const CmSelect cs{f.cm_cand, f.cm_cnt, f.cent_rows, f.cent_tiles, f.cm_S, f.cm_caps, f.num_clusters, f.b, f.cm_kappa, f.cm_xnmax, f.cp, f.cm_global};
    CmPre<PQF_BLOCK> cm_pre;
    if (COARSE == 2) cm_prefetch<PQF_BLOCK>(cs, (uint32_t)qi, f.q + (size_t)qi * f.qstride, cm_pre);
    uint32_t v0[PQF_R1];
    if (COARSE == 1) {
        const float* dist = f.cdist + (size_t)qi * (f.cent_ntiles * MDB_TILE);
#pragma unroll
        for (int r = 0; r < PQF_R1; ++r) {
            const uint32_t idx = (uint32_t)(r * PQF_BLOCK + tid);
            v0[r] = idx < f.num_clusters ? min(f32_orderable(dist[idx]), 0xFFFFFFFEu) : 0xFFFFFFFFu;   // (all ones = "none")
        }
    }
    // ---- 0. the query's codes (Q::QuantizedT::process_vector, index.rs:193): one wave per subspace (qcodes != nullptr: already
    //         computed by ivf_prep_kernel)
    if (!f.qcodes) {
        const float* qrow = f.q + (size_t)qi * f.qstride;
        for (int s0 = wave; s0 < m; s0 += PQF_NW) {
            const uint32_t code = pq_quantize_wave(qrow + (size_t)s0 * SUBDIM, cb + (size_t)s0 * K * SUBDIM, K, SUBDIM, f.sp, lane);
            if (lane == 0) qcode[s0] = code;
        }
    } else if (tid < m) qcode[tid] = f.qcodes[(size_t)qi * m + tid];
    PQF_STAMP(7);
#ifndef MDB_PQF_NO_TABLE_PREFETCH
    // the query's rows of the code-to-code table depend on its codes only: requested HERE (m K / PQF_BLOCK = MW words per thread), they
    // travel while the block selects its probes and are stored behind that phase — the table costs no round trip of its own
    float sdc_pre[MW];
    const bool tab_pre = COARSE == 2 && sdc != nullptr;
    if (tab_pre) {
        __syncthreads();   // qcode
#pragma unroll
        for (int x = 0; x < MW; ++x) {
            const int i = tid + x * PQF_BLOCK;
            sdc_pre[x] = sdc[((size_t)(i >> nbits) * K + qcode[i >> nbits]) * K + (i & (K - 1))];
        }
    }
#else
    const bool tab_pre = false;
    float sdc_pre[MW];
#endif

    // ---- 1. find_nearest_centroids: the num_probes nearest by (distance, index) among the distances of ivf_prep_kernel
    int np = f.num_probes;
    if (COARSE == 2) {
        // the candidates ivf_coarse_mfma_kernel left for this query: exact distances, rank by (distance, index) (mdb_ivf_coarse.hip.h)
        np = min(np, (int)f.num_clusters);
        // (their ids, counts and the query row were requested at the start of the block: cm_pre; the candidate records' area is free until phase 3)
        cm_select_probes<PQF_BLOCK>(cs, cm_pre, (uint32_t)qi, f.q + (size_t)qi * f.qstride, np, pstart, &misc[3], ck, (uint32_t)PQF_CAP, sel_lds, cand, probes_l, nan_seen, f.dbg, gm, &rot);
    } else if (COARSE == 1) {
        const uint32_t lpad = f.cent_ntiles * MDB_TILE;
        const float* dist = f.cdist + (size_t)qi * lpad;
        np = min(np, (int)f.num_clusters);
        uint32_t thr1 = 0xFFFFFFFFu;   // image of an upper bound of the np-th distance (tightens chunk by chunk)
        for (uint32_t c0 = 0; c0 < f.num_clusters; c0 += PQF_R1 * PQF_BLOCK) {
            uint32_t v[PQF_R1];
#pragma unroll
            for (int r = 0; r < PQF_R1; ++r) {
                const uint32_t idx = c0 + (uint32_t)(r * PQF_BLOCK + tid);
                if (c0 == 0) v[r] = v0[r];
                else v[r] = idx < f.num_clusters ? min(f32_orderable(dist[idx]), 0xFFFFFFFEu) : 0xFFFFFFFFu;   // (all ones = "none")
            }
            if (c0 == 0) PQF_SUB(8);
            thr1 = min(thr1, PQF_GROUP_BOUND ? block_group_bound<PQF_R1>(v, (uint32_t)np, gm, rot)
                                             : block_kth_bound<PQF_R1>(v, (uint32_t)np, hist, flip));
            if (c0 == 0) PQF_SUB(9);
#pragma unroll
            for (int r = 0; r < PQF_R1; ++r) {
                const bool in = v[r] <= thr1 && v[r] != 0xFFFFFFFFu;
                const unsigned long long bm = __ballot(in);
                if (bm) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&misc[2], (uint32_t)__popcll(bm));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    const uint32_t pos = base + (uint32_t)__popcll(bm & lt_mask);
                    if (in && pos < PQF_CAP) ck[pos] = ((uint64_t)v[r] << 32) | (c0 + (uint32_t)(r * PQF_BLOCK + tid));
                }
            }
        }
        __syncthreads();
        PQF_SUB(10);
        const uint32_t nc1 = misc[2];
        if (nc1 <= PQF_CAP) {
            // rank by counting: keys are distinct (the index is part of the key)
            for (uint32_t i = tid; i < nc1; i += PQF_BLOCK) {
                const uint64_t key = ck[i];
                uint32_t rank = 0;
                for (uint32_t j = 0; j < nc1; ++j) rank += ck[j] < key ? 1u : 0u;
                if (rank < (uint32_t)np) probes_l[rank] = (uint32_t)key;
            }
        } else {
            // thousands of centroids tie with the np-th: the streaming selector over all of them
            BlockSelect<PQF_BLOCK> sel;
            sel.init(sel_lds, np);
            for (uint32_t i0 = 0; i0 < f.num_clusters; i0 += PQF_BLOCK) {
                const uint32_t idx = i0 + (uint32_t)tid;
                sel.offer(idx < f.num_clusters ? (((uint64_t)min(f32_orderable(dist[idx]), 0xFFFFFFFEu) << 32) | idx) : MDB_KEY_MAX);
                sel.round_end();
            }
            sel.finish();
            if (tid < np) probes_l[tid] = (uint32_t)sel.buf[tid];
        }
    } else {
        np = a.probe_cnt ? (int)a.probe_cnt[qi] : a.probe_stride;
        if (tid < 64) probes_l[tid] = tid < np ? a.probes[(size_t)qi * a.probe_stride + tid] : 0xFFFFFFFFu;
    }
    __syncthreads();   // qcode (and probes_l)
    PQF_STAMP(1);
    // ---- 2. the query's own codebook rows (codes from ivf_prep_kernel), then the bound table (ivf_scan_pq3_kernel's arithmetic)
    for (int i = tid; i < m * SUBDIM; i += PQF_BLOCK) {
        const int s = i / SUBDIM;
        qv[i] = cb[((size_t)s * K + qcode[s]) * SUBDIM + (i % SUBDIM)];
    }
    // (with the row-sum table nothing below reads qv before the barrier behind the table: the codebook rows, the lists' tile offsets and
    // the table rows are ONE memory round trip instead of two)
    if (!sdc) __syncthreads();   // qv
    // ... and the flattened tile sequence of the probed lists (wave 0; independent of the table)
    if (tid < 64) {
        uint32_t t0 = 0, cnt = 0;
        if (tid < np) {
            const uint32_t c = probes_l[tid];
            if (c >= u.num_lists) bad = true;
            else {
                const uint32_t g = u.list_base + c;
                t0 = a.list_tile_off[g];
                cnt = a.list_tile_off[g + 1] - t0;
            }
        }
        pstart[tid] = t0;
        uint32_t incl = cnt;
#pragma unroll
        for (int o = 1; o < MDB_WAVE; o <<= 1) {
            const uint32_t vv = __shfl_up(incl, o);
            if (lane >= o) incl += vv;
        }
        ppref[tid + 1] = incl;   // entries past np repeat the total
        if (tid == 0) ppref[0] = 0;
    }
    if (tab_pre) {
#pragma unroll
        for (int x = 0; x < MW; ++x) btab[tid + x * PQF_BLOCK] = sdc_pre[x];
    } else if (sdc) {   // the query's rows of the code-to-code table (pq_sdc_kernel: the values the loop below computes)
        for (int i = tid; i < m * K; i += PQF_BLOCK) btab[i] = sdc[((size_t)(i >> nbits) * K + qcode[i >> nbits]) * K + (i & (K - 1))];
    } else
    for (int i = tid; i < m * K; i += PQF_BLOCK) {
        const float4* row = (const float4*)cb + (size_t)i * S4;
        const float4* q4 = (const float4*)qv + (i >> nbits) * S4;
        float sum = 0.0f;
#pragma unroll
        for (int x = 0; x < S4; ++x) {
            const float4 c = row[x], q = q4[x];
            sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q.x, c.x));   // every term >= 0
            sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q.y, c.y));
            sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q.z, c.z));
            sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q.w, c.w));
        }
        btab[i] = sum;   // S (1 - g) <= exact <= S (1 + g) for the total S of m such words, g as in ivf_scan_pq3_kernel
    }
    const float gmar = 1.5f * (float)(m * SUBDIM + m + SUBDIM + 16) * 5.9604645e-8f;
    const float lo_f = 1.0f - gmar, hi_f = 1.0f + gmar;
    __syncthreads();   // btab, pstart, ppref
    PQF_STAMP(2);
    const int T = (int)ppref[64];

    // lower / upper bound of one stored code against the query's
    auto bounds = [&](const uint32_t (&cwv)[MW], float& lb, float& ub) {
        float tot = 0.0f;
#pragma unroll
        for (int w = 0; w < MW; ++w) {
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                const uint32_t code = (cwv[w] >> (8 * bi)) & 0xFFu;
                tot = __fadd_rn(tot, btab[((w * 4 + bi) << nbits) + code]);
            }
        }
        lb = __fmul_rn(tot, lo_f);
        ub = __fmul_rn(tot, hi_f);
    };
    // exact symmetric distance of one stored code (ivf_scan_pq2_kernel::exact_key's terms and association; rows from L2)
    auto exact_key = [&](uint32_t vid, const uint32_t (&cwv)[MW]) -> uint64_t {
        float s16[16], s8[8], s4[4];
#pragma unroll
        for (int x = 0; x < 16; ++x) s16[x] = 0.0f;
#pragma unroll
        for (int x = 0; x < 8; ++x) s8[x] = 0.0f;
#pragma unroll
        for (int x = 0; x < 4; ++x) s4[x] = 0.0f;
#pragma unroll
        for (int w = 0; w < MW; ++w) {
#pragma unroll
            for (int bi = 0; bi < 4; ++bi) {
                const int s = w * 4 + bi;
                const uint32_t code = (cwv[w] >> (8 * bi)) & 0xFFu;
                const float4* c4 = (const float4*)cb + ((size_t)(s << nbits) + code) * S4;
                const float4* q4 = (const float4*)qv + s * S4;
                float trow[SUBDIM];
#pragma unroll
                for (int x = 0; x < S4; ++x) {
                    const float4 q = q4[x], cc = c4[x];
                    trow[4 * x + 0] = acc_term<MDB_METRIC_L2>(0.0f, q.x, cc.x);
                    trow[4 * x + 1] = acc_term<MDB_METRIC_L2>(0.0f, q.y, cc.y);
                    trow[4 * x + 2] = acc_term<MDB_METRIC_L2>(0.0f, q.z, cc.z);
                    trow[4 * x + 3] = acc_term<MDB_METRIC_L2>(0.0f, q.w, cc.w);
                }
                pq2_add_row<SUBDIM>(trow, s16, s8, s4);
            }
        }
        const float rs = __fadd_rn(__fadd_rn(__fadd_rn(reduce_ordered<16>(s16), reduce_ordered<8>(s8)), reduce_ordered<4>(s4)), 0.0f);
        if (rs != rs) nan_seen = true;
        return make_key(rs, vid);
    };
    // tile t of the flattened sequence -> its tile index
    auto tile_of = [&](int t) -> uint32_t {
        const int j = __popcll(__ballot(ppref[lane + 1] <= (uint32_t)t));   // lists that end at or before t (entries past np hold T > t)
        return pstart[j] + ((uint32_t)t - ppref[j]);
    };

    // ---- 3. bounds pass, a chunk of 16 TPW tiles at a time: wave w takes tiles c0 + w + 16 x (x < TPW), all fetched at once
    uint32_t thr_ub = 0xFFFFFFFFu;   // image of an upper bound of the k-th exact distance (tightens chunk by chunk)
    for (int c0 = 0; c0 < T; c0 += PQF_NW * TPW) {
        uint32_t pid[TPW], cw[TPW][MW];
#pragma unroll
        for (int x = 0; x < TPW; ++x) {
            const int t = c0 + wave + PQF_NW * x;
            pid[x] = 0xFFFFFFFFu;
#pragma unroll
            for (int w = 0; w < MW; ++w) cw[x][w] = 0;
            if (t < T) {   // wave-uniform
                const uint32_t tile = tile_of(t);
                pid[x] = a.slot_ids[(size_t)tile * MDB_TILE + lane];
                const uint32_t* cwp = codes + (size_t)tile * MW * MDB_TILE + lane;
#pragma unroll
                for (int w = 0; w < MW; ++w) cw[x][w] = cwp[(size_t)w * MDB_TILE];
            }
        }
        if (c0 == 0) PQF_SUB(11);
        uint32_t tw[TPW], aw[TPW];
#pragma unroll
        for (int x = 0; x < TPW; ++x) { tw[x] = 0u; aw[x] = 0xFFFFFFFFu; }
        if (!f.no_masks) {   // (a dependent memory trip of the chain: ~3 k of the step's 54 k cycles)
#pragma unroll
            for (int x = 0; x < TPW; ++x) {
                const uint32_t pz = pid[x] == 0xFFFFFFFFu ? 0u : pid[x];
                tw[x] = a.tomb[u.tomb_base + (pz >> 5)];
                aw[x] = a.allow[(size_t)qi * a.allow_stride + ((pz >> 5) & a.allow_mask)];
            }
        }
        if (c0 == 0) PQF_SUB(12);
        uint32_t ubi[TPW], lbi[TPW];
#pragma unroll
        for (int x = 0; x < TPW; ++x) {
            const bool take = pid[x] != 0xFFFFFFFFu && !((tw[x] >> (pid[x] & 31)) & 1u) && ((aw[x] >> (pid[x] & 31)) & 1u);
            ubi[x] = 0xFFFFFFFFu;
            lbi[x] = 0xFFFFFFFFu;   // "not taken"
            if (take) {
                ++scored;
                float lb, ub;
                bounds(cw[x], lb, ub);
                const uint32_t ui = f32_orderable(ub);
                ubi[x] = ui == 0xFFFFFFFFu ? 0xFFFFFFFEu : ui;                      // NaN: sorts last, never lowers the bound
                lbi[x] = lb == lb ? min(f32_orderable(lb), 0xFFFFFFFEu) : 0u;   // a NaN bound always survives: the exact pass reports it
            }
        }
        if (c0 == 0) PQF_SUB(13);
        thr_ub = min(thr_ub, PQF_GROUP_BOUND ? block_group_bound<TPW>(ubi, (uint32_t)a.k, gm, rot)
                                             : block_kth_bound<TPW>(ubi, (uint32_t)a.k, hist, flip));
        if (c0 == 0) PQF_SUB(14);
#pragma unroll
        for (int x = 0; x < TPW; ++x) {
            const bool surv = lbi[x] != 0xFFFFFFFFu && lbi[x] <= thr_ub;
            const unsigned long long sm = __ballot(surv);
            if (sm) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&misc[0], (uint32_t)__popcll(sm));
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                const uint32_t pos = base + (uint32_t)__popcll(sm & lt_mask);
                if (surv && pos < f.cap) {   // the exact pass needs no second trip to the posting list
                    cand[pos * (1 + MW)] = pid[x];
#pragma unroll
                    for (int w = 0; w < MW; ++w) cand[pos * (1 + MW) + 1 + w] = cw[x][w];
                }
            }
        }
    }
    {
        unsigned long long ws = scored;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ws += __shfl_xor((unsigned)ws, o);
        if (lane == 0 && ws) atomicAdd(&misc[1], (uint32_t)ws);
    }
    __syncthreads();
    PQF_STAMP(3);
    // one device-scope atomic per BLOCK: thousands of atomics on one cache line serialise
    if (tid == 0 && misc[1]) atomicAdd(&a.counters[2], (unsigned long long)misc[1]);
    const uint32_t nc = misc[0];
    int c = 0;   // winners
    // ---- 4. exact distances of the candidates, top-k by (distance, point id)
    if (nc <= f.cap) {
#ifdef MDB_PQF_EXACT_PER_THREAD
        for (uint32_t i = tid; i < nc; i += PQF_BLOCK) {
            uint32_t cwv[MW];
#pragma unroll
            for (int w = 0; w < MW; ++w) cwv[w] = cand[i * (1 + MW) + 1 + w];
            ck[i] = exact_key(cand[i * (1 + MW)], cwv);
        }
#else
        // exact_key's arithmetic with one THREAD PER ACCUMULATOR LANE of the reference's pass instead of one per candidate: the terms of
        // a subvector of SUBDIM elements go to min(SUBDIM, 16) lane accumulators (pq2_add_row), each an independent chain over the
        // subspaces — NL adjacent threads take the NL lanes of a candidate (their codebook loads are adjacent floats of the same rows),
        // then the lanes are summed in the reference's order.  The ~100 candidates of a query kept 2 of the block's 16 waves busy with
        // ~500 dependent instructions each (11 k of the step's 56 k cycles); now every wave works and a thread's chain is m terms.
        {
            constexpr int NL = SUBDIM >= 16 ? 16 : SUBDIM;   // accumulator lanes that receive terms (s16, s8 or s4 of pq2_add_row)
            constexpr int NCH = SUBDIM / NL;                  // elements of a row per lane (32-element subvectors: two)
            constexpr int SB = 16 / NCH;                      // subspaces whose loads are issued together
            constexpr int CPP = PQF_BLOCK / NL;               // candidates per pass
            const int jl = tid % NL;
            for (uint32_t i0 = 0; i0 < nc; i0 += CPP) {
                const uint32_t i = i0 + (uint32_t)(tid / NL);
                const bool valid = i < nc;
                float accl = 0.0f;
                uint32_t vid = 0;
                if (valid) {
                    vid = cand[i * (1 + MW)];
                    uint32_t cwv[MW];
#pragma unroll
                    for (int w = 0; w < MW; ++w) cwv[w] = cand[i * (1 + MW) + 1 + w];
#pragma unroll
                    for (int s0 = 0; s0 < m; s0 += SB) {
                        float cv[SB * NCH];
#pragma unroll
                        for (int x = 0; x < SB; ++x) {
                            const int sb = s0 + x;
                            if (sb < m) {
                                const uint32_t code = (cwv[sb >> 2] >> (8 * (sb & 3))) & 0xFFu;
#pragma unroll
                                for (int cc = 0; cc < NCH; ++cc) cv[x * NCH + cc] = cb[((size_t)(sb << nbits) + code) * SUBDIM + NL * cc + jl];
                            }
                        }
#pragma unroll
                        for (int x = 0; x < SB; ++x) {
                            const int sb = s0 + x;
                            if (sb < m) {
#pragma unroll
                                for (int cc = 0; cc < NCH; ++cc)
                                    accl = __fadd_rn(accl, acc_term<MDB_METRIC_L2>(0.0f, qv[sb * SUBDIM + NL * cc + jl], cv[x * NCH + cc]));
                            }
                        }
                    }
                }
                // reduce_ordered over the NL lanes (lane 0 first); the two accumulator groups that received nothing add +0.0
                float rs = 0.0f;
#pragma unroll
                for (int j = 0; j < NL; ++j) rs = __fadd_rn(rs, __shfl(accl, (lane & ~(NL - 1)) + j));
                rs = __fadd_rn(__fadd_rn(__fadd_rn(rs, 0.0f), 0.0f), 0.0f);
                if (valid && jl == 0) {
                    if (rs != rs) nan_seen = true;
                    ck[i] = make_key(rs, vid);
                }
            }
        }
#endif
        __syncthreads();
        PQF_STAMP(4);
        // rank by counting; equal keys (a point in two probed lists) are ordered by their place in the list
        for (uint32_t i = tid; i < nc; i += PQF_BLOCK) {
            const uint64_t key = ck[i];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nc; ++j) {
                const uint64_t o = ck[j];
                rank += (o < key || (o == key && j < i)) ? 1u : 0u;
            }
            if (rank < (uint32_t)a.k) wkey[rank] = key;
        }
        c = (int)min(nc, (uint32_t)a.k);
        __syncthreads();
    } else {
        // the list overflowed (thousands of vectors within the bound: heavy ties): second pass over the tiles with the streaming
        // selector, exact evaluation of everything the FINAL bound lets through
        BlockSelect<PQF_BLOCK> sel;
        sel.init(sel_lds, a.k);
        const int rounds = (T + PQF_NW - 1) / PQF_NW;
        for (int r = 0; r < rounds; ++r) {
            const int t = r * PQF_NW + wave;
            uint64_t key = MDB_KEY_MAX;
            if (t < T) {
                const uint32_t tile = tile_of(t);
                const uint32_t pidv = a.slot_ids[(size_t)tile * MDB_TILE + lane];
                const uint32_t* cwp = codes + (size_t)tile * MW * MDB_TILE + lane;
                uint32_t cwv[MW];
#pragma unroll
                for (int w = 0; w < MW; ++w) cwv[w] = cwp[(size_t)w * MDB_TILE];
                const uint32_t pz = pidv == 0xFFFFFFFFu ? 0u : pidv;
                const uint32_t twv = a.tomb[u.tomb_base + (pz >> 5)];
                const uint32_t awv = a.allow[(size_t)qi * a.allow_stride + ((pz >> 5) & a.allow_mask)];
                const bool take = pidv != 0xFFFFFFFFu && !((twv >> (pidv & 31)) & 1u) && ((awv >> (pidv & 31)) & 1u);
                if (take) {
                    float lb, ub;
                    bounds(cwv, lb, ub);
                    if (!(lb == lb && f32_orderable(__fmul_rn(lb, 0.99998f)) > thr_ub)) key = exact_key(pidv, cwv);
                }
            }
            sel.offer(key);
            sel.round_end();
        }
        sel.finish();
        c = (int)sel.count();
        if (tid < c) wkey[tid] = sel.buf[tid];
        __syncthreads();
    }
    PQF_STAMP(5);
    if (nan_seen) atomicOr(a.flags, MDB_FLAG_NAN);
    if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
    if (!f.doc_out) {  // (distance, point id) rows: search_with_centroids
        uint64_t* dst = a.partial + (size_t)qi * a.k;
        if (tid < a.k) dst[tid] = tid < c ? wkey[tid] : MDB_KEY_MAX;
        if (a.counts_out && tid == 0) a.counts_out[qi] = (uint32_t)c;
        return;
    }
    // ---- 5. search_with_centroids_and_remap: doc ids, IdWithScore order (remap_kernel's rank sort; k <= 64)
    if (tid < c) {
        const uint64_t key = wkey[tid];
        const uint64_t* dp = (const uint64_t*)(f.index_bytes + u.doc_ids_off + (size_t)key_id(key) * 16);
        rlo[tid] = dp[0];
        rhi[tid] = dp[1];
        rsc[tid] = key_dist(key);
    }
    __syncthreads();
    if (tid < a.k) {
        if (tid < c) {
            int rank = 0;
            const float sv = rsc[tid];
            const uint64_t l = rlo[tid], h = rhi[tid];
            for (int i = 0; i < c; ++i) {
                const float si = rsc[i];
                const bool less = si < sv || (si == sv && (rhi[i] < h || (rhi[i] == h && (rlo[i] < l || (rlo[i] == l && i < tid)))));
                rank += less ? 1 : 0;
            }
            f.doc_out[(size_t)qi * a.k + rank] = mdb_u128{l, h};
            f.score_out[(size_t)qi * a.k + rank] = sv;
        } else {
            f.doc_out[(size_t)qi * a.k + tid] = mdb_u128{~0ull, ~0ull};
            f.score_out[(size_t)qi * a.k + tid] = __uint_as_float(0x7F800000u);
        }
    }
    if (tid == 0 && f.doc_counts_out) f.doc_counts_out[qi] = (uint32_t)c;
    PQF_STAMP(6);
#undef PQF_STAMP
#undef PQF_SUB
}

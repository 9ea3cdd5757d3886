// mdb_ivf_pq2.hip.h — device code of mdb_ivf.hip, part 2: the PQ fast path (per-element table in LDS) and the two-phase PQ scan with its
// refine.  Included by mdb_ivf.hip only, after mdb_ivf_scan.hip.h.
#pragma once

// ------------------------------------------------------------------------------------------
// PQ posting-list scan, fast path: SUBDIM (compile time, multiple of 4, power of two) floats per
// codebook row, per-element table in LDS (bit-exact association).
//   * 1024 threads = 16 waves, one block per (query, split); the 128 KB table is built once per block
//     with float4 traffic only;
//   * all probed lists of the query are flattened into one tile sequence (LDS prefix array), so every
//     wave has a tile in every round whatever the list lengths;
//   * 2-deep software pipeline over rounds: slot ids + code words of round r+2 and the tombstone
//     words of round r+1 are in flight while round r adds table rows (the only barrier per round is
//     BlockSelect's).
// LDS reads are the floor: d/4 ds_read_b128 per scored vector.
#define PQ2_BLOCK 1024
#define PQ2_NW (PQ2_BLOCK / MDB_WAVE)
#define PQ2_PCH 512  // probes per chunk of the flattened tile sequence

template <int SUBDIM>
__device__ __forceinline__ void pq2_add_row(const float* __restrict__ row, float (&s16)[16], float (&s8)[8], float (&s4)[4]) {
    constexpr int N16 = SUBDIM / 16, N8 = (SUBDIM % 16) / 8, N4 = (SUBDIM % 8) / 4;
#pragma unroll
    for (int c = 0; c < N16; ++c) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            float4 t = *(const float4*)(row + 16 * c + 4 * v);
            s16[4 * v + 0] = __fadd_rn(s16[4 * v + 0], t.x);
            s16[4 * v + 1] = __fadd_rn(s16[4 * v + 1], t.y);
            s16[4 * v + 2] = __fadd_rn(s16[4 * v + 2], t.z);
            s16[4 * v + 3] = __fadd_rn(s16[4 * v + 3], t.w);
        }
    }
    if (N8) {
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            float4 t = *(const float4*)(row + 16 * N16 + 4 * v);
            s8[4 * v + 0] = __fadd_rn(s8[4 * v + 0], t.x);
            s8[4 * v + 1] = __fadd_rn(s8[4 * v + 1], t.y);
            s8[4 * v + 2] = __fadd_rn(s8[4 * v + 2], t.z);
            s8[4 * v + 3] = __fadd_rn(s8[4 * v + 3], t.w);
        }
    }
    if (N4) {
        float4 t = *(const float4*)(row + 16 * N16 + 8 * N8);
        s4[0] = __fadd_rn(s4[0], t.x);
        s4[1] = __fadd_rn(s4[1], t.y);
        s4[2] = __fadd_rn(s4[2], t.z);
        s4[3] = __fadd_rn(s4[3], t.w);
    }
}

// FULL: m == 4 MW and nbits == 8 (the usual codebooks) as COMPILE-TIME facts.  With run-time m / nbits every one of the m lookups
// of a vector sat behind its own uniform branch (`s < m`, the condition masks and per-subspace table bases were 48 spilled scalars,
// re-read with v_readlane per lookup) and its LDS read was waited for at once: m dependent LDS round trips per tile.  Constant-folded,
// the reads become m independent ds_reads with immediate offsets.
template <int METRIC, int SUBDIM, int MW, bool FILT, bool FULL>
__global__ __launch_bounds__(PQ2_BLOCK) void ivf_scan_pq2_kernel(ScanArgs a, const uint32_t* __restrict__ codes, int m_rt,
                                                                 int nbits_rt, const float* __restrict__ cb,
                                                                 const uint8_t* __restrict__ qcodes) {
    static_assert(SUBDIM % 4 == 0 && (SUBDIM & (SUBDIM - 1)) == 0, "SUBDIM: power of two >= 4");
    const int m = FULL ? 4 * MW : m_rt, nbits = FULL ? 8 : nbits_rt;
    if (a.gate && __builtin_nontemporal_load(a.gate) == 0u) return;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    BlockSelect<PQ2_BLOCK> sel;
    sel.init(lds, a.k);
    uint32_t* pstart = (uint32_t*)(lds + ((BlockSelect<PQ2_BLOCK>::lds_bytes(a.k) + 15) & ~(size_t)15));
    uint32_t* ppref = pstart + PQ2_PCH;             // [PQ2_PCH + 1] exclusive prefix of tile counts
    float* qv = (float*)(ppref + PQ2_PCH + 16);     // the query's own codebook rows [m][SUBDIM]
    float* lut = qv + m * SUBDIM;
    uint16_t* atab = (uint16_t*)(lut + (size_t)(m << nbits) * SUBDIM);  // FILT: lower bounds of the row sums, bf16
    const int qi = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid / MDB_WAVE), lane = tid % MDB_WAVE;
    const IvfUserDev u = a.users[a.q_user ? a.q_user[qi] : 0];
    const uint8_t* qc = qcodes + (size_t)qi * m;
    const int np = a.probe_cnt ? (int)a.probe_cnt[qi] : a.probe_stride;
    const int K = 1 << nbits;
    constexpr int S4 = SUBDIM / 4;
    bool nan_seen = false, bad = false;
    unsigned scored = 0;
    const bool eager_trim = a.eager_trim != 0;

    // ---- table: lut[s][c][e] = term(q_s[e], cb[s][c][e]), each individually rounded
    for (int i = tid; i < m * SUBDIM; i += PQ2_BLOCK) {
        int s = i / SUBDIM;
        qv[i] = cb[((size_t)s * K + qc[s]) * SUBDIM + (i % SUBDIM)];
    }
    __syncthreads();
    {
        const int row4 = K * S4, total4 = m * row4;
        const float4* cb4 = (const float4*)cb;
        for (int i4 = tid; i4 < total4; i4 += PQ2_BLOCK) {
            int s = i4 / row4;  // row4 is a power of two: a shift
            float4 q = ((const float4*)qv)[s * S4 + (i4 & (S4 - 1))];
            float4 c = cb4[i4], t;
            t.x = acc_term<METRIC>(0.0f, q.x, c.x);  // 0 + term == term exactly
            t.y = acc_term<METRIC>(0.0f, q.y, c.y);
            t.z = acc_term<METRIC>(0.0f, q.z, c.z);
            t.w = acc_term<METRIC>(0.0f, q.w, c.w);
            ((float4*)lut)[i4] = t;
        }
    }
    __syncthreads();
    if (FILT) {
        // L2 only (every term >= 0).  atab[s][c] <= the REAL sum of row (s, c): f32 sum, shrunk by more than its
        // rounding error, truncated to bf16.  A vector whose bound already exceeds the selector's admission threshold
        // cannot be admitted: its exact distance (sum of the same non-negative terms in the reference's order,
        // <= 64 roundings) is >= (1 - 2^-17) x the real sum.  16 two-byte LDS reads replace 16 row reads for it.
        for (int i = tid; i < (m << nbits); i += PQ2_BLOCK) {
            const float* row = lut + (size_t)i * SUBDIM;
            float sum = 0.0f;
#pragma unroll
            for (int e = 0; e < SUBDIM; ++e) sum = __fadd_rn(sum, row[e]);
            const float low = __fmul_rn(sum, 0.99999f);
            atab[i] = sum != sum ? (uint16_t)0x7FC0u : (uint16_t)(__float_as_uint(low) >> 16);
        }
        __syncthreads();
    }

    // exact symmetric distance of one stored code (this lane's) against the query's, as a selection key
    // (always_inline: left as a call for the widest shapes — SUBDIM 16 / 32 with 8 code words — its table reads became flat loads)
    auto exact_key = [&](uint32_t vid, const uint32_t (&cwv)[MW], bool active) __attribute__((always_inline)) -> uint64_t {
        if (!active) return MDB_KEY_MAX;
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
                int s = w * 4 + bi;
                if (s < m) {
                    uint32_t code = (cwv[w] >> (8 * bi)) & 0xFFu;
                    pq2_add_row<SUBDIM>(lut + ((size_t)(s << nbits) + code) * SUBDIM, s16, s8, s4);
                }
            }
        }
        float rs = __fadd_rn(__fadd_rn(__fadd_rn(reduce_ordered<16>(s16), reduce_ordered<8>(s8)), reduce_ordered<4>(s4)), 0.0f);
        float dist = METRIC == MDB_METRIC_L2 ? rs : -rs;
        if (dist != dist) nan_seen = true;
        return make_key(dist, vid);
    };
    // FILT: survivors of the bound filter waiting for their exact evaluation (one per lane, lanes < pend_n)
    uint32_t pend_pid = 0xFFFFFFFFu, pend_cw[MW];
#pragma unroll
    for (int w = 0; w < MW; ++w) pend_cw[w] = 0;
    int pend_n = 0;

    if (u.valid) {
        for (int p0 = 0; p0 < np; p0 += PQ2_PCH) {
            const int n = min(PQ2_PCH, np - p0);
            // flatten this chunk's lists into one tile sequence
            if (tid < PQ2_PCH) {
                uint32_t t0 = 0, cnt = 0;
                if (tid < n) {
                    uint32_t c = a.probes[(size_t)qi * a.probe_stride + p0 + tid];
                    if (c >= u.num_lists) bad = true;
                    else {
                        uint32_t g = u.list_base + c;
                        t0 = a.list_tile_off[g];
                        cnt = a.list_tile_off[g + 1] - t0;
                    }
                }
                pstart[tid] = t0;
                ppref[tid + 1] = cnt;
            }
            __syncthreads();
            if (wave == 0) {
                constexpr int PER = PQ2_PCH / MDB_WAVE;
                uint32_t loc[PER], sum = 0;
#pragma unroll
                for (int x = 0; x < PER; ++x) { loc[x] = ppref[1 + lane * PER + x]; sum += loc[x]; }
                uint32_t incl = sum;
#pragma unroll
                for (int o = 1; o < MDB_WAVE; o <<= 1) {
                    uint32_t v = __shfl_up(incl, o);
                    if (lane >= o) incl += v;
                }
                uint32_t run = incl - sum;
#pragma unroll
                for (int x = 0; x < PER; ++x) { run += loc[x]; ppref[1 + lane * PER + x] = run; }
                if (lane == 0) ppref[0] = 0;
            }
            __syncthreads();
            const int T = (int)ppref[PQ2_PCH];
            const int per_round = PQ2_NW * nsplit;
            const int rounds = (T + per_round - 1) / per_round;
            // 3-stage software pipeline over rounds, unrolled by 3 so that no loaded register is ever
            // moved (a move would force the wait right after the issue): stage set (r % 3) is fetched in
            // iteration r (slot id + code words, unconditional loads from clamped addresses), gets its
            // tombstone word in iteration r+1 and is consumed in iteration r+2.
            uint32_t pid[3], tw[3], aw[3], cw[3][MW];
            bool live[3] = {false, false, false};  // wave-uniform: the set holds a real tile
            int jsafe = 0;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                pid[x] = 0xFFFFFFFFu;
                tw[x] = 0;
                aw[x] = 0;
#pragma unroll
                for (int w = 0; w < MW; ++w) cw[x][w] = 0;
            }
            auto iteration = [&](int r, auto PH) {
                constexpr int FA = decltype(PH)::value, TB = (FA + 2) % 3, CC = (FA + 1) % 3;
                // ---- issue (branch-free, so that the compiler's vmcnt bookkeeping stays exact): fetch
                // round r into set FA; a wave without a tile reads tile 0 of the sequence and is marked dead
                {
                    int t = (r * nsplit + split) * PQ2_NW + wave;
                    int j = 0;  // number of lists that end at or before t
                    if (n <= MDB_WAVE) {  // (the usual probe counts: one ballot instead of eight — entries past n hold T > t)
                        j = __popcll(__ballot(ppref[lane + 1] <= (uint32_t)t));
                    } else {
#pragma unroll
                        for (int x = 0; x < PQ2_PCH / MDB_WAVE; ++x)
                            j += __popcll(__ballot(ppref[x * MDB_WAVE + lane + 1] <= (uint32_t)t));
                    }
                    live[FA] = r < rounds && t < T;  // then j < n: unused entries have prefix == T > t
                    j = live[FA] ? j : jsafe;
                    uint32_t tile = pstart[j] + (live[FA] ? (uint32_t)t - ppref[j] : 0u);
                    pid[FA] = a.slot_ids[(size_t)tile * MDB_TILE + lane];
                    const uint32_t* cwp = codes + (size_t)tile * MW * MDB_TILE + lane;
#pragma unroll
                    for (int w = 0; w < MW; ++w) cw[FA][w] = cwp[(size_t)w * MDB_TILE];
                }
                // ---- issue: tombstone word of round r-1 (set TB); padding slots read word 0
                {
                    uint32_t pz = pid[TB] == 0xFFFFFFFFu ? 0u : pid[TB];
                    tw[TB] = a.tomb[u.tomb_base + (pz >> 5)];
                    aw[TB] = a.allow[(size_t)qi * a.allow_stride + ((pz >> 5) & a.allow_mask)];
                }
                // ---- compute round r-2 (set CC)
                if (r >= 2) {
                    uint64_t key = MDB_KEY_MAX;
                    const bool take = live[CC] && pid[CC] != 0xFFFFFFFFu && !((tw[CC] >> (pid[CC] & 31)) & 1u) && ((aw[CC] >> (pid[CC] & 31)) & 1u);
                    if (FILT) {
                        // bound filter: only vectors whose lower bound does not exceed the admission threshold are
                        // evaluated exactly — later, from a wave-wide pending set in registers (compacted by a
                        // forward lane permute), so that the exact pass runs with (nearly) all lanes busy
                        bool surv = false;
                        if (take) {
                            ++scored;
                            float lb = 0.0f;
#pragma unroll
                            for (int w = 0; w < MW; ++w) {
#pragma unroll
                                for (int bi = 0; bi < 4; ++bi) {
                                    const int s = w * 4 + bi;
                                    if (s < m) {
                                        const uint32_t code = (cw[CC][w] >> (8 * bi)) & 0xFFu;
                                        lb = __fadd_rn(lb, __uint_as_float((uint32_t)atab[(s << nbits) + code] << 16));
                                    }
                                }
                            }
                            // a NaN bound (NaN term) always survives: the exact pass reports it
                            const uint32_t thr_hi = (uint32_t)(*sel.thr >> 32);
                            surv = !(lb == lb && f32_orderable(__fmul_rn(lb, 0.99998f)) > thr_hi);
                        }
                        const unsigned long long sm = __ballot(surv);
                        const int ns = __popcll(sm);
                        if (ns) {
                            bool flushed = false;
                            if (pend_n + ns > MDB_WAVE) {
                                key = exact_key(pend_pid, pend_cw, lane < pend_n);
                                pend_n = 0;
                                flushed = true;
                            }
                            const int dest = surv ? pend_n + __popcll(sm & ((1ull << lane) - 1ull)) : (pend_n + ns) & (MDB_WAVE - 1);
                            const uint32_t rp = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)pid[CC]);
                            const bool got = lane >= pend_n && lane < pend_n + ns;
                            pend_pid = got ? rp : pend_pid;
#pragma unroll
                            for (int w = 0; w < MW; ++w) {
                                const uint32_t rc = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)cw[CC][w]);
                                pend_cw[w] = got ? rc : pend_cw[w];
                            }
                            pend_n += ns;
                            if (!flushed && pend_n == MDB_WAVE) {
                                key = exact_key(pend_pid, pend_cw, true);
                                pend_n = 0;
                            }
                        }
                    } else if (take) {
                        key = exact_key(pid[CC], cw[CC], true);
                        ++scored;
                    }
                    if (p0 == 0 && r == 2) sel.warm_start(key);
                    sel.offer(key);
                    sel.round_end(FILT && eager_trim ? (uint32_t)a.k + 64u : 0xFFFFFFFFu);
                }
            };
            if (T > 0) {
                int j0 = 0;  // first non-empty list of the chunk: a safe tile for idle waves
#pragma unroll
                for (int x = 0; x < PQ2_PCH / MDB_WAVE; ++x) j0 += __popcll(__ballot(ppref[x * MDB_WAVE + lane + 1] == 0u));
                jsafe = j0;
                for (int r = 0; r < rounds + 2; r += 3) {  // surplus iterations offer nothing (uniform)
                    iteration(r, std::integral_constant<int, 0>{});
                    iteration(r + 1, std::integral_constant<int, 1>{});
                    iteration(r + 2, std::integral_constant<int, 2>{});
                }
            }
            __syncthreads();  // pstart / ppref are rewritten by the next chunk
        }
        if (FILT) {  // the survivors still pending
            sel.offer(exact_key(pend_pid, pend_cw, lane < pend_n));
            sel.round_end();
        }
    }
    if (nan_seen) atomicOr(a.flags, MDB_FLAG_NAN);
    if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
    {
        unsigned long long ws = scored;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ws += __shfl_xor((unsigned)ws, o);
        // one device-scope atomic per BLOCK (wave totals meet in LDS first): thousands of atomics on one cache
        // line serialise and were the largest fixed cost of a scan block
        if (lane == 0 && ws) atomicAdd(sel.spare(), (uint32_t)ws);
    }
    sel.finish();
    if (threadIdx.x == 0 && *sel.spare() && !a.gate) atomicAdd(&a.counters[2], (unsigned long long)*sel.spare());
    uint64_t* dst = a.partial + ((size_t)qi * nsplit + split) * a.k;
    uint32_t c = sel.count();
    for (int j = tid; j < a.k; j += PQ2_BLOCK) dst[j] = j < (int)c ? sel.buf[j] : MDB_KEY_MAX;
    if (a.counts_out && tid == 0) a.counts_out[qi] = c;
}

// ------------------------------------------------------------------------------------------
// PQ posting-list scan in TWO PHASES (L2, k <= 64): bounds first, exact distances for the few vectors that can matter.
// The one-phase kernel above is pinned to one block per CU by its 128 KB per-element table, and its waves spend 62 % of
// their time waiting (PMC).  Only ROW SUMS are needed to decide which vectors can enter the top-k:
//   phase 1 (ivf_scan_pq3_kernel): per (subspace, code) the block keeps ONE word — a bf16 lower bound and a bf16 upper bound of
//     the row's sum (16 KB in all: two 1024-thread blocks per CU, no table build).  For every scanned vector it adds up both;
//     the upper bounds feed a BlockSelect, whose k-th smallest U bounds the k-th exact distance from above (k vectors have
//     exact <= upper <= U); a vector whose LOWER bound exceeds U can never be in the top-k, every other one is a CANDIDATE:
//     its slot index goes to the (query, split) list.  With 8-bit mantissas the two bounds are 0.8 % apart, so little more
//     than the top-k itself survives once U has settled (warm start: the first round sets U).
//   phase 2 (ivf_pq3_refine_kernel): one block per query evaluates the candidates EXACTLY — the same per-element terms in the
//     same association as the table kernel, rows taken from the codebook in L2 — and selects the top-k: identical keys.
// A list that outgrows its capacity raises `ovf`; the one-phase kernel, launched behind it and gated on that word, then redoes
// the batch (both launches return at once otherwise).
// Row-sum table of the codebook against itself: sdc[s][a][c] = the f32 sum, in ivf_scan_pq3_kernel's own association, of the
// per-element terms of code a against code c in subspace s.  MuopDB's PQ distance is SYMMETRIC (the query is quantized too,
// quantization/pq.rs), so the 4 m K words a scan block needs are m rows of this table — a 16 KB copy out of L2 instead of 128 KB of
// codebook reads and 32 K term evaluations per block: on a C5 shard (12 K scanned vectors per query) the build was a third of the
// scan kernel.  Same arithmetic, same bits.
__global__ void pq_sdc_kernel(const float* __restrict__ cb, int m, int K, int subdim, float* __restrict__ sdc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)m * K * K;
    if (i >= total) return;
    const size_t c = i % K, a = (i / K) % K, s = i / ((size_t)K * K);
    const float* row = cb + (s * K + c) * subdim;
    const float* q = cb + (s * K + a) * subdim;
    float sum = 0.0f;
    for (int e = 0; e < subdim; ++e) sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q[e], row[e]));
    sdc[i] = sum;
}

struct Pq3Args {
    uint32_t* cand;       // [B][nsplit][cap] records of 1 + MW words: point id, the vector's code words (phase 2 makes no trip to the lists)
    uint32_t* cand_cnt;   // [B][nsplit]
    uint32_t cap;
    uint32_t* ovf;
};

template <int MW, int BLK, bool FULL>   // FULL: as in ivf_scan_pq2_kernel
__global__ __launch_bounds__(BLK) void ivf_scan_pq3_kernel(ScanArgs a, const uint32_t* __restrict__ codes, int m_rt, int nbits_rt, int subdim,
                                                                 const float* __restrict__ cb, const uint8_t* __restrict__ qcodes, Pq3Args c3,
                                                                 const float* __restrict__ sdc) {
    const int m = FULL ? 4 * MW : m_rt, nbits = FULL ? 8 : nbits_rt;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    BlockSelect<BLK> sel;
    sel.init(lds, a.k);
    uint32_t* pstart = (uint32_t*)(lds + ((BlockSelect<BLK>::lds_bytes(a.k) + 15) & ~(size_t)15));
    uint32_t* ppref = pstart + PQ2_PCH;
    uint32_t* ccnt = ppref + PQ2_PCH + 8;            // candidates of this block
    float* qv = (float*)(ppref + PQ2_PCH + 16);      // the query's own codebook rows [m][subdim]
    uint32_t* btab = (uint32_t*)(qv + m * subdim);   // [m << nbits]: the f32 sum of the row (as bits)
    const int qi = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid / MDB_WAVE), lane = tid % MDB_WAVE;
    const IvfUserDev u = a.users[a.q_user ? a.q_user[qi] : 0];
    const uint8_t* qc = qcodes + (size_t)qi * m;
    const int np = a.probe_cnt ? (int)a.probe_cnt[qi] : a.probe_stride;
    const int K = 1 << nbits;
    bool bad = false;
    unsigned scored = 0;
    uint32_t* const my_cand = c3.cand + ((size_t)qi * nsplit + split) * c3.cap * (1 + MW);
    const float gmar = 1.5f * (float)(m * subdim + m + subdim + 16) * 5.9604645e-8f;   // the bracket's relative half width (below)
    const float lo_f = 1.0f - gmar, hi_f = 1.0f + gmar;
    const int sel_mask = (a.eager_trim & 0xFF) >= 2 ? 0 : 7;   // MDB_PQ_EAGER_TRIM=2: the selector on every round (round 2's scan)
    const int sel_warm = 2 + ((a.eager_trim >> 8) & 0xFF);    // the selector's first rounds (MDB_PQ3_WARM_ROUNDS; r counts from the pipeline's fill)
    if (tid == 0) *ccnt = 0;
    if (sdc) {   // the query's rows of the code-to-code table (pq_sdc_kernel: the words the loop below computes)
        for (int i = tid; i < (m << nbits); i += BLK) btab[i] = __float_as_uint(sdc[((size_t)(i >> nbits) * K + qc[i >> nbits]) * K + (i & (K - 1))]);
    } else {
    for (int i = tid; i < m * subdim; i += BLK) {
        int s = i / subdim;
        qv[i] = cb[((size_t)s * K + qc[s]) * subdim + (i % subdim)];
    }
    __syncthreads();
    for (int i = tid; i < (m << nbits); i += BLK) {
        const float* row = cb + (size_t)i * subdim;
        const float* q = qv + (i >> nbits) * subdim;
        float sum = 0.0f;
        for (int e = 0; e < subdim; ++e) sum = __fadd_rn(sum, acc_term<MDB_METRIC_L2>(0.0f, q[e], row[e]));   // every term >= 0
        // ONE f32 word per (subspace, code): the row's sum itself.  It is within (1 +- (subdim + 2) eps) of the real row sum, the
        // scan's running total of m such words within (1 +- m eps) of theirs, and the exact distance (the same terms in the
        // reference's association) within (1 +- m subdim eps) of the real total: every term is >= 0, so the errors stay relative
        // and the bracket is  S (1 - g) <= exact <= S (1 + g),  g = 1.5 (m subdim + m + subdim + 16) eps  (1.5e-5 at m = 16, subdim = 8).
        // (Round 2 kept a bf16 lower and a bf16 upper bound per word and added both per subspace: seven instructions per subspace
        // instead of four on a VALU-bound scan, and brackets 0.8 % wide instead of 6e-5.)
        btab[i] = __float_as_uint(sum);
    }
    }
    __syncthreads();

    if (u.valid) {
        for (int p0 = 0; p0 < np; p0 += PQ2_PCH) {
            const int n = min(PQ2_PCH, np - p0);
            for (int e = tid; e < PQ2_PCH; e += BLK) {
                uint32_t t0 = 0, cnt = 0;
                if (e < n) {
                    uint32_t c = a.probes[(size_t)qi * a.probe_stride + p0 + e];
                    if (c >= u.num_lists) bad = true;
                    else {
                        uint32_t g = u.list_base + c;
                        t0 = a.list_tile_off[g];
                        cnt = a.list_tile_off[g + 1] - t0;
                    }
                }
                pstart[e] = t0;
                ppref[e + 1] = cnt;
            }
            __syncthreads();
            if (wave == 0) {
                constexpr int PER = PQ2_PCH / MDB_WAVE;
                uint32_t loc[PER], sum = 0;
#pragma unroll
                for (int x = 0; x < PER; ++x) { loc[x] = ppref[1 + lane * PER + x]; sum += loc[x]; }
                uint32_t incl = sum;
#pragma unroll
                for (int o = 1; o < MDB_WAVE; o <<= 1) {
                    uint32_t v = __shfl_up(incl, o);
                    if (lane >= o) incl += v;
                }
                uint32_t run = incl - sum;
#pragma unroll
                for (int x = 0; x < PER; ++x) { run += loc[x]; ppref[1 + lane * PER + x] = run; }
                if (lane == 0) ppref[0] = 0;
            }
            __syncthreads();
            const int T = (int)ppref[PQ2_PCH];
            constexpr int NW = BLK / MDB_WAVE;
            const int per_round = NW * nsplit;
            const int rounds = (T + per_round - 1) / per_round;
            // the same 3-stage pipeline as the one-phase kernel (fetch / tombstone word / consume)
            uint32_t pid[3], tw[3], aw[3], cw[3][MW], slot0[3];
            bool live[3] = {false, false, false};
            int jsafe = 0;
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                pid[x] = 0xFFFFFFFFu; tw[x] = 0; aw[x] = 0; slot0[x] = 0;
#pragma unroll
                for (int w = 0; w < MW; ++w) cw[x][w] = 0;
            }
            auto iteration = [&](int r, auto PH) {
                constexpr int FA = decltype(PH)::value, TB = (FA + 2) % 3, CC = (FA + 1) % 3;
                {
                    int t = (r * nsplit + split) * NW + wave;
                    int j = 0;
                    if (n <= MDB_WAVE) {
                        j = __popcll(__ballot(ppref[lane + 1] <= (uint32_t)t));
                    } else {
#pragma unroll
                        for (int x = 0; x < PQ2_PCH / MDB_WAVE; ++x)
                            j += __popcll(__ballot(ppref[x * MDB_WAVE + lane + 1] <= (uint32_t)t));
                    }
                    live[FA] = r < rounds && t < T;
                    j = live[FA] ? j : jsafe;
                    uint32_t tile = pstart[j] + (live[FA] ? (uint32_t)t - ppref[j] : 0u);
                    slot0[FA] = tile * MDB_TILE;
                    pid[FA] = a.slot_ids[(size_t)tile * MDB_TILE + lane];
                    const uint32_t* cwp = codes + (size_t)tile * MW * MDB_TILE + lane;
#pragma unroll
                    for (int w = 0; w < MW; ++w) cw[FA][w] = cwp[(size_t)w * MDB_TILE];
                }
                if (!a.no_masks) {   // (launch-uniform) two gathers per tile that an index nobody invalidated, searched without a filter, never needs
                    uint32_t pz = pid[TB] == 0xFFFFFFFFu ? 0u : pid[TB];
                    tw[TB] = a.tomb[u.tomb_base + (pz >> 5)];
                    aw[TB] = a.allow[(size_t)qi * a.allow_stride + ((pz >> 5) & a.allow_mask)];
                } else {
                    tw[TB] = 0u;
                    aw[TB] = 0xFFFFFFFFu;
                }
                if (r >= 2) {
                    uint64_t key = MDB_KEY_MAX;
                    const bool take = live[CC] && pid[CC] != 0xFFFFFFFFu && !((tw[CC] >> (pid[CC] & 31)) & 1u) && ((aw[CC] >> (pid[CC] & 31)) & 1u);
                    float lb = 0.0f;
                    if (take) {
                        ++scored;
                        float tot = 0.0f;
#pragma unroll
                        for (int w = 0; w < MW; ++w) {
#pragma unroll
                            for (int bi = 0; bi < 4; ++bi) {
                                const int s = w * 4 + bi;
                                if (s < m) {
                                    const uint32_t code = (cw[CC][w] >> (8 * bi)) & 0xFFu;
                                    tot = __fadd_rn(tot, __uint_as_float(btab[(s << nbits) + code]));
                                }
                            }
                        }
                        lb = __fmul_rn(tot, lo_f);
                        key = make_key(__fmul_rn(tot, hi_f), pid[CC]);   // NaN sorts last: it never lowers the threshold
                    }
                    if (p0 == 0 && r == 2) sel.warm_start(key);
                    // candidates against the threshold as it stands (it only tightens: a vector admitted early is merely superfluous)
                    const uint32_t thr_hi = (uint32_t)(*sel.thr >> 32);
                    const bool surv = take && !(lb == lb && f32_orderable(lb) > thr_hi);
                    const unsigned long long sm = __ballot(surv);
                    if (sm) {
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(ccnt, (uint32_t)__popcll(sm));
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                        const uint32_t pos = base + (uint32_t)__popcll(sm & ((1ull << lane) - 1ull));
                        if (surv && pos < c3.cap) {   // the record phase 2 evaluates: no second, scattered trip to slot ids and code tiles
                            my_cand[pos * (1 + MW)] = pid[CC];
#pragma unroll
                            for (int w = 0; w < MW; ++w) my_cand[pos * (1 + MW) + 1 + w] = cw[CC][w];
                        }
                    }
                    // The selector only has to supply A bound of the k-th distance, and any k upper bounds seen so far do: it runs on
                    // the first rounds (MDB_PQ3_WARM_ROUNDS, 4: the nearest probed lists come first in the tile sequence, the bound
                    // is nearly final after them) and on every eighth round after that — its block barrier per round cost 17 % of
                    // this kernel for 5 % fewer candidates.  (Round 4, a C5 share at 30 M rows: 8 / 6 / 4 / 3 / 2 first rounds ->
                    // scan + refine 218 / 211 / 207 / 203 / 204 us; the whole index: no difference.)
                    if (r < sel_warm || ((r - 2) & sel_mask) == 0) {   // block-uniform
                        sel.offer(key);
                        sel.round_end((uint32_t)a.k + 64u);   // eager: a slack threshold costs phase 2 exact evaluations
                    }
                }
            };
            if (T > 0) {
                int j0 = 0;
#pragma unroll
                for (int x = 0; x < PQ2_PCH / MDB_WAVE; ++x) j0 += __popcll(__ballot(ppref[x * MDB_WAVE + lane + 1] == 0u));
                jsafe = j0;
                for (int r = 0; r < rounds + 2; r += 3) {
                    iteration(r, std::integral_constant<int, 0>{});
                    iteration(r + 1, std::integral_constant<int, 1>{});
                    iteration(r + 2, std::integral_constant<int, 2>{});
                }
            }
            __syncthreads();
        }
    }
    if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
    {
        unsigned long long ws = scored;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ws += __shfl_xor((unsigned)ws, o);
        if (lane == 0 && ws) atomicAdd(sel.spare(), (uint32_t)ws);
    }
    __syncthreads();
    if (tid == 0) {
        if (*sel.spare()) atomicAdd(&a.counters[2], (unsigned long long)*sel.spare());
        const uint32_t c = *ccnt;
        c3.cand_cnt[(size_t)qi * nsplit + split] = min(c, c3.cap);
        if (c > c3.cap) atomicAdd(c3.ovf, 1u);
    }
}

// phase 2: exact symmetric distances of a query's candidates (all splits), top-k -> the final key rows
template <int SUBDIM, int MW, bool FULL>
__global__ __launch_bounds__(256) void ivf_pq3_refine_kernel(ScanArgs a, const uint32_t* __restrict__ codes, int m_rt, int nbits_rt,
                                                             const float* __restrict__ cb, const uint8_t* __restrict__ qcodes, Pq3Args c3,
                                                             int nsplit) {
    const int m = FULL ? 4 * MW : m_rt, nbits = FULL ? 8 : nbits_rt;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    BlockSelect<256> sel;
    sel.init(lds, a.k);
    float* qv = (float*)(lds + ((BlockSelect<256>::lds_bytes(a.k) + 15) & ~(size_t)15));
    const int qi = blockIdx.x, tid = threadIdx.x;
    const uint8_t* qc = qcodes + (size_t)qi * m;
    const int K = 1 << nbits;
    constexpr int S4 = SUBDIM / 4;
    for (int i = tid; i < m * SUBDIM; i += 256) {
        int s = i / SUBDIM;
        qv[i] = cb[((size_t)s * K + qc[s]) * SUBDIM + (i % SUBDIM)];
    }
    __syncthreads();
    bool nan_seen = false, first = true;
    for (int sp = 0; sp < nsplit; ++sp) {
        const uint32_t c = c3.cand_cnt[(size_t)qi * nsplit + sp];
        const uint32_t* __restrict__ list = c3.cand + ((size_t)qi * nsplit + sp) * c3.cap * (1 + MW);
        for (uint32_t base = 0; base < c; base += 256) {
            const uint32_t i = base + tid;
            uint64_t key = MDB_KEY_MAX;
            if (i < c) {
                const uint32_t* rec = list + (size_t)i * (1 + MW);
                const uint32_t vid = rec[0];
                float s16[16], s8[8], s4[4];
#pragma unroll
                for (int x = 0; x < 16; ++x) s16[x] = 0.0f;
#pragma unroll
                for (int x = 0; x < 8; ++x) s8[x] = 0.0f;
#pragma unroll
                for (int x = 0; x < 4; ++x) s4[x] = 0.0f;
#pragma unroll
                for (int w = 0; w < MW; ++w) {
                    const uint32_t word = rec[1 + w];
#pragma unroll
                    for (int bi = 0; bi < 4; ++bi) {
                        const int s = w * 4 + bi;
                        if (s < m) {
                            const uint32_t code = (word >> (8 * bi)) & 0xFFu;
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
                }
                const float rs = __fadd_rn(__fadd_rn(__fadd_rn(reduce_ordered<16>(s16), reduce_ordered<8>(s8)), reduce_ordered<4>(s4)), 0.0f);
                if (rs != rs) nan_seen = true;
                key = make_key(rs, vid);
            }
            if (first) { sel.warm_start(key); first = false; }
            sel.offer(key);
            sel.round_end();
        }
    }
    if (nan_seen) atomicOr(a.flags, MDB_FLAG_NAN);
    sel.finish();
    uint64_t* dst = a.partial + (size_t)qi * a.k;
    const uint32_t c = sel.count();
    for (int j = tid; j < a.k; j += 256) dst[j] = j < (int)c ? sel.buf[j] : MDB_KEY_MAX;
    if (a.counts_out && tid == 0) a.counts_out[qi] = c;
}

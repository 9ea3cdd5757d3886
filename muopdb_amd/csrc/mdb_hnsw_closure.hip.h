// mdb_hnsw_closure.hip.h — the upper layers of BlockBasedHnsw::ann_search (hnsw/block_based/index.rs:159-190, search_layer :212-287)
// expanded FRONTIER BY FRONTIER by the whole block.  Included by mdb_hnsw_upper.hip behind HnswUpArgs and mdb_hnsw_rank.hip.h.
//
// Every distance a layer >= 1 can ask for is in the table row T[q][.] before its traversal starts, and everything the layer hands on
// is a union, a count or a minimum: the visited set, the evaluations (points newly visited), the expansions (expanded points with a
// non-empty row) and the nearest evaluated point.  Let theta be the ef-th smallest canonical image of the row (index ef - 1 of the
// sorted row; +inf for a set of <= ef points) and call a point CERTAIN when d < theta.  At most ef - 2 other points are as near as a
// certain point c, so
//   * c is accepted whenever it is discovered (`|W| < ef or d < furthest` cannot fail), and is never evicted;
//   * the `distance > furthest` break cannot fire when c is popped, nor on anything popped while c is pending (the minimum
//     candidate is no farther than c).
// Every certain point that is discovered WILL be expanded, in whatever order: so the block expands all of them, whole frontiers per
// round (a group of lanes per frontier point, one lane per edge), until none is left; then it takes the one minimum unexpanded
// evaluated point u (smallest image, largest id among ties: the candidates heap's order) and restates the reference's stop test as
// counts over the evaluated set: #{d < d_u} >= ef: the layer is done; else u is expanded alone and the rounds resume.  Points the
// reference rejected at discovery stay in the evaluated set as pseudo-candidates: when one becomes the minimum it fails the count,
// and so does every true candidate behind it.  theta of a SUPERSET of the layer's points is no larger than the layer's own, so it is
// valid too, only less useful: one select over the launch's row serves its lowest layer, one over the TOP set the layers >= 2 (the
// split path's top launch numbers exactly that set; a launch over every upper layer reaches it through map21).
// hnsw_upper_kernel's closure of a layer of <= 64 points is the special case theta = +inf.
// What the counts cannot decide is an uncertain u that passes the strict test while ef OTHER evaluated points are no farther: whether
// the reference ever accepted u depends on the discovery order.  That, and any evaluated NaN (whose flag the sequential kernels raise
// where the reference panics), makes the query a FALLBACK: the block publishes nothing (its visited set is a copy in LDS) and the
// sequential traversal re-runs what the block ran, no more (tests/closure_model.py restates both forms; tests/test_gpu_hnsw_closure.py,
// test_gpu_hnsw_closure_local.py):
//   * a TOP block of the split path (CL_ROLE_TOP_LOCAL) re-runs its layers >= 2 itself, on sorted positions: the row is carried over
//     to the layout of mdb_hnsw_rank.hip.h, rank_tables + upper_traverse_rank1 publish the hand-over the sequential top launch has
//     always given layer 1 (NaN word included), and fb[q] = CL_FB_COUNT asks the layer-1 launch to count the query — the top launch
//     is the one that clears the counter words.  The layer-1 launch then runs the query like any other;
//   * a query flagged on layer 1 (or handed a NaN word or an overflow flag from above) sets fb[q] = CL_FB_RERUN, and a follow-up
//     launch of the sequential kernels, whose blocks exit at once unless their query's word says so, re-runs LAYER 1 from the top
//     launch's hand-over, which is still intact;
//   * where the top block cannot hold the sorted-position layout (more than 2048 TOP points, MDB_HNSW_RANK bit 1 clear) and in a
//     launch over every upper layer (CL_ROLE_SINGLE: batches below the split path) the protocol is the first one built: fb[q] =
//     CL_FB_RERUN from whichever launch flags, a query flagged above is skipped on layer 1, the follow-up launch starts at the top.
// mdb_hnsw_closure_fallbacks counts a query once, wherever it was flagged; every call writes fb[q] of each of its queries before it
// reads it (the words live in scratch that is reused).
// The form adds no kernel of its own: it is a mode of the launches it replaces — the 1024-thread hnsw_upper_rank_kernel behind the table
// (one block per CU either way: its LDS holds the query's table row) and the top blocks of hnsw_upper_top_rank_kernel — chosen by
// HnswUpArgs::fb_role, so the launch shape, the table blocks and the kernel inventory stay what they were.
#pragma once

// (CL_FR_CAP, CL_SUBHIST, CL_SH_WORDS and cl_lds_words: mdb_hnsw_route.h)
// shared words of the block
#define CL_SH_NNEXT 0            // [2] length of the next frontier, by round parity
#define CL_SH_EVALS 2
#define CL_SH_EXPANDED 3
#define CL_SH_HAZARD 4
#define CL_SH_LT 5
#define CL_SH_LE 6
#define CL_SH_DIGIT 7
#define CL_SH_K 8
#define CL_SH_KMIN 9
#define CL_SH_KMAX 10
#define CL_SH_MINU 12            // u64: min (image, ~id) over evaluated and unexpanded
#define CL_SH_MINE 14            // u64: min (image, id) over evaluated
#define CL_SH_FLAGGED 16         // how closure_traverse ended, for its caller
struct ClLds {
    uint32_t *sh, *hist, *fr, *vis, *ev, *ex, *vis_out, *row;
};
// (every part a multiple of four words: the row's copy is written with 16-byte stores)
__device__ __forceinline__ ClLds cl_carve(uint32_t* p, uint32_t vis_words, uint32_t out_words) {
    ClLds L;
    L.sh = p; p += CL_SH_WORDS;
    L.hist = p; p += CL_SUBHIST * 256;
    L.fr = p; p += 2 * CL_FR_CAP;
    L.vis = p; p += vis_words;
    L.ev = p; p += vis_words;
    L.ex = p; p += vis_words;
    L.vis_out = p; p += out_words;
    L.row = p;
    return L;
}

__device__ __forceinline__ uint64_t cl_wave_min_u64(uint64_t v) {
    const uint32_t hi = wave_min_u32((uint32_t)(v >> 32));
    const uint32_t lo = wave_min_u32((uint32_t)(v >> 32) == hi ? (uint32_t)v : 0xFFFFFFFFu);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t cl_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// theta: the canonical image at index ef - 1 of the sorted keys[0 .. n) (0xFFFFFFFF = +inf when n <= ef).  Exact block-wide radix
// select, most significant digit first, over the bits the row's key range has; a NaN sorts last (rk_canon).  idx != nullptr: over
// keys[idx[0 .. n)] (the TOP set inside the row of all upper points).  Called by every thread.
template <int NT>
__device__ __forceinline__ uint32_t cl_theta(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, const uint32_t n, const uint32_t ef,
                                             uint32_t* hist, uint32_t* sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n <= ef) return 0xFFFFFFFFu;
    if (tid == 0) { sh[CL_SH_KMIN] = 0xFFFFFFFFu; sh[CL_SH_KMAX] = 0u; }
    __syncthreads();
    {
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (uint32_t i = tid; i < n; i += NT) {
            const uint32_t k = rk_canon(keys[idx ? idx[i] : i]);
            mn = min(mn, k);
            mx = max(mx, k);
        }
        mn = wave_min_u32(mn);
        mx = wave_max_u32(mx);
        if (lane == 0) { atomicMin(&sh[CL_SH_KMIN], mn); atomicMax(&sh[CL_SH_KMAX], mx); }
    }
    __syncthreads();
    const uint32_t kmin = sh[CL_SH_KMIN], range = sh[CL_SH_KMAX] - kmin;
    int hi = range ? 32 - __builtin_clz(range) : 0;   // bits [lo, hi) are decided by the next pass; the bits above them equal `prefix`
    uint32_t prefix = 0u, k = ef - 1u;
    uint32_t* const hw = hist + (wave & (CL_SUBHIST - 1)) * 256;
    while (hi > 0) {                                   // (uniform: at most four passes)
        const int lo = hi > 8 ? hi - 8 : 0;
        const uint32_t dmask = (1u << (hi - lo)) - 1u;
        for (int i = tid; i < CL_SUBHIST * 256; i += NT) hist[i] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += NT) {
            const uint32_t kp = rk_canon(keys[idx ? idx[i] : i]) - kmin;
            const uint32_t above = hi >= 32 ? 0u : kp >> hi;
            if (above == prefix) atomicAdd(&hw[(kp >> lo) & dmask], 1u);
        }
        __syncthreads();
        if (wave == 0) {                               // lane l owns digits 4 l .. 4 l + 3
            uint32_t c[4], tot = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = 0u;
#pragma unroll
                for (int s = 0; s < CL_SUBHIST; ++s) c[j] += hist[s * 256 + 4 * lane + j];
                tot += c[j];
            }
            uint32_t inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += t;
            }
            uint32_t before = inc - tot;
            if (before <= k && k < inc) {              // exactly one lane
                int j = 0;
                while (j < 3 && before + c[j] <= k) { before += c[j]; ++j; }
                sh[CL_SH_DIGIT] = 4u * lane + j;
                sh[CL_SH_K] = k - before;
            }
        }
        __syncthreads();
        prefix = (prefix << (hi - lo)) | sh[CL_SH_DIGIT];
        k = sh[CL_SH_K];
        hi = lo;
    }
    return kmin + prefix;
}

// Layers a.layer_hi .. a.layer_lo of query qi on the table row `tq` (LDS or global memory), by every thread of the block.  L.vis holds
// the visited set handed in, and the caller's barrier stands behind it and the row.  Publishes the hand-over exactly as
// upper_traverse_wave0 leaves it, or — flagged — only fb[q] (CL_ROLE_TOP_LOCAL: nothing at all; the caller resolves the flag).
// Returns the flag, the same for every thread: read back from an LDS word, so that the compiler knows it.
template <int NT>
__device__ __forceinline__ bool closure_traverse(const HnswUpArgs& a, const int qi, const ClLds& L, const uint32_t* __restrict__ tq) {
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t ef = (uint32_t)a.ef, su = a.su;
    uint32_t gs = 1;                                   // lanes per frontier point: the row stride rounded up to a power of two (<= 64)
    while (gs < su) gs <<= 1;
    const uint32_t per = NT / gs, slot = (uint32_t)tid % gs, sub = (uint32_t)tid / gs;
    uint64_t* const sh_minu = (uint64_t*)(L.sh + CL_SH_MINU);
    uint64_t* const sh_mine = (uint64_t*)(L.sh + CL_SH_MINE);
    const uint32_t theta = cl_theta<NT>(tq, nullptr, a.nu, ef, L.hist, L.sh);
    // one launch over every upper layer: the layers >= 2 hold the TOP set only, and theta of the whole row would leave next to none of
    // its points certain (the layer would be popped one point at a time)
    const uint32_t theta_top = (a.top_map && a.layer_hi >= 2) ? cl_theta<NT>(tq, a.top_map, a.top_n, ef, L.hist, L.sh) : theta;
    uint32_t ep = a.in_ep ? a.in_ep[qi] : a.entry_c;
    uint32_t evals = a.in_cnt ? a.in_cnt[4 * qi + 0] : 0u, expanded = a.in_cnt ? a.in_cnt[4 * qi + 1] : 0u;
    bool flagged = (a.in_cnt && a.in_cnt[4 * qi + 2]) || (a.in_ovf && a.in_ovf[qi] != 0u) || ep >= a.nu;
    uint32_t* cur = L.fr;
    uint32_t* nxt = L.fr + CL_FR_CAP;

    for (int layer = a.layer_hi; layer >= a.layer_lo && !flagged; --layer) {
        const uint32_t* const lrows = a.rows + (size_t)(layer - a.row_layer0) * a.nu * su;
        // a layer of <= 64 points with edges only among them (ef >= 64): all of it is certain, whatever the row's other points say
        const uint32_t th = ((uint32_t)layer >= a.small_layer && ef >= 64u) ? 0xFFFFFFFFu : layer >= 2 ? theta_top : theta;
        __syncthreads();
        for (uint32_t i = tid; i < a.vis_words; i += NT) { L.ev[i] = 0u; L.ex[i] = 0u; }
        if (tid == 0) { L.sh[CL_SH_NNEXT] = 0u; L.sh[CL_SH_NNEXT + 1] = 0u; L.sh[CL_SH_EVALS] = 0u; L.sh[CL_SH_EXPANDED] = 0u; L.sh[CL_SH_HAZARD] = 0u; }
        __syncthreads();
        // ---- entry point: visited, evaluated (index.rs:219-231)
        const uint32_t k0 = rk_canon(tq[ep]);
        if (k0 == RK_NAN_KEY) { flagged = true; break; }
        uint32_t ncur = k0 < th ? 1u : 0u;
        if (tid == 0) {
            L.vis[ep >> 5] |= 1u << (ep & 31);
            L.ev[ep >> 5] |= 1u << (ep & 31);
            cur[0] = ep;
        }
        __syncthreads();
        uint32_t parity = 0u;
        for (uint32_t pass = 0; pass <= a.nu + 1u; ++pass) {     // every pass expands at least one point not expanded before
            if (pass > a.nu) { flagged = true; break; }
            // ---- whole frontiers at once: every point of `cur` is expanded by `gs` lanes, lane = edge slot
            while (ncur > 0u) {
                for (uint32_t base = 0; base < ncur; base += per) {
                    const uint32_t item = base + sub;
                    const bool act = item < ncur;
                    const uint32_t f = act ? cur[item] : 0u;
                    const uint32_t nbr = (act && slot < su) ? lrows[(size_t)f * su + slot] : 0xFFFFFFFFu;
                    if (act && slot == 0u) {
                        atomicOr(&L.ex[f >> 5], 1u << (f & 31));
                        if (nbr != 0xFFFFFFFFu) atomicAdd(&L.sh[CL_SH_EXPANDED], 1u);   // rows are packed: an edge in slot 0 or none at all
                    }
                    if (nbr != 0xFFFFFFFFu) {
                        if (nbr >= a.nu) { L.sh[CL_SH_HAZARD] = 1u; continue; }
                        const uint32_t bit = 1u << (nbr & 31);
                        if (!(atomicOr(&L.vis[nbr >> 5], bit) & bit)) {   // two lanes on one point (duplicate edges): exactly one is new
                            const uint32_t kk = rk_canon(tq[nbr]);
                            atomicOr(&L.ev[nbr >> 5], bit);
                            atomicAdd(&L.sh[CL_SH_EVALS], 1u);
                            if (kk == RK_NAN_KEY) L.sh[CL_SH_HAZARD] = 1u;
                            else if (kk < th) {
                                const uint32_t pos = atomicAdd(&L.sh[CL_SH_NNEXT + parity], 1u);
                                if (pos < CL_FR_CAP) nxt[pos] = nbr;
                                else L.sh[CL_SH_HAZARD] = 1u;
                            }
                        }
                    }
                }
                __syncthreads();
                ncur = L.sh[CL_SH_NNEXT + parity];
                const bool hz = L.sh[CL_SH_HAZARD] != 0u;
                if (tid == 0) L.sh[CL_SH_NNEXT + (parity ^ 1u)] = 0u;   // (last read a round ago, behind that round's second barrier)
                __syncthreads();
                parity ^= 1u;
                uint32_t* const t = cur; cur = nxt; nxt = t;
                if (hz) { flagged = true; break; }
            }
            if (flagged) break;
            // ---- the one minimum unexpanded evaluated point, and the layer's nearest evaluated point so far
            if (tid == 0) { *sh_minu = MDB_KEY_MAX; *sh_mine = MDB_KEY_MAX; L.sh[CL_SH_LT] = 0u; L.sh[CL_SH_LE] = 0u; }
            __syncthreads();
            {
                uint64_t mu = MDB_KEY_MAX, me = MDB_KEY_MAX;
                for (uint32_t w = tid; w < a.vis_words; w += NT) {
                    uint32_t be = L.ev[w];
                    const uint32_t bx = L.ex[w];
                    while (be) {
                        const uint32_t b = (uint32_t)__builtin_ctz(be);
                        be &= be - 1u;
                        const uint32_t c = 32u * w + b;
                        const uint64_t kk = (uint64_t)rk_canon(tq[c]) << 32;
                        me = min(me, kk | c);
                        if (!((bx >> b) & 1u)) mu = min(mu, kk | (uint32_t)~c);
                    }
                }
                mu = cl_wave_min_u64(mu);
                me = cl_wave_min_u64(me);
                if (lane == 0) {
                    if (mu != MDB_KEY_MAX) atomicMin((unsigned long long*)sh_minu, (unsigned long long)mu);
                    atomicMin((unsigned long long*)sh_mine, (unsigned long long)me);
                }
            }
            __syncthreads();
            const uint64_t ukey = *sh_minu;
            ep = (uint32_t)*sh_mine;                   // (smallest image, then smallest id: what the layer hands down, index.rs:177-181)
            if (ukey == MDB_KEY_MAX) break;            // nothing pending: the layer is done
            const uint32_t du = (uint32_t)(ukey >> 32), u = ~(uint32_t)ukey;
            // ---- the stop test by counting: evaluated points strictly closer than u, and no farther than u
            {
                uint32_t lt = 0u, le = 0u;
                for (uint32_t w = tid; w < a.vis_words; w += NT) {
                    uint32_t be = L.ev[w];
                    while (be) {
                        const uint32_t c = 32u * w + (uint32_t)__builtin_ctz(be);
                        be &= be - 1u;
                        const uint32_t kk = rk_canon(tq[c]);
                        lt += kk < du ? 1u : 0u;
                        le += kk <= du ? 1u : 0u;
                    }
                }
                lt = cl_wave_sum(lt);
                le = cl_wave_sum(le);
                if (lane == 0 && le) { atomicAdd(&L.sh[CL_SH_LT], lt); atomicAdd(&L.sh[CL_SH_LE], le); }
            }
            __syncthreads();
            const uint32_t lt = L.sh[CL_SH_LT], le = L.sh[CL_SH_LE];
            if (lt >= ef) break;                       // `distance > furthest.distance`: the layer is done (index.rs:246-248)
            if (le - 1u >= ef) { flagged = true; break; }   // ef others no farther than u: its acceptance hung on the discovery order
            if (tid == 0) cur[0] = u;
            ncur = 1u;
            __syncthreads();
        }
        if (flagged) break;
        evals += 1u + L.sh[CL_SH_EVALS];
        expanded += L.sh[CL_SH_EXPANDED];
    }
    __syncthreads();
    if (tid == 0) L.sh[CL_SH_FLAGGED] = flagged ? 1u : 0u;
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane((int)L.sh[CL_SH_FLAGGED]) != 0) {
        if (tid == 0 && a.fb_role != CL_ROLE_TOP_LOCAL) {
            // (a query the top launch resolved itself was counted at this block's entry: once, wherever it was flagged)
            const bool counted = a.fb_role == CL_ROLE_TOP || (a.fb_role == CL_ROLE_BOTTOM && a.fb[qi] == CL_FB_COUNT);
            a.fb[qi] = CL_FB_RERUN;
            if (!counted) atomicAdd(&a.counters[MDB_CTR_CLOSURE_FALLBACKS], 1ull);
        }
        return true;
    }
    // ---- the hand-over (see upper_traverse_wave0)
    if (a.vis_map) {
        // the next launch numbers the points differently (a superset): bit c -> bit vis_map[c]
        for (uint32_t i = tid; i < a.out_words; i += NT) L.vis_out[i] = 0u;
        __syncthreads();
        for (uint32_t w = tid; w < a.vis_words; w += NT) {
            uint32_t bits = L.vis[w];
            while (bits) {
                const uint32_t c = 32u * w + (uint32_t)__builtin_ctz(bits);
                bits &= bits - 1u;
                const uint32_t t = a.vis_map[c];
                atomicOr(&L.vis_out[t >> 5], 1u << (t & 31));
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < a.out_words; i += NT) a.out_vis[(size_t)qi * a.out_words + i] = L.vis_out[i];
    } else {
        for (uint32_t i = tid; i < a.vis_words; i += NT) a.out_vis[(size_t)qi * a.vis_words + i] = L.vis[i];
    }
    if (tid == 0) {
        a.fb[qi] = CL_FB_CLEAN;                    // (behind the top launch the word may hold CL_FB_COUNT)
        a.out_ep[qi] = a.ep_map[ep];
        a.out_ovf[qi] = 0u;
        if (a.out_cnt) {
            a.out_cnt[4 * qi + 0] = evals; a.out_cnt[4 * qi + 1] = expanded; a.out_cnt[4 * qi + 2] = 0u;
        } else {
            atomicAdd(&a.counters[0], (unsigned long long)evals);
            atomicAdd(&a.counters[1], (unsigned long long)expanded);
        }
    }
    return false;
}

// layers a.layer_hi .. a.layer_lo on the table rows of an earlier launch: the body of hnsw_upper_rank_kernel's block when the launch
// runs the frontier form (a.fb_role CL_ROLE_BOTTOM / CL_ROLE_SINGLE; declared in mdb_hnsw_rank.hip.h).  a.cl_tlds: the query's row is
// copied into LDS first (see hnsw_upper_kernel) — every lookup of the select, the rounds and the counts is then an LDS read.
template <int NT>
__device__ void closure_bottom_block(const HnswUpArgs& a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int qi = blockIdx.x;
    if (a.fb_role == CL_ROLE_BOTTOM) {
        const uint32_t above = a.fb[qi];
        if (above == CL_FB_RERUN) {                    // flagged above and left there: the follow-up launch takes it from the top
            if (threadIdx.x == 0) atomicAdd(&a.counters[MDB_CTR_CLOSURE_FALLBACKS], 1ull);
            return;
        }
        // flagged above and resolved there (the hand-over is the sequential form's): counted here, where the counter words are no
        // longer being cleared, and run like any other — thread 0 alone reads the word again should this pass flag it too
        if (above == CL_FB_COUNT && threadIdx.x == 0) atomicAdd(&a.counters[MDB_CTR_CLOSURE_FALLBACKS], 1ull);
    }
    const ClLds L = cl_carve((uint32_t*)lds, a.vis_words, a.vis_map ? a.out_words : 0u);
    const uint32_t* const tg = a.table + (size_t)qi * a.nu_pad;
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += NT) L.vis[i] = a.in_vis ? a.in_vis[(size_t)qi * a.vis_words + i] : 0u;
    if (a.cl_tlds) {
        const uint4* src = (const uint4*)tg;
        uint4* dst = (uint4*)L.row;
        for (uint32_t i = threadIdx.x; i < a.nu_pad / 4; i += NT) dst[i] = src[i];
    }
    __syncthreads();
    if (a.cl_tlds) closure_traverse<NT>(a, qi, L, L.row);   // (two copies of the traversal: its lookups are ds_read in one, global loads in the other)
    else closure_traverse<NT>(a, qi, L, tg);
}

// mdb_hnsw_closure.hip.h — the upper layers of BlockBasedHnsw::ann_search (hnsw/block_based/index.rs:159-190, search_layer :212-287)
// expanded FRONTIER BY FRONTIER by the whole block.  Included by mdb_hnsw_upper.hip behind HnswUpArgs and mdb_hnsw_rank.hip.h.
//
// Every distance a layer >= 1 can ask for is in the table row T[q][.] before its traversal starts, and everything the layer hands on
// is a union, a count or a minimum: the visited set, the evaluations (points newly visited), the expansions (expanded points with a
// non-empty row) and the nearest evaluated point.  A layer evaluates its entry point and the points it discovers that NO LAYER ABOVE
// HAS VISITED (the reference keeps one visited set per ann_search, shared by all layers; W and the candidates are per layer): its POOL
// is (the layer's points \ visited on entry) + {entry point}.  Let theta be NO LARGER than the ef-th smallest canonical image of the
// pool (index ef - 1 of the sorted pool; +inf for a pool of <= ef points) and call a point CERTAIN when d < theta.  At most ef - 2
// other points THAT THIS LAYER CAN EVALUATE are as near as a certain point c, so
//   * c is accepted whenever it is discovered (`|W| < ef or d < furthest` cannot fail), and is never evicted;
//   * the `distance > furthest` break cannot fire when c is popped, nor on anything popped while c is pending (the minimum
//     candidate is no farther than c).
// Every certain point that is discovered WILL be expanded, in whatever order: so the block expands all of them, whole frontiers per
// round (a group of lanes per frontier point, one lane per edge), until none is left; then it takes the one minimum unexpanded
// evaluated point u (smallest image, largest id among ties: the candidates heap's order) and restates the reference's stop test as
// counts over the evaluated set: #{d < d_u} >= ef: the layer is done; else u is expanded alone and the rounds resume.  Points the
// reference rejected at discovery stay in the evaluated set as pseudo-candidates: when one becomes the minimum it fails the count,
// and so does every true candidate behind it.  theta of a SUPERSET of the pool is no larger than the pool's own, so it is
// valid too, only less useful: one select over the launch's row serves its lowest layer, one over the TOP set the layers >= 2 (the
// split path's top launch numbers exactly that set; a launch over every upper layer reaches it through map21).
// hnsw_upper_kernel's closure of a layer of <= 64 points is the special case theta = +inf.
// THE POOL.  cl_theta gets the block's visited bitmap and skips every key whose bit is set, in both passes.
// A select runs LATE: at the first layer that uses it, behind that layer's entry into L.vis, so the layers above have left their visits there — and the layer's own entry point
// too, which the select therefore leaves out: it takes index ef - 2 (the (ef - 1)-th smallest) of the unvisited REST.  With the entry
// point put back that value sits at index ef - 2 or ef - 1 of the pool: never above the pool's index ef - 1, one rank conservative
// when the entry point is farther than it.  A rest of <= ef - 1 points is a pool of <= ef: +inf (the first pass's grand total is the
// rest's size).  A select is REUSED by every lower layer of the launch that uses the same set: the visited set only grows, and a lower
// layer's entry point was evaluated by the layer above it — unvisited, or the entry point, when the select ran — so every lower pool
// is a subset of rest + {that one point}, whose index ef - 1 is no smaller than the rest's index ef - 2.  On the bench the layers
// above hand layer 1 ~810 of the 977 TOP points, some six of them below the row's theta: each cost the select over the row a rank and
// the block a single pop (tests/closure_visited_model.py restates pool, rank, late select and reuse and holds chains of layers
// against closure_model.search_layer; tests/test_gpu_hnsw_closure_visited.py).
// THE COUNTED STOP TEST.  A single pop happens when the frontiers have run dry: every certain point discovered so far is expanded, so
// every pending (evaluated, unexpanded) point is uncertain and u is the nearest of them.  An evaluated point closer than u is not
// pending, hence expanded: a certain point (d < theta <= d_u) or an earlier single pop of this layer.  So
//     lt = #{evaluated, d <  d_u} = ncert + #{earlier pops p : d_p < d_u}
//     le = #{evaluated, d <= d_u} = lt + #{pending, d = d_u} + #{earlier pops p : d_p = d_u}
// with ncert = the certain points evaluated so far (the frontier lengths summed as the rounds read them, the entry point when it is
// certain), the pending ties counted by the one pass over the bitmap that finds u — each thread keeps how many of its points sit at
// its own minimum and adds them when that minimum turns out to be d_u — and the earlier pops' images kept in a list of CL_POP_CAP
// words (in `hist`, idle during the layers; wave 0 counts it).  `lt >= ef` and `le - 1 >= ef` mean what they meant.  A pop that finds
// the list full flags the query: the sequential form is exact (tests/closure_bound_model.py restates this form and holds it against
// closure_model.py's scan for every theta up to the exact one).
// THE INCREMENTAL PASS.  Between two single pops of a layer the evaluated set only grows, and the pending set loses exactly one point:
// the frontiers have run dry at a pop, so every certain point evaluated since the last pop is expanded by now and was never pending at
// a pop; an uncertain point stays pending until it is the single pop itself.  Where every thread owns at most one slice of the bitmap
// ((vis_words << ltpw) <= NT: up to 32 NT points — 8 k under the 256 threads of a top block, 32 k under the 1024 of the layer-1 block)
// it keeps, across the pops of a layer, `seen` (the bits of its slice already folded), `mu` (its minimum pending key), `mties` (its
// pending points at that image) and `me` (its minimum evaluated key), and a pop folds only ev & ~seen, skipping the expanded bits as
// before.  The thread whose slice holds the popped u forgets the slice (seen = 0, mu = max, mties = 0) and walks it again at the next
// pop, where u is expanded; ties of u in other threads' slices stay folded where they are.  So at every pop each thread's (mu, mties)
// is the minimum and the tie count over the pending points of its slice and its `me` the minimum over the evaluated ones — what the
// walk over the whole slice gives — and the block's u, lt, le, rows, counters and flags cannot depend on the change
// (tests/closure_incremental_model.py restates the bookkeeping and holds every pop against the scan).  All four values start anew at
// every layer: a layer that ends by lt >= ef leaves pending points behind, and they are not the next layer's.  With more slices
// than threads every thread walks all of its slices at every pop, as before.  Only the layer's end needs the nearest evaluated point,
// and `me` is a running minimum in either case (the evaluated set only grows): the block reduces it once, behind the layer's last pop.
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
#define CL_SH_ROWMIN 17          // smallest and largest canonical image of the row, where the caller took them while it made the row
#define CL_SH_ROWMAX 18
static_assert(CL_SH_ROWMAX < CL_SH_WORDS, "the block's shared words");
#define CL_POP_CAP 256u          // single pops of one layer whose images the block keeps (bench: 3.4 per block on layer 1, 1 in the top block)
// MDB_PIPE_DBG builds (mdb_hnsw_dev.hip.h), MDB_HNSW_DBG bit 2: the layer-1 launch, bit 3: the top launch — thread 0's cycle / event sums of the
// frontier form per call (a batch), in counters[5..15] (word 4 is the fallback counter):
//   row copy or evaluation | theta (both selects) | per layer: clear + entry point | rounds | trips inside them (count) | rounds (count) |
//   single pops: both passes | single pops that expanded (count) | hand-over | closure_traverse as a whole | blocks (count)
#define CL_DBG_ROW 1
#define CL_DBG_THETA 2
#define CL_DBG_CLEAR 3
#define CL_DBG_ROUNDS 4
#define CL_DBG_NTRIPS 5
#define CL_DBG_NROUNDS 6
#define CL_DBG_POPS 7
#define CL_DBG_NPOPS 8
#define CL_DBG_HAND 9
#define CL_DBG_TOTAL 10
#define CL_DBG_BLOCKS 11
#ifdef MDB_PIPE_DBG
#define CL_DBG_NOW() __builtin_readcyclecounter()
#define CL_DBG_FLUSH()                                                                                  \
    do {                                                                                                \
        PIPE_TE(CL_DBG_TOTAL, t_all);                                                                   \
        if (tid == 0 && a.dbg_on)                                                                       \
            for (int i = 1; i < 12; ++i) atomicAdd(&a.counters[4 + i], dbg_acc[i]);                     \
    } while (0)
#else
#define CL_DBG_NOW() 0ull
#define CL_DBG_FLUSH() do {} while (0)
#endif
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

// theta: a LOWER BOUND of the canonical image at index ef - 2 of the sorted keys[0 .. n) WHOSE BIT IN `vis` IS CLEAR (header: THE POOL;
// `vis` in the numbering of `keys`, the caller's entry point marked in it; 0xFFFFFFFF = +inf when n <= ef or when ef - 1 keys or fewer
// are left; 0 for ef < 2: no such index) — the lower edge of the histogram bin that holds that index after at most two block-wide
// passes of up to 11 bits each, most significant bits first, over the bits the row's key range has (the range of ALL n keys: a range
// over a superset is still a range; keys that are all one image give that image, whatever is left).  Exact for a range below 2^22
// images, else the bin is 2^(range bits - 22) images wide.
// What the header derives from theta is all derived from "at most ef - 2 other points are as near as a point with d < theta", which
// holds for every value up to the exact one.  A point between the bound and the exact value is uncertain instead of certain: it is
// popped alone, where the counts let it through (lt <= ef - 2) and cannot flag it (le - 1 <= ef - 2), and expanded as it would have
// been in a frontier — rows, counters and flags do not depend on the bound (tests/closure_bound_model.py), only the number of single
// pops does.  A NaN sorts last (rk_canon).  idx != nullptr: over keys[idx[0 .. n)] (the TOP set inside the row of all upper points).
// The histogram is `hist` and the two frontier lists behind it (idle outside the layers): CL_TH_WORDS = 2048 counters, one per digit;
// wave 0 scans the sums of 256 groups of 8, then the 8 words of the group that holds the index.  A pass is a block-wide scan of the
// keys with one LDS add per key: its cost is the passes times the keys per thread, which is why there are two and not five.
// have_mm: the keys' minimum and maximum are in sh[CL_SH_ROWMIN / _ROWMAX] (closure_traverse puts them there at its entry, from what
// the caller folded into the pass that produced the row).  Called by every thread.
#define CL_TH_WORDS (CL_SUBHIST * 256 + 2 * CL_FR_CAP)
static_assert(CL_TH_WORDS == 2048 && CL_TH_WORDS % 4 == 0, "cl_theta: 256 groups of 8 words, cleared with 16-byte stores");
static_assert(CL_POP_CAP <= CL_SUBHIST * 256, "the single pops' images live in hist");
template <int NT>
__device__ __forceinline__ uint32_t cl_theta(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ idx, const uint32_t n, const uint32_t ef,
                                             const uint32_t* vis, uint32_t* hist, uint32_t* sh, const bool have_mm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n <= ef) return 0xFFFFFFFFu;
    if (ef < 2u) return 0u;                            // (no rank ef - 2: nothing is certain, every point is popped alone)
    uint32_t kmin, range;
    if (!have_mm && tid == 0) { sh[CL_SH_KMIN] = 0xFFFFFFFFu; sh[CL_SH_KMAX] = 0u; }
    for (int i = tid; i < CL_TH_WORDS / 4; i += NT) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (have_mm) {                                     // closure_traverse reduced the caller's shares at its entry
        kmin = sh[CL_SH_ROWMIN];
        range = sh[CL_SH_ROWMAX] - kmin;
    } else {                                           // over the whole set: a range over a superset of the pool is still a range
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (uint32_t i = tid; i < n; i += NT) {
            const uint32_t k = rk_canon(keys[idx ? idx[i] : i]);
            mn = min(mn, k);
            mx = max(mx, k);
        }
        mn = wave_min_u32(mn);
        mx = wave_max_u32(mx);
        if (lane == 0) { atomicMin(&sh[CL_SH_KMIN], mn); atomicMax(&sh[CL_SH_KMAX], mx); }
        __syncthreads();
        kmin = sh[CL_SH_KMIN];
        range = sh[CL_SH_KMAX] - kmin;
    }
    int hi = range ? 32 - __builtin_clz(range) : 0;   // bits [lo, hi) are decided by the next pass; the bits above them equal `prefix`
    if (hi == 0 && !have_mm) __syncthreads();          // (no pass: the words just read are written again by the next select)
    uint32_t prefix = 0u, k = ef - 2u;
    for (int pass = 0; pass < 2 && hi > 0; ++pass) {   // (uniform)
        const int bits = min(hi, 11), lo = hi - bits;
        const uint32_t dmask = (1u << bits) - 1u;
        if (pass) {
            for (int i = tid; i < CL_TH_WORDS / 4; i += NT) ((uint4*)hist)[i] = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
        }
        for (uint32_t i = tid; i < n; i += NT) {
            const uint32_t c = idx ? idx[i] : i;
            if ((vis[c >> 5] >> (c & 31)) & 1u) continue;   // visited on a layer above (or this layer's entry point): not in the pool
            const uint32_t kp = rk_canon(keys[c]) - kmin;
            const uint32_t above = hi >= 32 ? 0u : kp >> hi;
            if (above == prefix) atomicAdd(&hist[(kp >> lo) & dmask], 1u);
        }
        __syncthreads();
        if (wave == 0) {                               // lane l owns the groups 4 l .. 4 l + 3
            uint32_t c[4], tot = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 x = ((const uint4*)hist)[2 * (4 * lane + j)], y = ((const uint4*)hist)[2 * (4 * lane + j) + 1];
                c[j] = x.x + x.y + x.z + x.w + y.x + y.y + y.z + y.w;
                tot += c[j];
            }
            uint32_t inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
                if (lane >= o) inc += t;
            }
            uint32_t before = inc - tot;
            // the first pass's grand total is the pool's size: ef - 1 unvisited points or fewer leave the layer <= ef points to evaluate
            const uint32_t pool = (uint32_t)__shfl((int)inc, 63, 64);
            if (pass == 0 && pool <= ef - 1u) {
                if (lane == 0) sh[CL_SH_DIGIT] = 0xFFFFFFFFu;
            } else if (before <= k && k < inc) {       // exactly one lane
                int j = 0;
                while (j < 3 && before + c[j] <= k) { before += c[j]; ++j; }
                const uint32_t* const g = hist + 8u * (4u * lane + j);   // the word inside the group
                uint32_t w = 0u;
                while (w < 7u && before + g[w] <= k) { before += g[w]; ++w; }
                sh[CL_SH_DIGIT] = 8u * (4u * lane + j) + w;
                sh[CL_SH_K] = k - before;
            }
        }
        __syncthreads();
        const uint32_t digit = sh[CL_SH_DIGIT];
        if (digit == 0xFFFFFFFFu) return 0xFFFFFFFFu;  // (block-uniform; the word is next written behind the next select's barriers)
        prefix = (prefix << bits) | digit;
        k = sh[CL_SH_K];
        hi = lo;
    }
    return kmin + (prefix << hi);                      // the bin's lower edge: the bits below `hi` stay open
}

// Layers a.layer_hi .. a.layer_lo of query qi on the table row `tq` (LDS or global memory), by every thread of the block.  L.vis holds
// the visited set handed in, and the caller's barrier stands behind it and the row.  Publishes the hand-over exactly as
// upper_traverse_wave0 leaves it, or — flagged — only fb[q] (CL_ROLE_TOP_LOCAL: nothing at all; the caller resolves the flag).
// Returns the flag, the same for every thread: read back from an LDS word, so that the compiler knows it.
// have_mm: the caller took the minimum and maximum of the row's canonical images while it produced the row (mn, mx: this thread's share).
template <int NT>
__device__ __forceinline__ bool closure_traverse(const HnswUpArgs& a, const int qi, const ClLds& L, const uint32_t* __restrict__ tq,
                                                 const bool have_mm, const uint32_t mn, const uint32_t mx, const unsigned long long row_cycles) {
    const int tid = threadIdx.x, lane = tid & 63;
#ifdef MDB_PIPE_DBG
    unsigned long long dbg_acc[12] = {0, row_cycles, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
#endif
    PIPE_T(t_all);
    const uint32_t ef = (uint32_t)a.ef, su = a.su;
    uint32_t gs = 1;                                   // lanes per frontier point: the row stride rounded up to a power of two (<= 64)
    while (gs < su) gs <<= 1;
    const uint32_t per = NT / gs, slot = (uint32_t)tid % gs, sub = (uint32_t)tid / gs;
    // threads per word of the evaluated bitmap in the single pop's pass (a power of two <= 32): a thread walks its bits one dependent
    // row lookup after the other, and the TOP set's bitmap is ~32 dense words for 256 threads
    uint32_t ltpw = 0u;
    while (ltpw < 5u && (a.vis_words << (ltpw + 1u)) <= (uint32_t)NT) ++ltpw;
    const uint32_t wbits = 32u >> ltpw, wmask = ltpw ? (1u << wbits) - 1u : 0xFFFFFFFFu;
    // every thread owns at most one slice (up to 32 NT points: both launches of the split path on the bench, 31 k and 1 k points):
    // the pass is incremental
    const bool own_one = (a.vis_words << ltpw) <= (uint32_t)NT;
    const uint32_t own_w = (uint32_t)tid >> ltpw, own_b0 = ((uint32_t)tid & ((1u << ltpw) - 1u)) * wbits;
    uint64_t* const sh_minu = (uint64_t*)(L.sh + CL_SH_MINU);
    uint64_t* const sh_mine = (uint64_t*)(L.sh + CL_SH_MINE);
    // the selects run late (header: THE POOL): each at the first layer that uses it, behind that layer's entry into L.vis.  The caller's
    // shares of the row's key range are reduced here, so that no thread carries them through the layers above
    if (have_mm) {
        if (tid == 0) { L.sh[CL_SH_ROWMIN] = 0xFFFFFFFFu; L.sh[CL_SH_ROWMAX] = 0u; }
        __syncthreads();
        const uint32_t wmn = wave_min_u32(mn), wmx = wave_max_u32(mx);
        if (lane == 0) { atomicMin(&L.sh[CL_SH_ROWMIN], wmn); atomicMax(&L.sh[CL_SH_ROWMAX], wmx); }   // (read behind the first layer's barriers)
    }
    // theta: over the launch's row; theta_top: one launch over every upper layer — the layers >= 2 hold the TOP set only, and theta of
    // the whole row would leave next to none of its points certain (the layer would be popped one point at a time)
    uint32_t theta = 0u, theta_top = 0u;
    bool have_theta = false, have_top = false;
    uint32_t ep = a.in_ep ? a.in_ep[qi] : a.entry_c;
    uint32_t evals = a.in_cnt ? a.in_cnt[4 * qi + 0] : 0u, expanded = a.in_cnt ? a.in_cnt[4 * qi + 1] : 0u;
    bool flagged = (a.in_cnt && a.in_cnt[4 * qi + 2]) || (a.in_ovf && a.in_ovf[qi] != 0u) || ep >= a.nu;
    uint32_t* cur = L.fr;
    uint32_t* nxt = L.fr + CL_FR_CAP;

    for (int layer = a.layer_hi; layer >= a.layer_lo && !flagged; --layer) {
        const uint32_t* const lrows = a.rows + (size_t)(layer - a.row_layer0) * a.nu * su;
        // a layer of <= 64 points with edges only among them (ef >= 64): all of it is certain, whatever the row's other points say
        const bool all_certain = (uint32_t)layer >= a.small_layer && ef >= 64u;
        const bool use_top = layer >= 2 && a.top_map != nullptr;
        PIPE_T(t_clear);
        __syncthreads();
        for (uint32_t i = tid; i < a.vis_words; i += NT) { L.ev[i] = 0u; L.ex[i] = 0u; }
        if (tid == 0) {
            L.sh[CL_SH_NNEXT] = 0u; L.sh[CL_SH_NNEXT + 1] = 0u; L.sh[CL_SH_EVALS] = 0u; L.sh[CL_SH_EXPANDED] = 0u; L.sh[CL_SH_HAZARD] = 0u;
            *sh_minu = MDB_KEY_MAX; *sh_mine = MDB_KEY_MAX; L.sh[CL_SH_LT] = 0u; L.sh[CL_SH_LE] = 0u;   // (a layer may open with a single pop)
        }
        __syncthreads();
        // ---- entry point: visited, evaluated (index.rs:219-231)
        const uint32_t k0 = rk_canon(tq[ep]);
        if (k0 == RK_NAN_KEY) { flagged = true; break; }
        if (tid == 0) {
            L.vis[ep >> 5] |= 1u << (ep & 31);
            L.ev[ep >> 5] |= 1u << (ep & 31);
            cur[0] = ep;
        }
        __syncthreads();
        PIPE_TE(CL_DBG_CLEAR, t_clear);
        // ---- this layer's theta: a select taken at a layer above over the same set serves (the visited set has only grown since, and
        // this entry point was unvisited, or the entry point, when it ran); else it runs now, over the points L.vis leaves
        if (!all_certain && !(use_top ? have_top : have_theta)) {   // (block-uniform)
            PIPE_T(t_theta);
            if (use_top) { theta_top = cl_theta<NT>(tq, a.top_map, a.top_n, ef, L.vis, L.hist, L.sh, false); have_top = true; }
            else { theta = cl_theta<NT>(tq, nullptr, a.nu, ef, L.vis, L.hist, L.sh, have_mm); have_theta = true; }
            if (tid == 0) cur[0] = ep;                 // (the histogram lay over the frontier lists)
            __syncthreads();
            PIPE_TE(CL_DBG_THETA, t_theta);
        }
        const uint32_t th = all_certain ? 0xFFFFFFFFu : use_top ? theta_top : theta;
        uint32_t ncur = k0 < th ? 1u : 0u;
        uint32_t parity = 0u;
        uint32_t ncert = ncur, npops = 0u;             // certain points evaluated so far (counted where they are discovered) | single pops of this layer
        // the single pops' pass, per thread and per layer (header: the incremental pass): bits of its slice already folded | minimum
        // pending key (image, ~id) | pending points at that image | minimum evaluated key (image, id)
        uint32_t seen = 0u, mties = 0u;
        uint64_t mu = MDB_KEY_MAX, me = MDB_KEY_MAX;
        for (uint32_t pass = 0; pass <= a.nu + 1u; ++pass) {     // every pass expands at least one point not expanded before
            if (pass > a.nu) { flagged = true; break; }
            // ---- whole frontiers at once: every point of `cur` is expanded by `gs` lanes, lane = edge slot
            PIPE_T(t_rounds);
            while (ncur > 0u) {
                PIPE_ACC(CL_DBG_NROUNDS, 1);
                for (uint32_t base = 0; base < ncur; base += per) {
                    PIPE_ACC(CL_DBG_NTRIPS, 1);
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
                ncert += ncur;
                const bool hz = L.sh[CL_SH_HAZARD] != 0u;
                if (tid == 0) {
                    L.sh[CL_SH_NNEXT + (parity ^ 1u)] = 0u;   // (last read a round ago, behind that round's second barrier)
                    // the words of the next single pop (last read before the barrier that closed the pop before this round)
                    *sh_minu = MDB_KEY_MAX; *sh_mine = MDB_KEY_MAX; L.sh[CL_SH_LT] = 0u; L.sh[CL_SH_LE] = 0u;
                }
                __syncthreads();
                parity ^= 1u;
                uint32_t* const t = cur; cur = nxt; nxt = t;
                if (hz) { flagged = true; break; }
            }
            PIPE_TE(CL_DBG_ROUNDS, t_rounds);
            if (flagged) break;
            PIPE_T(t_pop);
            // ---- ONE pass over the evaluated bitmap (`tpw` threads per word): the minimum pending point u with the pending points that
            // tie with it; the layer's nearest evaluated point so far stays in the threads' `me`
            // the bits `be` of the slice at bit b0 of word w (bx: the expanded bitmap, shifted alike): every point into me, the pending ones
            // into mu and mties (pending points of this thread at its own minimum image)
            const auto fold = [&](const uint32_t w, const uint32_t b0, uint32_t be, const uint32_t bx) {
                while (be) {
                    const uint32_t b = (uint32_t)__builtin_ctz(be);
                    be &= be - 1u;
                    const uint32_t c = 32u * w + b0 + b;
                    const uint32_t k32 = rk_canon(tq[c]);
                    const uint64_t kk = (uint64_t)k32 << 32;
                    me = min(me, kk | c);
                    if (!((bx >> b) & 1u)) {
                        const uint32_t mk = (uint32_t)(mu >> 32);
                        mties = k32 < mk ? 1u : mties + (k32 == mk ? 1u : 0u);
                        mu = min(mu, kk | (uint32_t)~c);
                    }
                }
            };
            if (own_one) {                             // (block-uniform) only the bits evaluated since this thread's last walk
                if ((uint32_t)tid < (a.vis_words << ltpw)) {
                    const uint32_t be = ((L.ev[own_w] >> own_b0) & wmask) & ~seen;
                    seen |= be;
                    fold(own_w, own_b0, be, L.ex[own_w] >> own_b0);
                }
            } else {                                   // several slices per thread: all of them, from nothing
                mu = MDB_KEY_MAX; mties = 0u;        // (me runs on: the evaluated set only grows)
                for (uint32_t item = tid; item < (a.vis_words << ltpw); item += NT) {
                    const uint32_t w = item >> ltpw, b0 = (item & ((1u << ltpw) - 1u)) * wbits;
                    fold(w, b0, (L.ev[w] >> b0) & wmask, L.ex[w] >> b0);
                }
            }
            {
                const uint64_t wmu = cl_wave_min_u64(mu);     // (me is a running minimum: reduced once, behind the layer's last pop)
                if (lane == 0 && wmu != MDB_KEY_MAX) atomicMin((unsigned long long*)sh_minu, (unsigned long long)wmu);
            }
            __syncthreads();
            const uint64_t ukey = *sh_minu;
            if (ukey == MDB_KEY_MAX) { PIPE_TE(CL_DBG_POPS, t_pop); break; }   // nothing pending: the layer is done
            const uint32_t du = (uint32_t)(ukey >> 32), u = ~(uint32_t)ukey;
            // ---- the stop test by counting, without a second pass (header: the counted stop test): what is closer than u is expanded —
            // a certain point or an earlier single pop; what ties with u is pending (counted above) or an earlier single pop
            if (mties && (uint32_t)(mu >> 32) == du) atomicAdd(&L.sh[CL_SH_LE], mties);
            if (tid < 64) {                            // wave 0: the earlier single pops (two ballots per 64 of them)
                uint32_t plt = 0u, ple = 0u;
                for (uint32_t i0 = 0; i0 < npops; i0 += 64) {
                    const bool have = i0 + lane < npops;
                    const uint32_t pk = have ? L.hist[i0 + lane] : 0u;
                    plt += (uint32_t)__popcll(__ballot(have && pk < du));
                    ple += (uint32_t)__popcll(__ballot(have && pk <= du));
                }
                if (lane == 0 && ple) { atomicAdd(&L.sh[CL_SH_LT], plt); atomicAdd(&L.sh[CL_SH_LE], ple); }
            }
            __syncthreads();
            const uint32_t lt = ncert + L.sh[CL_SH_LT], le = ncert + L.sh[CL_SH_LE];
            if (lt >= ef) { PIPE_TE(CL_DBG_POPS, t_pop); break; }   // `distance > furthest.distance`: the layer is done (index.rs:246-248)
            if (le - 1u >= ef) { flagged = true; break; }   // ef others no farther than u: its acceptance hung on the discovery order
            if (npops >= CL_POP_CAP) { flagged = true; break; }   // the list of this layer's single pops is full: the sequential form decides
            if (tid == 0) { cur[0] = u; L.hist[npops] = du; }
            // u leaves the pending set: the thread that folded it forgets its slice and walks it again at the next pop
            if (own_one && (uint32_t)tid == ((u >> 5) << ltpw) + ((u & 31u) >> (5u - ltpw))) { seen = 0u; mu = MDB_KEY_MAX; mties = 0u; }
            ++npops;
            ncur = 1u;
            __syncthreads();
            PIPE_TE(CL_DBG_POPS, t_pop);
            PIPE_ACC(CL_DBG_NPOPS, 1);
        }
        if (flagged) break;
        {   // the layer's nearest evaluated point (smallest image, then smallest id: what the layer hands down, index.rs:177-181); the word
            // is still at its reset value: no pop writes it
            const uint64_t wme = cl_wave_min_u64(me);
            if (lane == 0) atomicMin((unsigned long long*)sh_mine, (unsigned long long)wme);
            __syncthreads();
            ep = (uint32_t)*sh_mine;
        }
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
        CL_DBG_FLUSH();
        return true;
    }
    // ---- the hand-over (see upper_traverse_wave0)
    PIPE_T(t_hand);
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
    PIPE_TE(CL_DBG_HAND, t_hand);
    CL_DBG_FLUSH();
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
    const unsigned long long t_row = CL_DBG_NOW();
    const uint32_t* const tg = a.table + (size_t)qi * a.nu_pad;
    for (uint32_t i = threadIdx.x; i < a.vis_words; i += NT) L.vis[i] = a.in_vis ? a.in_vis[(size_t)qi * a.vis_words + i] : 0u;
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;             // of the row's images, taken from the registers the copy passes through
    if (a.cl_tlds) {
        const uint4* src = (const uint4*)tg;
        uint4* dst = (uint4*)L.row;
        for (uint32_t i = threadIdx.x; i < a.nu_pad / 4; i += NT) {
            const uint4 v = src[i];
            dst[i] = v;
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t k = 4u * i + j < a.nu ? rk_canon(w[j]) : 0xFFFFFFFFu;   // (the padding behind the row's points is not a key)
                mn = min(mn, k);
                mx = 4u * i + j < a.nu ? max(mx, k) : mx;
            }
        }
    }
    __syncthreads();
    const unsigned long long row_cycles = CL_DBG_NOW() - t_row;
    // (two copies of the traversal: its lookups are ds_read in one, global loads in the other)
    if (a.cl_tlds) closure_traverse<NT>(a, qi, L, L.row, true, mn, mx, row_cycles);
    else closure_traverse<NT>(a, qi, L, tg, false, 0u, 0u, row_cycles);
}

// mdb_hnsw_dev.hip.h — device helpers shared by the HNSW traversal kernels (mdb_hnsw.hip: hnsw_beam_kernel;
// mdb_hnsw_upper.hip: hnsw_upper_kernel, hnsw_upper_top_kernel): wave-wide DPP reductions, LDS accessors, the MDB_PIPE_DBG
// macros, and the register beam — the `search_layer` state of one wave — as a type with its operations.
#pragma once
#include "mdb_device.hip.h"

// ---- wave-wide reductions for the register-resident beam (hnsw_beam_kernel)
#define SLOT_EMPTY 0xFFFFFFFFu

#define MDB_DPP_U32(v, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp((int)(v), (int)(v), (ctrl), (rmask), 0xF, false))
// Volatile accesses through a GENERIC pointer are never rewritten to the LDS address space (InferAddressSpaces leaves volatile
// memory operations alone): they compile to flat_load / flat_store with system scope and an s_waitcnt vmcnt(0) each — a poll of
// the mailbox then costs a flat round trip AND waits for every outstanding global load of the wave.  These accessors name the
// address space, so the accesses are plain ds_read / ds_write.
typedef __attribute__((address_space(3))) uint32_t mdb_lds_u32;
typedef __attribute__((address_space(3))) uint64_t mdb_lds_u64;
__device__ __forceinline__ uint32_t lds_vload(const uint32_t* p) { return *(const volatile mdb_lds_u32*)p; }
__device__ __forceinline__ uint64_t lds_vload(const uint64_t* p) { return *(const volatile mdb_lds_u64*)p; }
__device__ __forceinline__ void lds_vstore(uint32_t* p, uint32_t v) { *(volatile mdb_lds_u32*)p = v; }
// Wave-wide min / max in six DPP steps, the DPP operand folded into the min / max itself (v_min_u32_dpp): 12 issue slots
// instead of the 24 of "copy, nop, dpp-move, min" — these reductions sit on wave 0's serial chain, where a slot is ~10 cycles.
// (s_nop 1 = the two wait states a DPP read of a just-written VGPR needs; nobody adds them inside asm.)
#define MDB_WAVE_REDUCE_ASM(op)                                                        \
    asm volatile("s_nop 1\n\t" op " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
                 "s_nop 1\n\t" op " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
                 "s_nop 1\n\t" op " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
                 "s_nop 1\n\t" op " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"          \
                 "s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"        \
                 "s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"        \
                 "s_nop 1"                                                             \
                 : "+v"(v))
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    MDB_WAVE_REDUCE_ASM("v_min_u32_dpp");
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    MDB_WAVE_REDUCE_ASM("v_max_u32_dpp");
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- MDB_PIPE_DBG builds: cycle / event sums of one wave's step into dbg_acc[0..11] = counters[4..15] (MDB_HNSW_DBG=1 prints them).
// Both traversal kernels write the same words, so one of the two files is built with the flag at a time:
//   hnsw_beam_kernel: cycles of P2 | barrier | shadow (selection) | barrier | P4, steps, steps with > 12 / > 24 / > 28 new neighbours,
//                     a distance wave's phase, compactions by the bound / by the select;
//   upper kernels:    cycles of issue + selection | wait | accept | push | pop, steps, new neighbours, prefilter survivors, accepted,
//                     steps that accept one, compactions by the bound / by the select.
// Level 2 (-DMDB_PIPE_DBG=2, the upper file): slots 6..11 hold a finer split of selection and pop — with the waits made explicit —
// in place of the event counts.
#ifdef MDB_PIPE_DBG
#define PIPE_T(t) const unsigned long long t = __builtin_readcyclecounter()
#define PIPE_TE(slot, t) dbg_acc[slot] += __builtin_readcyclecounter() - (t)
#define PIPE_ACC(slot, v) dbg_acc[slot] += (v)
#else
#define PIPE_T(t) do {} while (0)
#define PIPE_TE(slot, t) do {} while (0)
#define PIPE_ACC(slot, v) do {} while (0)
#endif
#if defined(MDB_PIPE_DBG) && MDB_PIPE_DBG >= 2
#define PIPE_T2(t) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t = __builtin_readcyclecounter()
#define PIPE_T2L(t) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long t = __builtin_readcyclecounter()
#define PIPE_ACC2(slot, v) dbg_acc[slot] += (v)
#else
#define PIPE_T2(t) do {} while (0)
#define PIPE_T2L(t) do {} while (0)
#define PIPE_ACC2(slot, v) do {} while (0)
#endif
#if defined(MDB_PIPE_DBG) && MDB_PIPE_DBG < 2
#define PIPE_CNT(slot, v) dbg_acc[slot] += (v)
#else
#define PIPE_CNT(slot, v) do {} while (0)
#endif

// ---- the register beam of one wave: the `search_layer` state of hnsw_beam_kernel's wave 0 and of the upper kernels' wave.
// The upper kernels (upper_traverse_wave0) run their step on the type and operations below.  hnsw_beam_kernel keeps the same
// state as plain arrays and the same step written out in its P4 / shadow, and shares beam_best_id and beam_compact only: on the
// operations its layer-0 instance measured 1.0 - 1.7 % slower in every form tried, with fewer instructions and no more registers
// (HISTORY, "HNSW register beam as a type").  A change to the step is still made in two places until that is understood.
// B is over-full and unsorted: slot s lives in lane s & 63, register s >> 6 (NB registers: 4 / 5 serve ef <= 256, 8 ef <= 448).
// What holds between any two operations:
//  * B is a superset of the working set W of the reference (its ef nearest points seen on this layer): nothing is evicted when a
//    point is accepted, so B also keeps points that have fallen behind furthest.  Every test counts — "fewer than ef elements of B
//    are closer" — and a slot beyond furthest never enters such a count's outcome;
//  * ids are unique in B (a point enters once: the visited set), so a slot is named by its id and no slot index is carried;
//  * slots 0 .. n-1 are used, the others hold (SLOT_EMPTY, 0); cdv is bd on the unexpanded slots (the candidates) and SLOT_EMPTY
//    elsewhere;
//  * fbound >= furthest.distance (SLOT_EMPTY while nothing was rejected on this layer).  It only prefilters the accept test
//    and bounds what a compaction keeps;
//  * a compaction (n + accepted > 64 NB) may drop exactly the slots beyond fbound or, failing that, beyond the ef-th smallest image:
//    never a member of W, possibly the runner-up or the best accepted neighbour of an earlier chunk — the caller selects again.
// The operations take the beam BY VALUE and those that change it return it (secondary results through references to scalars).
// The form is part of the code: a helper is simplified on its own before it is inlined, and what it makes of the beam's arrays
// differs from what the same lines give inside the kernel — check the code objects with scripts/compare_kernels.py and the
// benchmark's HNSW line against the parent after touching one.
template <int NB>
struct Beam {
    uint32_t bd[NB], bi[NB];   // distance image / id per slot
    uint32_t cdv[NB];          // the candidates' images
    int n;                     // used slots
    uint32_t fbound;           // an upper bound of furthest.distance
};
// a candidate in pop order: smallest distance image first, LARGEST id among equals
struct BeamCand {
    uint32_t o, id;
    bool have;
};
__device__ __forceinline__ bool beam_pops_before(const BeamCand x, const BeamCand y) {
    return !y.have || x.o < y.o || (x.o == y.o && x.id > y.id);
}

// B = {entry point}, unexpanded slots: none (the caller expands it at once)
template <int NB>
__device__ __forceinline__ Beam<NB> beam_seed(const uint32_t ep, const uint32_t od, const int lane) {
    Beam<NB> b;
#pragma unroll
    for (int r = 0; r < NB; ++r) { b.bd[r] = SLOT_EMPTY; b.bi[r] = 0; b.cdv[r] = SLOT_EMPTY; }
    if (lane == 0) { b.bd[0] = od; b.bi[0] = ep; }
    b.n = 1;
    b.fbound = SLOT_EMPTY;
    return b;
}

// #{b in B : d_b < o}
template <int NB>
__device__ __forceinline__ int beam_count_closer(const Beam<NB> b, const uint32_t o) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) c += __popcll(__ballot(b.bd[r] < o));
    return c;
}

// nearest unexpanded candidate in pop order (beam_select: .have is false if none; beam_best_id: returns false).  The kernel marks the popped slot by id and needs no slot
// index (the kernels are SGPR-bound: every spilled scalar costs a v_readlane on the wave's critical path).
// One min reduction; the winner's id is the per-lane maximum over the lane's matching slots (in-lane ties resolved for free),
// read from the single matching lane — only distance ties ACROSS lanes pay a second reduction.
template <int NB>
__device__ __forceinline__ bool beam_best_id(const uint32_t (&cdv)[NB], const uint32_t (&bi)[NB], uint32_t& o_out, uint32_t& id_out) {
    uint32_t lm = cdv[0];
#pragma unroll
    for (int r = 1; r < NB; ++r) lm = min(lm, cdv[r]);
    const uint32_t m = wave_min_u32(lm);
    o_out = m;
    if (m == SLOT_EMPTY) return false;
    uint32_t li = 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) li = max(li, cdv[r] == m ? bi[r] : 0u);
    const unsigned long long hm = __ballot(lm == m);
    uint32_t id;
    if (__builtin_expect((hm & (hm - 1)) == 0, 1)) {
        id = (uint32_t)__builtin_amdgcn_readlane((int)li, __ffsll((long long)hm) - 1);
    } else {
        id = wave_max_u32(lm == m ? li : 0u);
    }
    id_out = id;
    return true;
}
template <int NB>
__device__ __forceinline__ BeamCand beam_select(const Beam<NB> b) {
    BeamCand c{SLOT_EMPTY, 0, false};
    c.have = beam_best_id(b.cdv, b.bi, c.o, c.id);
    return c;
}

// Acceptance by counting of one chunk of at most 64 new neighbours, lane = neighbour (`have`, image `od`; `chunk` of them): a
// neighbour is accepted when fewer than ef elements — of B and of the chunk's neighbours before it in edge order — are at most as
// far.  Only the neighbours inside fbound are counted at all; a rejected one tightens fbound: >= ef elements lie within its distance,
// so furthest does from now on.  Returns the beam (fbound refreshed) and the accepted lanes.
template <int NB>
__device__ __forceinline__ Beam<NB> beam_accept(Beam<NB> b, const bool have, const uint32_t od, const int chunk, const int ef,
                                                unsigned long long& accepted_out) {
    unsigned long long surv = __ballot(have && od < b.fbound);
    unsigned long long accepted = 0;
    // fill phase of a layer (every layer restarts from its entry point): with this chunk B still holds at most ef elements, so
    // every count below is < ef — all neighbours are accepted without counting
    if (b.n + chunk <= ef) { accepted = surv; surv = 0; }
    while (surv) {
        const int sidx = __ffsll((long long)surv) - 1;
        surv &= surv - 1;
        const uint32_t ds = (uint32_t)__builtin_amdgcn_readlane((int)od, sidx);
        int cnt = __popcll(__ballot(have && od <= ds) & ((1ull << sidx) - 1ull));
#pragma unroll
        for (int r = 0; r < NB; ++r) cnt += __popcll(__ballot(b.bd[r] <= ds));
        if (cnt < ef) accepted |= 1ull << sidx;
        else b.fbound = min(b.fbound, ds);
    }
    accepted_out = accepted;
    return b;
}

// Push of the accepted lanes' (od, id) into slots n .. n + na - 1 (free: the caller compacts first), in edge order, as candidates;
// `best` is merged with the best accepted neighbour in pop order (a row of more than 64 edges pushes several chunks per step).
template <int NB>
__device__ __forceinline__ Beam<NB> beam_push(Beam<NB> b, const unsigned long long accepted, const uint32_t od, const uint32_t id,
                                              const int lane, BeamCand& best) {
    const int na = __popcll(accepted);
    // ---- one or two accepted neighbours (every step outside a layer's fill phase): each enters its slot n, n + 1 through two scalar
    // reads of its lane — no ds_permute round trip (the pair came back ~130 cycles later, and the NEXT step's selection reads the
    // beam first thing) and no 64-lane select tree; the same loop keeps the best accepted neighbour
#ifndef MDB_HNSW_NO_FAST_PUSH
    if (na <= 2) {
        unsigned long long am = accepted;
        int pos = b.n;
        while (am) {
            const int sidx = __ffsll((long long)am) - 1;
            am &= am - 1;
            const BeamCand c{(uint32_t)__builtin_amdgcn_readlane((int)od, sidx), (uint32_t)__builtin_amdgcn_readlane((int)id, sidx), true};
            const bool me = lane == (pos & 63);
            const int rg = pos >> 6;   // wave-uniform
#pragma unroll
            for (int r = 0; r < NB; ++r) {
                // (one register of NB: the hint keeps these SCALAR branches — folded into selects, every push rewrites all 3 NB registers)
                if (__builtin_expect(rg == r, 0)) {
                    b.bd[r] = me ? c.o : b.bd[r];
                    b.bi[r] = me ? c.id : b.bi[r];
                    b.cdv[r] = me ? c.o : b.cdv[r];
                }
            }
            ++pos;
            if (beam_pops_before(c, best)) best = c;
        }
    } else
#endif
    {
        // ---- forward lane permute: the accepted lane of rank r sends its pair to lane (n + r) & 63, everybody else to an unused
        // lane; no LDS staging round trip on the wave's path
        const bool mine = (accepted >> lane) & 1ull;
        const int dest = mine ? (b.n + __popcll(accepted & ((1ull << lane) - 1ull))) & 63 : (b.n + na) & 63;
        const uint32_t rod = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)od);
        const uint32_t rid = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)id);
        const int rel = (lane - b.n) & 63;
        const bool got = rel < na;
        const int reg = (b.n + rel) >> 6;
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const bool w = got && reg == r;
            b.bd[r] = w ? rod : b.bd[r];
            b.bi[r] = w ? rid : b.bi[r];
            b.cdv[r] = w ? rod : b.cdv[r];
        }
        if (na > 2) {
            // many accepted (fill phase): two wave reductions instead of a scalar loop over them
            const uint32_t mo = wave_min_u32(mine ? od : SLOT_EMPTY);
            const BeamCand c{mo, wave_max_u32(mine && od == mo ? id : 0u), true};
            if (beam_pops_before(c, best)) best = c;
        } else {   // (MDB_HNSW_NO_FAST_PUSH builds only)
            unsigned long long am = accepted;
            while (am) {
                const int sidx = __ffsll((long long)am) - 1;
                am &= am - 1;
                const BeamCand c{(uint32_t)__builtin_amdgcn_readlane((int)od, sidx), (uint32_t)__builtin_amdgcn_readlane((int)id, sidx), true};
                if (beam_pops_before(c, best)) best = c;
            }
        }
    }
    b.n += na;
    return b;
}

// candidates.pop(): the runner-up `ru` (beam_select, taken before this step's pushes) against the best accepted neighbour `best`;
// the winner is popped — its slot leaves the candidates — unless `distance > furthest.distance` (index.rs:246-248): ef or more
// elements of B are closer.  ru_closer is that count for the runner-up, this step's pushes included (the caller takes it in the
// shadow of the distance phase); for `best` it is taken here, and only when `count_needed`: the caller knows a cheap bound of the
// count, and below ef there is nothing to count.  hnsw_beam_kernel passes n >= ef (the count is at most n).  The upper kernels pass
// nexp >= ef, nexp = the expanded slots of B: every unexpanded slot is at least as far as the candidate about to be popped, so the
// count is at most nexp — a layer stops after >= ef expansions or not at all — and they keep ru_closer at 0 until then.
enum BeamPop { BEAM_POP_STOP, BEAM_POP_RUNNER_UP, BEAM_POP_BEST };
template <int NB>
__device__ __forceinline__ Beam<NB> beam_pop(Beam<NB> b, const BeamCand ru, const int ru_closer, const BeamCand best,
                                             const bool count_needed, const int ef, BeamPop& what) {
    const bool take_ru = ru.have && beam_pops_before(ru, best);
    what = BEAM_POP_STOP;   // no candidate left, or the nearest one is beyond furthest
    if (take_ru || best.have) {
        const int closer = take_ru ? ru_closer : count_needed ? beam_count_closer(b, best.o) : 0;
        if (closer >= ef) {
        } else if (take_ru) {   // (one branch per winner: the caller's own branch on `what` folds into it)
            what = BEAM_POP_RUNNER_UP;
#pragma unroll
            for (int r = 0; r < NB; ++r)
                if (b.bi[r] == ru.id) b.cdv[r] = SLOT_EMPTY;   // ids are unique in B (unused slots: already EMPTY)
        } else {
            what = BEAM_POP_BEST;
#pragma unroll
            for (int r = 0; r < NB; ++r)
                if (b.bi[r] == best.id) b.cdv[r] = SLOT_EMPTY;
        }
    }
    return b;
}

// what a layer hands down (index.rs:177-181: first minimum of the (distance, id)-sorted working set): smallest distance, then
// smallest id — two wave reductions over B instead of sorting it
template <int NB>
__device__ __forceinline__ uint32_t beam_nearest_id(const Beam<NB> b) {
    uint32_t m = b.bd[0];
#pragma unroll
    for (int r = 1; r < NB; ++r) m = min(m, b.bd[r]);
    m = wave_min_u32(m);
    uint32_t im = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < NB; ++r) im = b.bd[r] == m ? min(im, b.bi[r]) : im;
    return wave_min_u32(im);
}

// Compaction of the over-full beam B (`n + na > 64 NB`: the step's `na` accepted neighbours find no free slots).  Everything
// farther than furthest.distance may go: it is outside the working set W and cannot tie with furthest; what is kept goes through
// the staging words (C / stage_flag: 64 NB keys / flags of LDS) into slots 0 .. kept-1, in slot order.
//  * bound first: `fbound` — the accept test's prefilter, refreshed whenever a prefilter survivor is rejected — is an upper bound
//    of furthest.distance as it will be once this step's accepted neighbours are in.  When the slots within fbound leave room
//    (16 free slots behind the `na` pushes, so that the next compaction is not the next step's), exactly those
//    are kept: NB ballots.  B then holds W and a few slots between furthest and fbound — the same kind of slot it holds between
//    two compactions anyway (the counts of the accept and stop tests never see a slot beyond furthest);
//  * otherwise (no rejection yet on this layer: fbound == SLOT_EMPTY; or a long run of ties at the bound) the exact ef-th smallest
//    image of B by a 32-step ballot radix select (EMPTY = 0xFFFFFFFF sorts last) — 32 NB ballots on a lone wave.
// n and fbound are updated; returns true when the bound sufficed.  The caller re-checks `n + na` (overflow) and re-selects its
// runner-up, which may have been dropped.
#ifndef MDB_HNSW_BOUND_COMPACT
#define MDB_HNSW_BOUND_COMPACT 1
#endif
template <int NB>
__device__ __forceinline__ bool beam_compact(uint32_t (&bd)[NB], uint32_t (&bi)[NB], uint32_t (&cdv)[NB], int& n, uint32_t& fbound,
                                             const int ef, const int na, uint64_t* const C, uint32_t* const stage_flag, const int lane,
                                             const unsigned long long lt_mask) {
    constexpr int MARGIN = 16;   // free slots the bound drop must leave behind the pushes
    bool by_bound = false;
    if (MDB_HNSW_BOUND_COMPACT && fbound != SLOT_EMPTY) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < NB; ++r) c += __popcll(__ballot(bd[r] <= fbound));
        by_bound = c + na <= 64 * NB - MARGIN;
    }
    uint32_t f = fbound;
    if (!by_bound) {
        uint32_t prefix = 0;
        int need = ef;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t hi_mask = bit == 31 ? 0u : (0xFFFFFFFFu << (bit + 1));
            int cnt0 = 0;
#pragma unroll
            for (int r = 0; r < NB; ++r)
                cnt0 += __popcll(__ballot((((bd[r] ^ prefix) & hi_mask) == 0u) && !((bd[r] >> bit) & 1u)));
            if (cnt0 < need) { need -= cnt0; prefix |= 1u << bit; }
        }
        f = prefix;
    }
    int kept = 0;
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const bool keep = bd[r] <= f;  // EMPTY never kept (f is a real distance: n > ef here)
        const unsigned long long km = __ballot(keep);
        if (keep) {
            const int pos = kept + __popcll(km & lt_mask);
            C[pos] = ((uint64_t)bd[r] << 32) | bi[r];
            stage_flag[pos] = cdv[r] != SLOT_EMPTY ? 1u : 0u;
        }
        kept += __popcll(km);
    }
#pragma unroll
    for (int r = 0; r < NB; ++r) {
        const int idx = lane + 64 * r;
        const bool in = idx < kept;
        const uint64_t kk = in ? C[idx] : 0;
        bd[r] = in ? (uint32_t)(kk >> 32) : SLOT_EMPTY;
        bi[r] = in ? (uint32_t)kk : 0u;
        cdv[r] = (in && stage_flag[idx] != 0u) ? bd[r] : SLOT_EMPTY;
    }
    n = kept;
    fbound = min(fbound, f);
    return by_bound;
}
template <int NB>
__device__ __forceinline__ Beam<NB> beam_compact(Beam<NB> b, const int ef, const int na, uint64_t* const C, uint32_t* const stage_flag,
                                                 const int lane, bool& by_bound_out) {
    by_bound_out = beam_compact<NB>(b.bd, b.bi, b.cdv, b.n, b.fbound, ef, na, C, stage_flag, lane, (1ull << lane) - 1ull);
    return b;
}

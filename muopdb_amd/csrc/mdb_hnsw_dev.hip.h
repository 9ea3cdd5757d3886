// mdb_hnsw_dev.hip.h — device helpers shared by the HNSW traversal kernels (mdb_hnsw.hip: hnsw_beam_kernel;
// mdb_hnsw_upper.hip: hnsw_upper_kernel): wave-wide DPP reductions, LDS accessors, the register beam's selection.
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

// the register beam: NB registers of 64 slots per array (5: ef <= 256; 8: ef <= 448) — a template parameter of the traversal kernels

// nearest unexpanded candidate in pop order (smallest distance image, LARGEST id among equals); `cdv` holds the distance
// image of unexpanded slots and SLOT_EMPTY elsewhere.  Returns false if none.  Ids are unique in B, so the kernel marks
// the popped slot by id and needs no slot index (the kernel is SGPR-bound: every spilled scalar costs a v_readlane on wave
// 0's critical path).
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


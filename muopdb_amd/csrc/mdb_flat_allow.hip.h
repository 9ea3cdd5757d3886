// mdb_flat_allow.hip.h — flat_scan_kernel under a per-call allow bitmap over ROW ids (mdb_flat_search_filtered): not a kernel of its
// own but three hooks into flat_scan_kernel's scan loop, taken when FlatAllow::bits is set: the distance cascade, the keys, the
// selector rounds and the epilogue (the NaN raise, finish, the store of the partial lists) are the unfiltered scan's own.
//
// A filter of density rho leaves a 64-row tile with ~64 rho live lanes.  With the dead lanes' loads switched off a masked scan fetches
// the same 64-byte sectors as a gather of the live rows (measured: DESIGN 5e), but it spends a block-wide selector round — QT selectors,
// a barrier — on every group of mostly dead keys.  What the ring below saves is ROUNDS, where a block loops over many groups; so
// each tile is treated by ITS OWN popcount c (the OR of the group's QT bitmaps — two wave-uniform word loads per query):
//   c >= dense    the tile is scanned in place: lane = row, as the unfiltered scan does;
//   0 < c < dense nothing is fetched: the wave appends its live row ids to a ring of pending ids in LDS (position = the rows below it in
//                 the mask, one LDS atomic per wave for the slot range).  When 64 ids are pending a wave without a dense tile takes
//                 them as a VIRTUAL tile: lane l scores row ring[l] through the same TileLoader / exact_sums — the same bits — at
//                 one sector per row;
//   c == 0        two scalar loads and nothing else.
// What is left in the ring after the last group is drained with the lanes past its end idle.
//
// BlockSelect's rounds are block-wide (warm_start / offer / round_end hold barriers), so whether a group runs a round is decided
// block-uniformly from ONE LDS word per group, read behind one barrier: bits 0-15 the ids the group's sparse waves appended, bits
// 16-19 the waves with a dense tile.  The words rotate by three exactly as BlockSelect's admission counters do: the word of group j
// is cleared behind the barrier of group j + 1 (its readers are all past it) and used again by group j + 3.  Everything else — the
// ring's write and read positions, the waves' roles — is recomputed by every thread from those words and stays uniform in registers.
// A group that only enqueues runs no round; the selectors' warm start moves to the first round that does run.
//
// Ring: positions are running totals, slot = position % FLAT_ALLOW_RING.  At most 63 ids stay pending behind a group (free waves >=
// sparse waves, so a group consumes at least what it appended once 64 are pending) and a group appends at most 4 x 64, so live
// positions span < 320 slots; a slot is overwritten only behind the round_end barrier of the round that read it.
#pragma once
#include "mdb_device.hip.h"
#include "mdb_kernels.h"

#define FLAT_ALLOW_RING 512   // ids; power of two >= 4 * 64 + 4 * (dense - 1) + 63 for every dense <= 65
#define FLAT_ALLOW_LDS (FLAT_ALLOW_RING * 4 + 16)

// the 64 allow bits of `tile` for one bitmap row (wave-uniform: scalar loads); words past the bitmap's last are not read
__device__ __forceinline__ uint64_t flat_allow_tile_bits(const uint32_t* __restrict__ row, size_t tile, size_t nwords) {
    const size_t w = tile * 2;
    const uint32_t lo = w < nwords ? row[w] : 0u;
    const uint32_t hi = w + 1 < nwords ? row[w + 1] : 0u;
    return ((uint64_t)hi << 32) | lo;
}

// mdb_stats::scored_vectors: the allowed rows below n of this block's queries, counted from the bitmaps themselves by the first
// FLAT_ALLOW_COUNT_BLOCKS blocks of every query group, each a share of the words (a shared bitmap: by the first group alone, times the
// batch) — a few device atomics per query, none in the scan.  (ONE block walking the 32 K words of a 1 M-row bitmap was the longest
// block of the launch at low densities.)  Block-uniform; `word` is a zeroed LDS word and is left zero.
#define FLAT_ALLOW_COUNT_BLOCKS 16
template <int QT>
__device__ __forceinline__ void flat_allow_count(const FlatAllow& fa, size_t n, size_t q0, uint32_t* word) {
    const size_t nwords = (n + 31) / 32;
    const int nq = fa.stride ? (int)min((size_t)QT, (size_t)fa.nq - q0) : 1;
    for (int i = 0; i < nq; ++i) {
        const uint32_t* row = fa.bits + (q0 + i) * (size_t)fa.stride;
        uint32_t c = 0;
        // share s of the words: s, s + COUNT_BLOCKS, ... blocks of 256 (a constant stride: a run-time one makes the unrolled loop's trip
        // count a 64-bit division); a grid of fewer blocks takes several shares per block
        for (unsigned s = blockIdx.x; s < FLAT_ALLOW_COUNT_BLOCKS; s += gridDim.x)
        for (size_t w = (size_t)s * MDB_BLOCK + threadIdx.x; w < nwords; w += (size_t)FLAT_ALLOW_COUNT_BLOCKS * MDB_BLOCK) {
            uint32_t x = row[w];
            if (w == nwords - 1 && (n & 31)) x &= (1u << (n & 31)) - 1u;
            c += (uint32_t)__popc(x);
        }
        if (c) atomicAdd(word, c);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long rows = *word;
            if (rows) atomicAdd(fa.scored, fa.stride ? rows : rows * fa.nq);
            *word = 0;
        }
        __syncthreads();
    }
}

// ---- the mode's three hooks into flat_scan_kernel's ONE scan loop (one exact_sums call site for both modes: a second inlined copy of
// the cascade doubled the kernel's scalar spills and left it a private segment).  qlds: FLAT_ALLOW_LDS bytes of LDS behind the selectors.
struct FlatAllowRun {   // uniform across the block
    uint32_t tail = 0, head = 0;   // ids appended / consumed so far
    int slot = 0;                  // this group's state word
    int nreal = 0;                 // queries of this group that exist (the rest: padding)
};
enum { FLAT_ALLOW_DONE = 0, FLAT_ALLOW_NO_ROUND = 1, FLAT_ALLOW_ROUND = 2 };

// before the loop (block-uniform): clears the state words, counts the allowed rows
template <int QT>
__device__ __forceinline__ void flat_allow_begin(const FlatAllow& fa, FlatAllowRun& r, size_t n, size_t q0, char* qlds, uint32_t* word) {
    r.nreal = q0 < fa.nq ? (int)min((size_t)QT, (size_t)fa.nq - q0) : 0;
    if (threadIdx.x < 3) ((uint32_t*)qlds)[threadIdx.x] = 0;
    __syncthreads();
    if (blockIdx.x < FLAT_ALLOW_COUNT_BLOCKS && fa.scored && r.nreal > 0 && (fa.stride || blockIdx.y == 0)) flat_allow_count<QT>(fa, n, q0, word);
}

// one pass: group g, or a drain pass (g >= ngroups, nothing appended) while ids are pending.  FLAT_ALLOW_DONE: leave the loop;
// FLAT_ALLOW_NO_ROUND: the group only enqueued, or held nothing; FLAT_ALLOW_ROUND: this lane scores row v if `have` and the block
// runs a selector round.  The result is block-uniform.
template <int QT>
__device__ __forceinline__ int flat_allow_group(const FlatAllow& fa, FlatAllowRun& r, char* qlds, size_t g, size_t ngroups, size_t n,
                                                size_t ntiles, size_t q0, uint32_t& v, bool& have) {
    uint32_t* const state = (uint32_t*)qlds;          // [3] the groups' rotating words
    uint32_t* const ring = (uint32_t*)(qlds + 16);    // [FLAT_ALLOW_RING] pending row ids
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / MDB_WAVE)), lane = threadIdx.x % MDB_WAVE;
    const size_t nwords = (n + 31) / 32;
    const bool drain = g >= ngroups;
    if (drain && r.tail == r.head) return FLAT_ALLOW_DONE;
    const size_t tile = g * 4 + wave;
    uint64_t any = 0;
    if (!drain && tile < ntiles) {
        const int nrows = fa.stride ? r.nreal : (r.nreal > 0 ? 1 : 0);
#pragma unroll
        for (int i = 0; i < QT; ++i)
            if (i < nrows) any |= flat_allow_tile_bits(fa.bits + (q0 + i) * (size_t)fa.stride, tile, nwords);
        const size_t left = n - tile * MDB_TILE;   // >= 1
        if (left < MDB_TILE) any &= (1ull << left) - 1ull;
    }
    const uint32_t c = (uint32_t)__popcll(any);
    const bool dense = c > 0 && c >= fa.dense;
    if (dense) {
        if (lane == 0) atomicAdd(&state[r.slot], 0x10000u << wave);
    } else if (c > 0) {
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&state[r.slot], c) & 0xFFFFu;
        at = r.tail + (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
        if ((any >> lane) & 1ull) ring[(at + (uint32_t)__popcll(any & ((1ull << lane) - 1ull))) & (FLAT_ALLOW_RING - 1)] = (uint32_t)(tile * MDB_TILE + lane);
    }
    __syncthreads();
    const uint32_t word = state[r.slot];
    if (threadIdx.x == 0) state[r.slot == 0 ? 2 : r.slot - 1] = 0;
    r.slot = r.slot == 2 ? 0 : r.slot + 1;
    r.tail += word & 0xFFFFu;
    const uint32_t dmask = word >> 16, pending = r.tail - r.head;
    const uint32_t nfree = 4u - (uint32_t)__popc(dmask);
    // virtual tiles: whole ones while groups follow, the remainder too in a drain pass
    const uint32_t taken = min(drain ? (pending + 63u) / 64u : pending / 64u, nfree);
    if (dmask == 0 && taken == 0) return FLAT_ALLOW_NO_ROUND;
    v = 0;
    have = false;
    if (dense) {
        v = (uint32_t)(tile * MDB_TILE + lane);
        have = (any >> lane) & 1ull;
    } else {
        const uint32_t fr = (uint32_t)__popc(~dmask & ((1u << wave) - 1u));   // this wave among the free ones
        if (fr < taken) {
            const uint32_t pos = r.head + fr * 64u + lane;
            have = (int32_t)(r.tail - pos) > 0;
            if (have) v = ring[pos & (FLAT_ALLOW_RING - 1)];
        }
    }
    r.head += min(taken * 64u, pending);
    return FLAT_ALLOW_ROUND;
}

// row v's bit per query of the group (a virtual tile's rows come from many tiles); padding queries: 0
template <int QT>
__device__ __forceinline__ void flat_allow_row_bits(const FlatAllow& fa, const FlatAllowRun& r, size_t q0, uint32_t v, uint32_t (&bit)[QT]) {
#pragma unroll
    for (int i = 0; i < QT; ++i) bit[i] = i < r.nreal ? (fa.bits[(q0 + i) * (size_t)fa.stride + (v >> 5)] >> (v & 31)) & 1u : 0u;
}

// mdb_ivf_scan.hip.h — device code of mdb_ivf.hip, part 1: the load-time gathers, the scans' arguments and tile map, and the one-phase
// posting-list scans (f32, PQ by codebook rows).  Included by mdb_ivf.hip only.
#pragma once

// ------------------------------------------------------------------------------------------ load-time kernels
__global__ void fill_u32_kernel(uint32_t* p, size_t n, uint32_t v) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) p[t] = v;
}

// Gather f32 vectors (row-major, 4-byte aligned, arbitrary base) into SoA tiles.
// tile_src[t] = byte offset in `src` of vector 0 of the store the tile reads from;
// ids == nullptr => vector index = tile_first[t] + lane, valid if < tile_count[t].
__global__ __launch_bounds__(256) void gather_f32_tiles_kernel(const uint8_t* __restrict__ src,
                                                               const uint64_t* __restrict__ tile_src,
                                                               const uint32_t* __restrict__ tile_limit,
                                                               const uint32_t* __restrict__ ids,
                                                               const uint32_t* __restrict__ tile_first, int d, int d4,
                                                               float4* __restrict__ tiles, size_t total4,
                                                               uint32_t* __restrict__ flags) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    size_t lane = t % MDB_TILE;
    size_t c4 = (t / MDB_TILE) % d4;
    size_t tile = t / ((size_t)MDB_TILE * d4);
    uint32_t id = ids ? ids[tile * MDB_TILE + lane] : tile_first[tile] + (uint32_t)lane;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    bool valid = ids ? (id != 0xFFFFFFFFu) : (id < tile_limit[tile]);
    if (valid && ids && id >= tile_limit[tile]) {
        atomicOr(flags, MDB_FLAG_RANGE);  // "index out of bounds" (async_storage.rs:113-115)
        valid = false;
    }
    if (valid) {
        const float* p = (const float*)(src + tile_src[tile] + (size_t)id * d * 4);
        int e = (int)c4 * 4;
        r.x = e + 0 < d ? p[e + 0] : 0.f;
        r.y = e + 1 < d ? p[e + 1] : 0.f;
        r.z = e + 2 < d ? p[e + 2] : 0.f;
        r.w = e + 3 < d ? p[e + 3] : 0.f;
    }
    tiles[t] = r;
}

// f32 POSTING LISTS are laid out in UNITS of 16 slots (slot s = unit s / 16, position s % 16; a list's slots are consecutive).  A
// wave's tile is four consecutive units stored as ONE 64-lane SoA tile (`(unit0 * d4 * 16) + c4 * 64 + lane`) — or, for a list's LAST
// tile when n = 1..3 units are left, those n units stored 16 n wide (`(unit0 * d4 * 16) + c4 * 16 n + lane`, lanes >= 16 n idle): a
// list pads to 16 slots, not 64.  (MuopDB's SPANN lists average ~64 vectors — C4: 64.25 — so half of them used to spill one or two
// vectors into a second 64-slot tile: 1.56 x the rows resident; in units of 16: 1.13 x.  Capacity only: idle lanes never loaded anything.)
// unit_desc[u] = (first unit of the tile << 4) | (u's position in the tile) << 2 | (units of a narrow tail tile, 0 = a whole tile).
__global__ __launch_bounds__(256) void gather_f32_units_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ unit_src,
                                                               const uint32_t* __restrict__ unit_limit, const uint32_t* __restrict__ ids,
                                                               const uint32_t* __restrict__ unit_desc, int d, int d4,
                                                               float4* __restrict__ tiles, size_t total4, uint32_t* __restrict__ flags) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total4) return;
    const size_t l = t % MDB_UNIT;
    const size_t c4 = (t / MDB_UNIT) % d4;
    const size_t unit = t / ((size_t)MDB_UNIT * d4);
    const uint32_t id = ids[unit * MDB_UNIT + l];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    bool valid = id != 0xFFFFFFFFu;
    if (valid && id >= unit_limit[unit]) {
        atomicOr(flags, MDB_FLAG_RANGE);  // "index out of bounds" (async_storage.rs:113-115)
        valid = false;
    }
    if (valid) {
        const float* p = (const float*)(src + unit_src[unit] + (size_t)id * d * 4);
        int e = (int)c4 * 4;
        r.x = e + 0 < d ? p[e + 0] : 0.f;
        r.y = e + 1 < d ? p[e + 1] : 0.f;
        r.z = e + 2 < d ? p[e + 2] : 0.f;
        r.w = e + 3 < d ? p[e + 3] : 0.f;
    }
    const uint32_t ds = unit_desc[unit];
    const size_t w = (ds & 3u) ? (size_t)(ds & 3u) * MDB_UNIT : MDB_TILE;
    tiles[(size_t)(ds >> 4) * d4 * MDB_UNIT + c4 * w + (size_t)((ds >> 2) & 3u) * MDB_UNIT + l] = r;
}

// Gather PQ codes (m bytes per vector) into tiles of 64 slots x mw 4-byte words:
// word index of (tile, w, lane) = (tile*mw + w)*64 + lane, zero padded.
__global__ __launch_bounds__(256) void gather_code_tiles_kernel(const uint8_t* __restrict__ src,
                                                                const uint64_t* __restrict__ tile_src,
                                                                const uint32_t* __restrict__ tile_limit,
                                                                const uint32_t* __restrict__ ids, int m, int mw,
                                                                uint32_t* __restrict__ codes, size_t total,
                                                                uint32_t* __restrict__ flags) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    size_t lane = t % MDB_TILE;
    size_t w = (t / MDB_TILE) % mw;
    size_t tile = t / ((size_t)MDB_TILE * mw);
    uint32_t id = ids[tile * MDB_TILE + lane];
    uint32_t v = 0;
    if (id != 0xFFFFFFFFu) {
        if (id >= tile_limit[tile]) {
            atomicOr(flags, MDB_FLAG_RANGE);
        } else {
            const uint8_t* p = src + tile_src[tile] + (size_t)id * m;
            for (int i = 0; i < 4; ++i) {
                int e = (int)w * 4 + i;
                if (e < m) v |= (uint32_t)p[e] << (8 * i);
            }
        }
    }
    codes[t] = v;
}

// ------------------------------------------------------------------------------------------ scan kernels
struct ScanArgs {
    const IvfUserDev* users;
    const uint32_t* q_user;        // nullptr => user 0
    const uint32_t* list_tile_off; // [G+1] tile index of each global list
    const uint32_t* slot_ids;      // [tiles*64]
    const uint32_t* tomb;          // tombstone bitmap arena
    const uint32_t* probes;        // [B][probe_stride] centroid (list) ids local to the user
    const uint32_t* probe_cnt;     // nullptr => probe_stride probes for every query
    int probe_stride;
    int k;
    uint64_t* partial;             // [B][nsplit][k]
    uint32_t* flags;
    unsigned long long* counters;  // [2] += scored vectors
    // Planner hook (scan_posting_list, index.rs:214-226): query i keeps point p iff bit p of
    // allow[i*allow_stride ...] is set.  Without a filter `allow` points at one all-ones word and
    // allow_mask = 0 folds every index onto it (branch-free in the pipelined PQ kernel).
    const uint32_t* allow;
    uint32_t allow_stride, allow_mask;
    uint32_t* counts_out;          // nsplit == 1: `partial` is the final [B][k] key array and the row lengths go here (no merge launch)
    const uint32_t* gate;          // non-null: the launch is a fallback and returns at once unless *gate != 0 (its scored count is not added)
    int eager_trim;                // PQ bound-filter scan: tighten the selector's threshold as soon as k + 64 keys are queued
    uint32_t no_masks = 0;         // nothing was ever invalidated and the call has no planner filter: neither tombstone nor allow words are read
};

__device__ __forceinline__ bool tomb_test(const uint32_t* tomb, uint32_t base_word, uint32_t pid) {
    return (tomb[base_word + (pid >> 5)] >> (pid & 31)) & 1u;
}
__device__ __forceinline__ bool allow_test(const ScanArgs& a, int qi, uint32_t pid) {
    return (a.allow[(size_t)qi * a.allow_stride + ((pid >> 5) & a.allow_mask)] >> (pid & 31)) & 1u;
}

// ------------------------------------------------------------------------------------------
// Flattened tile sequence of one query's probed lists (shared by the f32 and the PQ scan): the lists of
// up to MAP_PCH probes are laid end to end, so wave w of round r takes tile (r*nsplit + split)*NW + w
// whatever the individual list lengths are (short lists would otherwise idle most waves).
#define MAP_PCH 512
struct TileMap {
    uint32_t* pstart;  // [MAP_PCH]     first tile of probe j
    uint32_t* ppref;   // [MAP_PCH + 1] exclusive prefix of tile counts (unused entries == total)
    static __host__ __device__ size_t lds_bytes() { return (2 * MAP_PCH + 16) * 4; }
    __device__ void init(void* lds) {
        pstart = (uint32_t*)lds;
        ppref = pstart + MAP_PCH;
    }
    // all threads of the block (>= MAP_PCH threads not required); returns the number of tiles; sets bad on
    // an out-of-range list id ("Index out of bound", storage.rs:280-286 — the list is skipped)
    // (f32 lists: list_tile_off counts UNITS of 16 slots — gather_f32_units_kernel; a list of n units is ceil(n / 4) wave tiles, the
    // last one n % 4 units wide when that is not 0: bits 30-31 of pstart)
    __device__ int build(const ScanArgs& a, const IvfUserDev& u, int qi, int p0, int n, bool& bad) {
        const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
        for (int j = tid; j < MAP_PCH; j += nthr) {
            uint32_t t0 = 0, cnt = 0;
            if (j < n) {
                uint32_t c = a.probes[(size_t)qi * a.probe_stride + p0 + j];
                if (c >= u.num_lists) bad = true;
                else {
                    uint32_t g = u.list_base + c;
                    t0 = a.list_tile_off[g];
                    const uint32_t units = a.list_tile_off[g + 1] - t0;
                    cnt = (units + MDB_UPT - 1) / MDB_UPT;
                    t0 |= (units & (MDB_UPT - 1)) << 30;
                }
            }
            pstart[j] = t0;
            ppref[j + 1] = cnt;
        }
        __syncthreads();
        if (tid < MDB_WAVE) {
            constexpr int PER = MAP_PCH / MDB_WAVE;
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
        return (int)ppref[MAP_PCH];
    }
    // wave-uniform t < total: index of the list holding tile t (all 64 lanes must call)
    __device__ __forceinline__ int list_of(uint32_t t) const {
        const int lane = threadIdx.x & 63;
        int j = 0;
#pragma unroll
        for (int x = 0; x < MAP_PCH / MDB_WAVE; ++x) j += __popcll(__ballot(ppref[x * MDB_WAVE + lane + 1] <= t));
        return j;
    }
    // first unit of wave tile t of list j; `width`: its slots (64, or 16 / 32 / 48 for the list's narrow tail)
    __device__ __forceinline__ uint32_t unit_of(uint32_t t, int j, uint32_t& width) const {
        const uint32_t ps = pstart[j], local = t - ppref[j];
        width = ((ps >> 30) && local + 1 == ppref[j + 1] - ppref[j]) ? (ps >> 30) * MDB_UNIT : MDB_TILE;
        return (ps & 0x3FFFFFFFu) + MDB_UPT * local;
    }
};

// NoQuantizer<D>: distance = D::calculate(query, vector) (noq/mod.rs:44-51): sqrt L2 / neg dot
// BLK: threads per block (256; 128 / 64 for short probe sets: a block ends with its slowest wave, so 9 tiles on 4 waves idle a quarter
// of the block's wave rounds; fewer waves per block, and more splits of the tile sequence, waste less)
template <int METRIC, int BLK>
__global__ __launch_bounds__(BLK) void ivf_scan_f32_kernel(ScanArgs a, const float4* __restrict__ tiles, DistPlan p,
                                                                 const float* __restrict__ q, int qstride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    TileMap map;
    map.init(lds + ((BlockSelect<BLK>::lds_bytes(a.k) + 15) & ~(size_t)15));
    // workgroups go to the 8 XCDs round robin (id = query x nsplit + blockIdx.x), and the splits of a query are unequal — the first
    // ones hold four tiles, the last one the remainder, those beyond return at once.  Taken as is, 8 splits put every query's split s
    // on XCD s: four XCDs stream, four run empty blocks (full C4: 0.65 ms per step at 8 splits, 0.97 at 16, 0.55 at 4 and 12 against
    // 0.49-0.50 at 3, 5, 6).  The split index is rotated by the query index, slowed to the period the XCD assignment has in it.
    const int qi = blockIdx.y, nsplit = gridDim.x;
    // (shifts and a subtract loop, no integer division: its expansion goes through v_rcp / v_fma, which the exact kernels' code
    // objects are checked not to contain)
    const int xsh = (nsplit & 7) == 0 ? 0 : ((nsplit & 3) == 0 ? 1 : ((nsplit & 1) == 0 ? 2 : 3));   // log2(8 / gcd(nsplit, 8))
    int split = (int)blockIdx.x + ((qi >> xsh) & 15);
    while (split >= nsplit) split -= nsplit;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / MDB_WAVE), lane = threadIdx.x % MDB_WAVE;
    constexpr int NW = BLK / MDB_WAVE;
    const IvfUserDev u = a.users[a.q_user ? a.q_user[qi] : 0];
    const float* qb = q + (size_t)qi * qstride;
    const int np = a.probe_cnt ? (int)a.probe_cnt[qi] : a.probe_stride;
    bool nan_seen = false, bad = false, first = true;
    unsigned scored = 0;
    int T0 = -1;
    if (u.valid && np <= MAP_PCH && nsplit > 1) {
        // one chunk of probes (the usual case): a split beyond the query's tiles has nothing to scan — it leaves an empty row behind
        // without setting a selector up, so the launch can afford as many splits as the LONGEST probe sets want
        T0 = map.build(a, u, qi, 0, np, bad);
        if (split * NW >= T0) {   // uniform
            if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
            uint64_t* dst0 = a.partial + ((size_t)qi * nsplit + split) * a.k;
            for (int j = threadIdx.x; j < a.k; j += BLK) dst0[j] = MDB_KEY_MAX;
            return;
        }
    }
    BlockSelect<BLK> sel;
    sel.init(lds, a.k);
    if (u.valid) {
        for (int p0 = 0; p0 < np; p0 += MAP_PCH) {
            const int T = T0 >= 0 ? T0 : map.build(a, u, qi, p0, min(MAP_PCH, np - p0), bad);
            const int per_round = NW * nsplit;
            const int rounds = (T + per_round - 1) / per_round;
            for (int r = 0; r < rounds; ++r) {
                const int t = (r * nsplit + split) * NW + wave;
                uint64_t key = MDB_KEY_MAX;
                if (t < T) {
                    uint32_t width;
                    const uint32_t unit = map.unit_of((uint32_t)t, map.list_of((uint32_t)t), width);   // wave-uniform
                    const uint32_t pid = (uint32_t)lane >= width ? 0xFFFFFFFFu : a.slot_ids[(size_t)unit * MDB_UNIT + lane];
                    if (pid != 0xFFFFFFFFu && (a.no_masks || (!tomb_test(a.tomb, u.tomb_base, pid) && allow_test(a, qi, pid)))) {
                        // (a constant-stride path for whole tiles measured no different: 355.8 / 360.3 / 356.2 vs 359.4 / 353.4 / 358.6 us, full C4)
                        UnitLoader ld{tiles + (size_t)unit * p.d4 * MDB_UNIT + lane, (size_t)width};
                        float raw[1];
                        exact_sums<METRIC, 1, UnitLoader, 3>(ld, qb, 0, p, raw);
                        float dist = finish_distance<METRIC>(raw[0]);
                        if (dist != dist) nan_seen = true;
                        key = make_key(dist, pid);
                        ++scored;
                    }
                }
                if (first) { sel.warm_start(key); first = false; }
                sel.offer(key);
                sel.round_end();
            }
            __syncthreads();  // the map is rebuilt by the next chunk
        }
    }
    if (nan_seen) atomicOr(a.flags, MDB_FLAG_NAN);
    if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
    {
        unsigned long long ws = scored;  // wave total -> one atomic per wave
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ws += __shfl_xor((unsigned)ws, m);
        // one device-scope atomic per BLOCK (wave totals meet in LDS first): thousands of atomics on one cache
        // line serialise and were the largest fixed cost of a scan block
        if (lane == 0 && ws) atomicAdd(sel.spare(), (uint32_t)ws);
    }
    sel.finish();
    if (threadIdx.x == 0 && *sel.spare()) atomicAdd(&a.counters[2], (unsigned long long)*sel.spare());
    uint64_t* dst = a.partial + ((size_t)qi * nsplit + split) * a.k;
    uint32_t c = sel.count();
    for (int j = threadIdx.x; j < a.k; j += BLK) dst[j] = j < (int)c ? sel.buf[j] : MDB_KEY_MAX;
    if (a.counts_out && threadIdx.x == 0) a.counts_out[qi] = c;
}

template <int METRIC, bool LUT_LDS>
__global__ __launch_bounds__(MDB_BLOCK) void ivf_scan_pq_kernel(ScanArgs a, const uint32_t* __restrict__ codes, int m,
                                                                int mw, int K, int subdim, DistPlan sp,
                                                                const float* __restrict__ cb,
                                                                const uint8_t* __restrict__ qcodes) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    BlockSelect<MDB_BLOCK> sel;
    sel.init(lds, a.k);
    float* lut = (float*)(lds + ((BlockSelect<MDB_BLOCK>::lds_bytes(a.k) + 15) & ~(size_t)15));
    const int qi = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x;
    const int wave = threadIdx.x / MDB_WAVE, lane = threadIdx.x % MDB_WAVE;
    const IvfUserDev u = a.users[a.q_user ? a.q_user[qi] : 0];
    const uint8_t* qc = qcodes + (size_t)qi * m;
    const int np = a.probe_cnt ? (int)a.probe_cnt[qi] : a.probe_stride;
    bool nan_seen = false, bad = false;
    unsigned scored = 0;
    if (LUT_LDS) {
        const int rowlen = K * subdim, total = m * rowlen;
        for (int i = threadIdx.x; i < total; i += MDB_BLOCK) {
            int s = i / rowlen, e = i % subdim;
            float av = cb[((size_t)s * K + qc[s]) * subdim + e];
            lut[i] = acc_term<METRIC>(0.0f, av, cb[i]) ;  // 0 + term == term exactly (term >= +0 or any finite)
        }
        __syncthreads();
    }
    if (u.valid) {
        for (int j = split; j < np; j += nsplit) {
            uint32_t c = a.probes[(size_t)qi * a.probe_stride + j];
            if (c >= u.num_lists) { bad = true; continue; }
            uint32_t g = u.list_base + c;
            uint32_t t0 = a.list_tile_off[g], t1 = a.list_tile_off[g + 1];
            for (uint32_t tb = t0; tb < t1; tb += 4) {
                uint32_t tile = tb + wave;
                uint64_t key = MDB_KEY_MAX;
                if (tile < t1) {
                    uint32_t pid = a.slot_ids[(size_t)tile * MDB_TILE + lane];
                    if (pid != 0xFFFFFFFFu && !tomb_test(a.tomb, u.tomb_base, pid) && allow_test(a, qi, pid)) {
                        const uint32_t* cw = codes + (size_t)tile * mw * MDB_TILE + lane;
                        float s16[16], s8[8], s4[4], s1 = 0.0f;
#pragma unroll
                        for (int x = 0; x < 16; ++x) s16[x] = 0.0f;
#pragma unroll
                        for (int x = 0; x < 8; ++x) s8[x] = 0.0f;
#pragma unroll
                        for (int x = 0; x < 4; ++x) s4[x] = 0.0f;
                        for (int w = 0; w < mw; ++w) {
                            uint32_t word = cw[(size_t)w * MDB_TILE];
#pragma unroll
                            for (int bi = 0; bi < 4; ++bi) {
                                int s = w * 4 + bi;
                                if (s < m) {
                                    uint32_t code = (word >> (8 * bi)) & 0xFFu;
                                    const float* row;
                                    const float* arow = nullptr;
                                    if (LUT_LDS) row = lut + ((size_t)s * K + code) * subdim;
                                    else {
                                        row = cb + ((size_t)s * K + code) * subdim;
                                        arow = cb + ((size_t)s * K + qc[s]) * subdim;
                                    }
                                    // per-element term, either pre-rounded (LUT) or computed here
#define MDB_TERM(acc, e) (LUT_LDS ? __fadd_rn((acc), row[(e)]) : acc_term<METRIC>((acc), arow[(e)], row[(e)]))
                                    for (int cc = 0; cc < sp.n16; ++cc)
#pragma unroll
                                        for (int x = 0; x < 16; ++x) s16[x] = MDB_TERM(s16[x], 16 * cc + x);
                                    for (int cc = 0; cc < sp.n8; ++cc)
#pragma unroll
                                        for (int x = 0; x < 8; ++x) s8[x] = MDB_TERM(s8[x], sp.off8 + 8 * cc + x);
                                    for (int cc = 0; cc < sp.n4; ++cc)
#pragma unroll
                                        for (int x = 0; x < 4; ++x) s4[x] = MDB_TERM(s4[x], sp.off4 + 4 * cc + x);
                                    if (sp.ntail > 0) {
                                        float tt = 0.0f;
                                        for (int x = 0; x < sp.ntail; ++x) tt = MDB_TERM(tt, sp.offt + x);
                                        s1 = tt;  // overwritten, not accumulated (pq/mod.rs:259-261)
                                    }
#undef MDB_TERM
                                }
                            }
                        }
                        float r = __fadd_rn(__fadd_rn(__fadd_rn(reduce_ordered<16>(s16), reduce_ordered<8>(s8)),
                                                      reduce_ordered<4>(s4)), s1);
                        float dist = METRIC == MDB_METRIC_L2 ? r : -r;
                        if (dist != dist) nan_seen = true;
                        key = make_key(dist, pid);
                        ++scored;
                    }
                }
                sel.offer(key);
                sel.round_end();
            }
        }
    }
    if (nan_seen) atomicOr(a.flags, MDB_FLAG_NAN);
    if (bad) atomicOr(a.flags, MDB_FLAG_RANGE);
    {
        unsigned long long ws = scored;  // wave total -> one atomic per wave
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ws += __shfl_xor((unsigned)ws, m);
        // one device-scope atomic per BLOCK (wave totals meet in LDS first): thousands of atomics on one cache
        // line serialise and were the largest fixed cost of a scan block
        if (lane == 0 && ws) atomicAdd(sel.spare(), (uint32_t)ws);
    }
    sel.finish();
    if (threadIdx.x == 0 && *sel.spare()) atomicAdd(&a.counters[2], (unsigned long long)*sel.spare());
    uint64_t* dst = a.partial + ((size_t)qi * nsplit + split) * a.k;
    uint32_t c = sel.count();
    for (int j = threadIdx.x; j < a.k; j += MDB_BLOCK) dst[j] = j < (int)c ? sel.buf[j] : MDB_KEY_MAX;
    if (a.counts_out && threadIdx.x == 0) a.counts_out[qi] = c;
}

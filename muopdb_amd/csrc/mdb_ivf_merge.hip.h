// mdb_ivf_merge.hip.h — device code of mdb_ivf.hip, part 4: keys -> doc-id rows (remap), the points blocks of the list-sharded search and
// their merge, and the merge of a scan's splits fused with the remap.  Included by mdb_ivf.hip only, after mdb_ivf_fused.hip.h.
#pragma once

// keys (distance, point id) -> (u128 doc id, score) rows ordered by IdWithScore (score, doc id).
// One block per query; rank sort (k <= MDB_MAX_K).
__global__ __launch_bounds__(256) void remap_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts,
                                                    int k, const IvfUserDev* __restrict__ users,
                                                    const uint32_t* __restrict__ q_user,
                                                    const uint8_t* __restrict__ index_bytes, mdb_u128* __restrict__ doc_out,
                                                    float* __restrict__ score_out, uint32_t* __restrict__ counts_out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint64_t* lo = (uint64_t*)lds;
    uint64_t* hi = lo + k;
    float* sc = (float*)(hi + k);
    const int qi = blockIdx.x;
    const IvfUserDev u = users[q_user ? q_user[qi] : 0];
    const int c = (int)counts[qi];
    for (int j = threadIdx.x; j < c; j += blockDim.x) {
        uint64_t key = keys[(size_t)qi * k + j];
        uint32_t pid = key_id(key);
        const uint64_t* dp = (const uint64_t*)(index_bytes + u.doc_ids_off + (size_t)pid * 16);
        lo[j] = dp[0];
        hi[j] = dp[1];
        sc[j] = key_dist(key);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        if (j < c) {
            int rank = 0;
            float s = sc[j];
            uint64_t l = lo[j], h = hi[j];
            for (int i = 0; i < c; ++i) {
                float si = sc[i];
                bool less = si < s || (si == s && (hi[i] < h || (hi[i] == h && (lo[i] < l || (lo[i] == l && i < j)))));
                rank += less ? 1 : 0;
            }
            doc_out[(size_t)qi * k + rank] = mdb_u128{l, h};
            score_out[(size_t)qi * k + rank] = s;
        } else {
            doc_out[(size_t)qi * k + j] = mdb_u128{~0ull, ~0ull};
            score_out[(size_t)qi * k + j] = __uint_as_float(0x7F800000u);
        }
    }
    if (threadIdx.x == 0 && counts_out) counts_out[qi] = (uint32_t)c;
}


// ------------------------------------------------------------------------------------------ exact list-sharded search (§8e)
// One rank's POINTS block: { uint32 point_ids[b][k]; float scores[b][k]; uint32 counts[b]; uint8 found[b]; pad to 16 } — its
// search_with_centroids rows (index.rs:250-286: ascending by (distance, point id)) BEFORE the doc-id remap.
__global__ __launch_bounds__(256) void pack_points_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts,
                                                          const uint8_t* __restrict__ found, int k, size_t b, uint32_t* __restrict__ pid_out,
                                                          float* __restrict__ score_out, uint32_t* __restrict__ counts_out,
                                                          uint8_t* __restrict__ found_out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b * (size_t)(k > 0 ? k : 1)) return;
    const size_t qi = k > 0 ? t / k : t;
    const int j = k > 0 ? (int)(t % k) : 0;
    const uint32_t c = counts[qi];
    if (j == 0) { counts_out[qi] = c; found_out[qi] = found ? found[qi] : (uint8_t)1; }
    if (k == 0) return;
    if ((uint32_t)j < c) { const uint64_t key = keys[t]; pid_out[t] = key_id(key); score_out[t] = key_dist(key); }
    else { pid_out[t] = 0xFFFFFFFFu; score_out[t] = __uint_as_float(0x7F800000u); }
}

// The merge of `world` points blocks, per query: the k smallest of the union by (distance, point id) — exactly the heap of
// search_with_centroids (index.rs:250-286) run over ALL probed lists, since every list is on one rank and each rank kept its
// own k smallest — and only then the doc ids and the IdWithScore order of search_with_centroids_and_remap (:298-332).  (A merge
// of already remapped rows by (score, doc id) would keep a different document when scores tie at rank k and doc ids are not
// monotone in point ids.)  Rows are ascending, so an element's rank is its own index plus one binary search per other row;
// equal keys (a point assigned to lists on two ranks) are ordered by rank.  One block per query.
__global__ __launch_bounds__(256) void merge_points_kernel(const char* __restrict__ blocks, size_t stride, int world, size_t b, int k,
                                                           const IvfUserDev* __restrict__ users, const uint32_t* __restrict__ q_user,
                                                           const uint8_t* __restrict__ index_bytes, mdb_u128* __restrict__ doc_out,
                                                           float* __restrict__ score_out, uint32_t* __restrict__ counts_out,
                                                           uint8_t* __restrict__ found_out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int cap = world * k;
    uint64_t* keys = (uint64_t*)lds;          // [world * k]
    uint64_t* lo = keys + cap;                // winners [k]
    uint64_t* hi = lo + k;
    float* sc = (float*)(hi + k);
    uint32_t* pos = (uint32_t*)(sc + k);      // [world + 1] prefix of the rows' lengths
    const size_t qi = blockIdx.x;
    const size_t o_sc = b * (size_t)k * 4, o_cnt = b * (size_t)k * 8, o_found = o_cnt + b * 4;
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int w = 0; w < world; ++w) {
            pos[w] = acc;
            const uint32_t c = ((const uint32_t*)(blocks + (size_t)w * stride + o_cnt))[qi];
            acc += c < (uint32_t)k ? c : (uint32_t)k;
        }
        pos[world] = acc;
    }
    __syncthreads();
    const int n = (int)pos[world];
    for (int t = threadIdx.x; t < cap; t += blockDim.x) {
        const int w = t / k, j = t % k;
        if ((uint32_t)j < pos[w + 1] - pos[w]) {
            const char* blk = blocks + (size_t)w * stride;
            const size_t src = qi * (size_t)k + j;
            keys[pos[w] + j] = make_key(((const float*)(blk + o_sc))[src], ((const uint32_t*)blk)[src]);
        }
    }
    __syncthreads();
    const IvfUserDev u = users[q_user ? q_user[qi] : 0];
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        int w = 0;
        while ((int)pos[w + 1] <= t) ++w;
        const uint64_t key = keys[t];
        int rank = t - (int)pos[w];
        for (int w2 = 0; w2 < world && rank < k; ++w2) {
            if (w2 == w) continue;
            int a0 = (int)pos[w2], a1 = (int)pos[w2 + 1];  // first index with key > `key` (w2 < w) / >= `key` (w2 > w)
            const int base = a0;
            while (a0 < a1) {
                const int mid = (a0 + a1) >> 1;
                const uint64_t km = keys[mid];
                if (w2 < w ? km <= key : km < key) a0 = mid + 1; else a1 = mid;
            }
            rank += a0 - base;
        }
        if (rank < k) {
            const uint64_t* dp = (const uint64_t*)(index_bytes + u.doc_ids_off + (size_t)key_id(key) * 16);
            lo[rank] = dp[0];
            hi[rank] = dp[1];
            sc[rank] = key_dist(key);
        }
    }
    __syncthreads();
    const int c = n < k ? n : k;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        if (j < c) {
            int rank = 0;
            const float s = sc[j];
            const uint64_t l = lo[j], h = hi[j];
            for (int i = 0; i < c; ++i) {
                const float si = sc[i];
                const bool less = si < s || (si == s && (hi[i] < h || (hi[i] == h && (lo[i] < l || (lo[i] == l && i < j)))));
                rank += less ? 1 : 0;
            }
            doc_out[qi * (size_t)k + rank] = mdb_u128{l, h};
            score_out[qi * (size_t)k + rank] = s;
        } else {
            doc_out[qi * (size_t)k + j] = mdb_u128{~0ull, ~0ull};
            score_out[qi * (size_t)k + j] = __uint_as_float(0x7F800000u);
        }
    }
    if (threadIdx.x == 0) {
        if (counts_out) counts_out[qi] = (uint32_t)c;
        if (found_out) found_out[qi] = ((const uint8_t*)(blocks + o_found))[qi];   // replicated centroid graphs: the same on every rank
    }
}
// merge_sorted_rows_kernel (mdb_flat.hip) + remap_kernel in ONE launch: the splits' ascending rows of a query -> its k smallest keys (ranks by
// binary search; any unsorted row: by counting), then doc ids and the IdWithScore rank sort.  Two 5 us launches and a gap of a 130 us SPANN step.
__global__ __launch_bounds__(256) void merge_rows_remap_kernel(const uint64_t* __restrict__ keys, int rows, int k, const IvfUserDev* __restrict__ users,
                                                               const uint32_t* __restrict__ q_user, const uint8_t* __restrict__ index_bytes,
                                                               uint64_t* __restrict__ keys_out, uint32_t* __restrict__ counts_mid,
                                                               mdb_u128* __restrict__ doc_out, float* __restrict__ score_out,
                                                               uint32_t* __restrict__ counts_out, const uint8_t* __restrict__ found_src,
                                                               uint8_t* __restrict__ found_dst, unsigned long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int per = rows * k, tid = threadIdx.x;
    // the step's last launch: its counters [0..3] move to [24..27] (what mdb_get_stats reads) and start the next call at zero — no memset
    // launch in front of it (every kernel that adds to them has finished: stream order)
    if (counters && blockIdx.x == 0 && tid < 4) {
        counters[24 + tid] = counters[tid];
        counters[tid] = 0ull;
    }
    uint64_t* K = (uint64_t*)lds;          // [rows * k]
    uint64_t* wk = K + per;                // [k] winners, ascending
    uint64_t* lo = wk + k;                 // [k] doc id halves
    uint64_t* hi = lo + k;
    float* sc = (float*)(hi + k);          // [k]
    __shared__ uint32_t unsorted, nvalid;
    const size_t q = blockIdx.x;
    const uint64_t* src = keys + q * per;
    if (tid == 0) { unsorted = 0; nvalid = 0; }
    for (int i = tid; i < per; i += 256) K[i] = src[i];
    __syncthreads();
    for (int i = tid; i + 1 < per; i += 256)
        if ((i + 1) % k != 0 && K[i] > K[i + 1]) unsorted = 1;
    __syncthreads();
    const bool sorted = unsorted == 0;
    for (int i = tid; i < per; i += 256) {
        const uint64_t key = K[i];
        const int row = i / k;
        int rank;
        if (sorted) {
            rank = i - row * k;
            for (int o = 0; o < rows; ++o) {
                if (o == row) continue;
                const uint64_t* R = K + o * k;
                int l = 0, h = k;   // first index whose key is not before `key` (rows below this one win ties)
                while (l < h) {
                    const int mid = (l + h) >> 1;
                    const bool before = o < row ? R[mid] <= key : R[mid] < key;
                    if (before) l = mid + 1; else h = mid;
                }
                rank += l;
            }
        } else {
            rank = 0;
            for (int t = 0; t < per; ++t) rank += (K[t] < key || (K[t] == key && t < i)) ? 1 : 0;
        }
        if (rank < k) {
            wk[rank] = key;
            if (key != MDB_KEY_MAX) atomicAdd(&nvalid, 1u);
            if (keys_out) keys_out[q * k + rank] = key;
        }
    }
    __syncthreads();
    const int c = (int)nvalid;   // (the padding keys sort last: the valid winners are wk[0 .. c))
    const IvfUserDev u = users[q_user ? q_user[q] : 0];
    for (int j = tid; j < c; j += 256) {
        const uint64_t key = wk[j];
        const uint64_t* dp = (const uint64_t*)(index_bytes + u.doc_ids_off + (size_t)key_id(key) * 16);
        lo[j] = dp[0];
        hi[j] = dp[1];
        sc[j] = key_dist(key);
    }
    __syncthreads();
    for (int j = tid; j < k; j += 256) {
        if (j < c) {
            int rank = 0;
            const float s = sc[j];
            const uint64_t l = lo[j], h = hi[j];
            for (int i = 0; i < c; ++i) {
                const float si = sc[i];
                const bool less = si < s || (si == s && (hi[i] < h || (hi[i] == h && (lo[i] < l || (lo[i] == l && i < j)))));
                rank += less ? 1 : 0;
            }
            doc_out[q * k + rank] = mdb_u128{l, h};
            score_out[q * k + rank] = s;
        } else {
            doc_out[q * k + j] = mdb_u128{~0ull, ~0ull};
            score_out[q * k + j] = __uint_as_float(0x7F800000u);
        }
    }
    if (tid == 0) {
        if (counts_mid) counts_mid[q] = (uint32_t)c;
        if (counts_out) counts_out[q] = (uint32_t)c;
        if (found_dst) found_dst[q] = found_src[q];
    }
}

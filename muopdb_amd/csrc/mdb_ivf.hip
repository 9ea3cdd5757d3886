// mdb_ivf.hip — IVF / SPANN posting-list scoring.
//
// Load (BlockBasedIvf::new_with_offset, rs/index/src/ivf/block_based/index.rs:94-138): the
// `index` and `vectors` files are uploaded to HBM in one bulk copy each; posting lists are
// Elias-Fano-decoded on the GPU (mdb_ef.hip) and the vectors are re-laid LIST-CONTIGUOUS:
// list g owns whole tiles of 64 slots; tile t stores float4 #c4 of its 64 vectors as one
// 1 KiB line (f32) or the 64 16-byte code words as one 1 KiB line (PQ m%16==0).  A point that
// sits in several lists is stored once per list (the reference does not dedup across lists
// either, index.rs:250-286).  Point ids live in a side array (4 B per slot).
//
// Search (scan_posting_list :175-237, search_with_centroids :250-286, ..._and_remap :298-332):
// one block per (query, probe-split); one thread per posting-list slot keeps the reference's
// lane association in registers (bit-exact distances); tombstones are a bitmap; the block
// keeps its k best (distance, point id) keys with BlockSelect; a merge kernel combines the
// splits; a final kernel maps point ids to u128 doc ids and orders by IdWithScore
// (score, doc id) — rs/index/src/utils.rs:95-114.
// Bound: HBM — (d*4+4) B per scored vector (NoQ) or (m+4) B (PQ), SURVEY.md §8d.
#include <type_traits>
#include <unordered_map>

#include "mdb_device.hip.h"
#include "mdb_ivf.h"
#include "mdb_kernels.h"
#include "mdb_launch.hip.h"

// the kernels, in the order they were written (this file: load, dispatch and the C ABI)
#include "mdb_ivf_scan.hip.h"
#include "mdb_ivf_pq2.hip.h"
#include "mdb_ivf_fused.hip.h"
#include "mdb_ivf_merge.hip.h"

// ------------------------------------------------------------------------------------------ IvfSet: load
// The host half — container parse, every range check, list ownership and the tile tables — is ivf_plan_files (mdb_files.cpp):
// nothing below it reads a file field that it has not bounded.
mdb_status IvfSet::load(mdb_ctx* ctx_, const uint8_t* index, size_t index_len, const uint8_t* vectors, size_t vectors_len,
                        const std::vector<std::pair<size_t, size_t>>& offsets, const mdb_quant_desc* quant,
                        uint32_t shard_rank, uint32_t shard_world) {
    IvfPlan plan;
    std::string why;
    const mdb_status st = ivf_plan_files(index, index_len, vectors, vectors_len, offsets, quant, shard_rank, shard_world, plan_opts(ctx_), plan, why);
    if (st != MDB_OK) return mdb_fail(ctx_, st, "%s", why.c_str());
    return upload(ctx_, plan, index, index_len, vectors, vectors_len, quant);
}

mdb_status IvfSet::upload(mdb_ctx* ctx_, const IvfPlan& plan, const uint8_t* index, size_t index_len, const uint8_t* vectors,
                          size_t vectors_len, const mdb_quant_desc* quant) {
    ctx = ctx_;
    kind = plan.kind;
    metric = plan.metric;
    num_features = plan.num_features;
    quantized_dimension = plan.quantized_dimension;
    const size_t U = plan.blobs.size();
    blobs = plan.blobs;
    h_users = plan.users;
    max_user_vectors = plan.max_user_vectors;
    user_points = plan.user_points;
    total_slots_valid = plan.total_slots_valid;
    const std::vector<uint64_t>&list_byte_off = plan.list_byte_off, &tile_src = plan.tile_src, &cent_tile_src = plan.cent_tile_src;
    const std::vector<uint32_t>&list_len = plan.list_len, &h_list_tile_off = plan.list_tile_off, &tile_limit = plan.tile_limit,
                               &unit_desc = plan.unit_desc, &cent_tile_first = plan.cent_tile_first, &cent_tile_limit = plan.cent_tile_limit;
    const bool units = plan.units;   // f32 lists: list_tile_off counts 16-slot units
    const size_t tomb_words = plan.tomb_words;
    G = list_len.size();
    const size_t ntiles = h_list_tile_off.back();   // (f32 lists: units)
    const size_t slots_per = units ? MDB_UNIT : MDB_TILE;
    total_tiles = plan.wave_tiles;
    // ---- uploads
    DevBuf<uint8_t> d_vec;
    if (d_index.alloc(index_len + 16) != hipSuccess || d_vec.alloc(vectors_len + 16) != hipSuccess)
        return mdb_fail(ctx, MDB_ERR_OOM, "index/vector upload alloc");
    MDB_HIP(ctx, hipMemcpyAsync(d_index.p, index, index_len, hipMemcpyHostToDevice, ctx->stream));
    MDB_HIP(ctx, hipMemcpyAsync(d_vec.p, vectors, vectors_len, hipMemcpyHostToDevice, ctx->stream));
    DevBuf<uint64_t> d_lbo, d_oo, d_tsrc, d_ctsrc;
    DevBuf<uint32_t> d_tlim, d_ctfirst, d_ctlim, d_udesc;
    std::vector<uint64_t> out_off(G);
    for (size_t g = 0; g < G; ++g) out_off[g] = (uint64_t)h_list_tile_off[g] * slots_per;
    auto up64 = [&](DevBuf<uint64_t>& d, const std::vector<uint64_t>& h) -> mdb_status {
        if (d.alloc(h.size() + 1) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "alloc");
        if (!h.empty()) MDB_HIP(ctx, hipMemcpyAsync(d.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        return MDB_OK;
    };
    auto up32 = [&](DevBuf<uint32_t>& d, const std::vector<uint32_t>& h) -> mdb_status {
        if (d.alloc(h.size() + 1) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "alloc");
        if (!h.empty()) MDB_HIP(ctx, hipMemcpyAsync(d.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        return MDB_OK;
    };
    // compact the owned, non-empty lists for the decode launch
    std::vector<uint64_t> dec_off, dec_out;
    for (size_t g = 0; g < G; ++g)
        if (list_len[g]) { dec_off.push_back(list_byte_off[g]); dec_out.push_back(out_off[g]); }
    MDB_TRY(up64(d_lbo, dec_off));
    MDB_TRY(up64(d_oo, dec_out));
    MDB_TRY(up64(d_tsrc, tile_src));
    MDB_TRY(up32(d_tlim, tile_limit));
    MDB_TRY(up64(d_ctsrc, cent_tile_src));
    MDB_TRY(up32(d_ctfirst, cent_tile_first));
    MDB_TRY(up32(d_ctlim, cent_tile_limit));
    MDB_TRY(up32(d_list_tile_off, h_list_tile_off));
    if (d_users.alloc(U + 2) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "alloc");
    MDB_HIP(ctx, hipMemcpyAsync(d_users.p, h_users.data(), (U + 1) * sizeof(IvfUserDev), hipMemcpyHostToDevice, ctx->stream));
    h_tomb.assign(tomb_words + 1, 0);
    if (d_tomb.alloc(tomb_words + 1) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "alloc");
    MDB_HIP(ctx, hipMemsetAsync(d_tomb.p, 0, (tomb_words + 1) * 4, ctx->stream));
    ones_word = tomb_words;  // the spare last word: "no planner" allow bitmap
    MDB_HIP(ctx, hipMemsetAsync(d_tomb.p + ones_word, 0xFF, 4, ctx->stream));
    // ---- decode posting lists into the slot id array
    const size_t nslots = ntiles * slots_per;
    if (d_slot_ids.alloc(nslots + 1) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "slot ids alloc");
    if (nslots) fill_u32_kernel<<<dim3((unsigned)((nslots + 255) / 256)), 256, 0, ctx->stream>>>(d_slot_ids.p, nslots, 0xFFFFFFFFu);
    MDB_TRY(ef_decode_lists(ctx, d_index.p, d_lbo.p, d_oo.p, dec_off.size(), d_slot_ids.p));
    // ---- re-lay the vectors list-contiguous
    if (kind == MDB_QUANT_PQ) {
        MDB_TRY(pq_upload(ctx, quant, pq));
        {   // the code-to-code row-sum table of the symmetric L2 distance (pq_sdc_kernel), when it is small enough to stay in L2 / MALL
            const size_t words = (size_t)pq.m * pq.K * pq.K;
            if (metric == MDB_METRIC_L2 && words && words * 4 <= (size_t)std::max<long long>(0, ctx->opt.pq_sdc_max_mb) << 20) {
                // an OPTIONAL accelerator: without it the scan blocks build their table rows themselves (sdc == nullptr), as before
                if (pq.sdc.alloc(words + 4) != hipSuccess) {
                    (void)hipGetLastError();
                    pq.sdc.release();
                } else {
                    pq_sdc_kernel<<<dim3((unsigned)((words + 255) / 256)), 256, 0, ctx->stream>>>(pq.codebook.p, pq.m, pq.K, pq.subdim, pq.sdc.p);
                    MDB_HIP(ctx, hipGetLastError());
                }
            }
        }
        mw = (pq.m + 3) / 4;
        size_t total = ntiles * MDB_TILE * (size_t)mw;
        if (d_codes.alloc(total + 4) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "code tiles alloc");
        if (total)
            gather_code_tiles_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, ctx->stream>>>(
                d_vec.p, d_tsrc.p, d_tlim.p, d_slot_ids.p, pq.m, mw, d_codes.p, total, ctx->d_flags);
    } else {
        int d4 = ((int)num_features + 3) / 4;
        size_t total4 = ntiles * MDB_UNIT * (size_t)d4;
        MDB_TRY(up32(d_udesc, unit_desc));
        if (d_tiles.alloc(total4 * 4 + 4) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "vector tiles alloc (%zu MiB)", total4 * 16 >> 20);
        if (total4)
            gather_f32_units_kernel<<<dim3((unsigned)((total4 + 255) / 256)), 256, 0, ctx->stream>>>(
                d_vec.p, d_tsrc.p, d_tlim.p, d_slot_ids.p, d_udesc.p, (int)num_features, d4, (float4*)d_tiles.p, total4, ctx->d_flags);

    }
    MDB_HIP(ctx, hipGetLastError());
    // ---- centroids into tiles (coarse quantizer scan, find_nearest_centroids)
    {
        int d4 = ((int)num_features + 3) / 4;
        size_t nct = cent_tile_src.size();
        size_t total4 = nct * MDB_TILE * (size_t)d4;
        if (d_cent_tiles.alloc(total4 * 4 + 4) != hipSuccess) return mdb_fail(ctx, MDB_ERR_OOM, "centroid tiles alloc");
        if (total4)
            gather_f32_tiles_kernel<<<dim3((unsigned)((total4 + 255) / 256)), 256, 0, ctx->stream>>>(
                d_index.p, d_ctsrc.p, d_ctlim.p, nullptr, d_ctfirst.p, (int)num_features, d4, (float4*)d_cent_tiles.p, total4,
                ctx->d_flags);
        MDB_HIP(ctx, hipGetLastError());
        // one index with a large coarse quantizer (C5: 65 536 lists): large batches of queries go through the batched flat
        // path (sample bound + matrix-core filter + exact refine) — the same probe ids, several times faster
        // one index with a mid-sized coarse quantizer (C3: 4096 lists): find_nearest_centroids — inside the fused step or alone — runs on the matrix
        // cores (mdb_ivf_coarse.hip.h); an optional accelerator — cm_build leaves it empty when memory is short
        if (U == 1 && coarse_by_scan && ctx->opt.ivf_coarse_mfma) {   // (find_nearest_centroids is sqrt-L2 whatever the index's metric: index.rs:155)
            TileView cv{d_cent_tiles.p, blobs[0].num_clusters, (blobs[0].num_clusters + MDB_TILE - 1) / MDB_TILE, (int)num_features, d4};
            MDB_TRY(cm_build(ctx, cv, cmf));
        }
        if (U == 1 && blobs[0].num_clusters >= 65536) {
            TileView cv{d_cent_tiles.p, blobs[0].num_clusters, (blobs[0].num_clusters + MDB_TILE - 1) / MDB_TILE, (int)num_features, d4};
            const size_t sdiv = (size_t)std::max<long long>(1, ctx->opt.ivf_coarse_sample_div);
            MDB_TRY(flat_build_aux(ctx, cv, cent_aux, (cv.n / MDB_TILE) / sdiv, MDB_METRIC_L2,
                                   cv.n * (size_t)cv.d * 4 <= ((size_t)std::max<long long>(0, ctx->opt.flat_rows_max_mb) << 20)));
        }
    }
    mdb_status st = mdb_check_flags(ctx);  // synchronises: temporaries may now be released
    if (st != MDB_OK) return st;
    doc_maps.resize(U);
    return MDB_OK;
}

// doc id -> point id map of one user, built on first use (BlockBasedIvf::new builds it eagerly,
// index.rs:67-73; here it is only needed by invalidate / is_invalidated)
mdb_status IvfSet::build_doc_map(size_t ui, mdb_ctx* ectx) {   // ectx: the CALLING handle's context (errors are reported there)
    mdb_ctx* const ctx = ectx;
    if (!doc_maps[ui].empty() || blobs[ui].num_vectors == 0) return MDB_OK;
    const IvfBlobInfo& bi = blobs[ui];
    std::vector<uint64_t> ids(bi.num_vectors * 2);
    MDB_HIP(ctx, hipMemcpy(ids.data(), d_index.p + bi.doc_id_mapping_offset + 16, bi.num_vectors * 16, hipMemcpyDeviceToHost));
    auto& m = doc_maps[ui];
    m.reserve(bi.num_vectors * 2);
    for (uint64_t i = 0; i < bi.num_vectors; ++i) m[U128Key{ids[2 * i], ids[2 * i + 1]}] = (uint32_t)i;  // later ids win, like HashMap::collect
    return MDB_OK;
}

// The tombstone set is ONE per resident index (`invalid_point_ids: DashSet<u32>`, index.rs:30), whatever handle it is
// reached through: the host mirror and the doc-id maps live in the root set; the device word is written on the calling
// handle's stream.
mdb_status IvfSet::invalidate(size_t ui, const mdb_u128* doc_ids, size_t n, uint8_t* flags_out, bool test_only) {
    IvfSet& r = root ? *root : *this;
    if (ui >= blobs.size()) { for (size_t i = 0; i < n; ++i) flags_out[i] = 0; return MDB_OK; }
    std::lock_guard<std::mutex> tg(r.tomb_mu);
    if (r.doc_maps[ui].empty() && r.blobs[ui].num_vectors) MDB_TRY(r.build_doc_map(ui, ctx));   // the root's ctx is never touched: its searches run meanwhile
    // a batch (the tombstone log replayed at open: thousands of records of one user) uploads the span of words it touched
    // once; words in between are rewritten with the values they have
    size_t wlo = SIZE_MAX, whi = 0;
    for (size_t i = 0; i < n; ++i) {
        auto it = r.doc_maps[ui].find(U128Key{doc_ids[i].lo, doc_ids[i].hi});
        if (it == r.doc_maps[ui].end()) { flags_out[i] = 0; continue; }
        uint32_t pid = it->second;
        size_t w = h_users[ui].tomb_base + (pid >> 5);
        uint32_t bit = 1u << (pid & 31);
        bool was = r.h_tomb[w] & bit;
        if (test_only) { flags_out[i] = was; continue; }
        flags_out[i] = !was;  // DashSet::insert returns true when newly inserted (index.rs:421-426)
        if (!was) {
            r.h_tomb[w] |= bit;
            r.tomb_any.store(1u);
            wlo = std::min(wlo, w);
            whi = std::max(whi, w);
        }
    }
    if (wlo != SIZE_MAX) {
        MDB_HIP(ctx, hipMemcpyAsync(d_tomb.p + wlo, &r.h_tomb[wlo], (whi - wlo + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
        MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MDB_OK;
}

void IvfSet::view_of(IvfSet& src, mdb_ctx* ctx2) {
    ctx = ctx2;
    root = src.root ? src.root : &src;
    kind = src.kind; metric = src.metric; num_features = src.num_features; quantized_dimension = src.quantized_dimension;
    blobs = src.blobs; h_users = src.h_users; G = src.G; total_tiles = src.total_tiles; total_slots_valid = src.total_slots_valid;
    d_index.borrow(src.d_index); d_list_tile_off.borrow(src.d_list_tile_off); d_users.borrow(src.d_users); d_tomb.borrow(src.d_tomb);
    d_slot_ids.borrow(src.d_slot_ids); d_codes.borrow(src.d_codes); d_tiles.borrow(src.d_tiles); d_cent_tiles.borrow(src.d_cent_tiles);
    pq.metric = src.pq.metric; pq.dimension = src.pq.dimension; pq.subdim = src.pq.subdim; pq.num_bits = src.pq.num_bits;
    pq.m = src.pq.m; pq.K = src.pq.K; pq.h_codebook = src.pq.h_codebook; pq.codebook.borrow(src.pq.codebook); pq.sdc.borrow(src.pq.sdc);
    mw = src.mw; ones_word = src.ones_word; max_user_vectors = src.max_user_vectors; user_points = src.user_points;
    flat_aux_view(src.cent_aux, cent_aux);
    cmf.borrow(src.cmf);
}

// allow bitmaps: bit p of bitmap i keeps point p for query i (n_bitmaps == 1: one bitmap for every query).  A bitmap
// must cover every point id a scan can meet, a per-query set every query of the batch: anything shorter would be read
// out of bounds by allow_test.
mdb_status IvfSet::stage_filter(const uint32_t* allow, size_t n_bitmaps, size_t words, mdb_mem mem, size_t b, ScanFilter* out,
                                const uint32_t* q_user) {
    *out = ScanFilter{};
    if (!allow) return MDB_OK;
    if (n_bitmaps == 0 || words == 0) return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "empty filter bitmap");
    uint64_t need = max_user_vectors;
    if (q_user) {   // only the users this call searches (unknown users — slot >= the table — scan nothing)
        const std::vector<uint64_t>& up = root ? root->user_points : user_points;
        need = 0;
        for (size_t i = 0; i < b; ++i)
            if (q_user[i] < up.size()) need = std::max(need, up[q_user[i]]);
    }
    if (words < (need + 31) / 32)
        return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "filter bitmaps of %zu words do not cover %zu point ids", words, (size_t)need);
    if (n_bitmaps != 1 && n_bitmaps < b)
        return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "%zu filter bitmaps for a batch of %zu queries", n_bitmaps, b);
    if (n_bitmaps != 1) n_bitmaps = b;
    out->n_bitmaps = n_bitmaps;
    out->words = words;
    if (mem == MDB_MEM_DEVICE) { out->allow = allow; return MDB_OK; }
    const size_t bytes = n_bitmaps * words * 4;
    void *pin, *dev;
    MDB_TRY(mdb_pinned(ctx, MDB_PIN_FILTER, bytes, &pin));
    memcpy(pin, allow, bytes);
    MDB_TRY(mdb_scratch(ctx, bytes, &dev));
    MDB_HIP(ctx, hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    out->allow = (const uint32_t*)dev;
    return MDB_OK;
}

// ------------------------------------------------------------------------------------------ IvfSet: search
// the filter's and the tombstones' part of a scan's arguments, for IvfSet::scan and IvfSet::search_fused alike
mdb_status IvfSet::scan_masks(const ScanFilter* filter, size_t b, ScanMasks* out) const {
    static const ScanFilter no_filter{};
    const ScanFilter& f = filter && filter->allow ? *filter : no_filter;
    if (f.allow && f.n_bitmaps != 1 && f.n_bitmaps < b)
        return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "%zu filter bitmaps for a batch of %zu queries", f.n_bitmaps, b);
    out->allow = f.allow ? f.allow : d_tomb.p + ones_word;
    out->allow_stride = f.allow && f.n_bitmaps != 1 ? (uint32_t)f.words : 0u;
    out->allow_mask = f.allow ? 0xFFFFFFFFu : 0u;
    out->no_masks = (!f.allow && (root ? root : this)->tomb_any.load() == 0u && !ctx->opt.scan_masks_always) ? 1u : 0u;
    return MDB_OK;
}

// d_q: staged queries [b][qstride]; probes: device [b][probe_stride]; outputs: device keys [b][k] + counts
mdb_status IvfSet::scan(const float* d_q, int qstride, size_t b, const uint32_t* d_q_user, const uint32_t* d_probes,
                        const uint32_t* d_probe_cnt, int probe_stride, size_t k, uint64_t* d_keys, uint32_t* d_counts,
                        const ScanFilter* filter, ScanRemap* rm) {
    if (b == 0) return MDB_OK;
    ctx->counters_clean = false;   // this writes d_counters[0..3]: whoever relies on "still zero from the last call" (spann_search_impl) re-arms the flag AFTER it
    if (k > MDB_MAX_K) return mdb_fail(ctx, MDB_ERR_UNSUPPORTED, "k=%zu exceeds MDB_MAX_K=%d", k, MDB_MAX_K);
    ScanMasks sm;
    MDB_TRY(scan_masks(filter, b, &sm));
    int nsplit = 1;
    if (probe_stride > 1) {
        size_t want = (1024 + b - 1) / b;  // aim for >= ~1024 blocks
        nsplit = (int)std::min<size_t>(std::max<size_t>(want, 1), (size_t)probe_stride);
        nsplit = std::min(nsplit, 64);
    }
    if (kind != MDB_QUANT_PQ && probe_stride > 1) {
        // f32 posting lists: a block's four waves take one tile each per round, so a query wants about (its tiles) / 4 blocks — all of
        // its tiles stream at once and no block waits through a last round with one busy wave.  The tiles of a query are estimated on
        // the host: average tiles per list x probes (x 0.6 when a ratio filter trims the probe lists: SPANN).  Full C4 (1024 queries of
        // ~9 lists): 1 block per query 0.522 ms per step, 3: 0.493, 5: 0.488, 4 (= 3 + an empty block each): 0.521, 12: 0.595.
        const double tiles = (double)total_tiles / (double)std::max<size_t>(G, 1) * probe_stride;   // (a split beyond a query's tiles returns at once)
        // small batches (one or two resident blocks per CU at 219 registers): blocks of TWO waves, so that twice as many of a query's
        // tiles stream at once (C4 at 128 users, same box: 4-wave blocks x 8 splits 0.1183 ms per step, 2-wave x 12 0.1123, x 16 0.1120)
        const int wpb = (b <= 256 && !ctx->opt.scan_f32_blk) ? 2 : ((int)ctx->opt.scan_f32_blk == 64 ? 1 : ((int)ctx->opt.scan_f32_blk == 128 ? 2 : 4));
        const int by_tiles = (int)std::min<double>(16.0, std::max(1.0, std::ceil(tiles / (double)wpb)));
        nsplit = std::min(std::max(nsplit, by_tiles), probe_stride);
        if (ctx->opt.scan_f32_nsplit > 0) nsplit = (int)std::min<long long>(ctx->opt.scan_f32_nsplit, probe_stride);
    }
    // PQ fast path (ivf_scan_pq2_kernel): compile-time subvector width, table + selector + tile map in LDS
    size_t pq2_lds = 0, pq2_lds_f = 0;
    bool pq2 = false, pq2_filt = false, pq_full = false;
    if (kind == MDB_QUANT_PQ && !ctx->opt.pq_no_fast) {
        pq2_lds = ((BlockSelect<PQ2_BLOCK>::lds_bytes((int)k) + 15) & ~(size_t)15) + (2 * PQ2_PCH + 16) * 4 +
                  (size_t)pq.m * pq.subdim * 4 + (size_t)pq.m * pq.K * pq.subdim * 4;
        pq2 = (pq.subdim == 4 || pq.subdim == 8 || pq.subdim == 16 || pq.subdim == 32) && (mw == 1 || mw == 2 || mw == 4 || mw == 8) &&
              pq.K == (1 << pq.num_bits) && pq.num_bits <= 8 && pq2_lds <= 160 * 1024 - 256;
        // L2: bound filter in front of the exact row sums (ivf_scan_pq2_kernel<.., FILT>) when its table fits too
        pq2_lds_f = pq2_lds + (size_t)pq.m * pq.K * 2;
        pq2_filt = pq2 && metric == MDB_METRIC_L2 && pq2_lds_f <= 160 * 1024 - 256 && !ctx->opt.pq_no_filter;
        pq_full = pq.m == 4 * mw && pq.num_bits == 8 && !ctx->opt.pq_no_full;
        if (pq2) {  // one block per CU (LDS).  More, shorter blocks do NOT balance skewed lists better here: the hardware
            // dispatches 150 KB-LDS workgroups in order, so CUs idle between blocks (measured: 256 blocks 98 us,
            // 512 blocks 140 us, 1024 blocks 247 us for the same work)
            const size_t target = (size_t)std::max<long long>(1, ctx->opt.pq_blocks);
            nsplit = (int)std::min<size_t>(std::max<size_t>((target + b - 1) / b, 1), 16);
        }
    }
    // one block per query: its sorted keys ARE the result — written in place, no merge launch
    const bool direct = nsplit == 1 && k > 0;
    void* partial = d_keys;
    if (!direct) MDB_TRY(mdb_scratch(ctx, b * (size_t)nsplit * std::max<size_t>(k, 1) * 8, &partial));
    ScanArgs a{d_users.p, d_q_user, d_list_tile_off.p, d_slot_ids.p, d_tomb.p, d_probes, d_probe_cnt, probe_stride,
               (int)k, (uint64_t*)partial, ctx->d_flags, ctx->d_counters,
               sm.allow, sm.allow_stride, sm.allow_mask,
               direct ? d_counts : nullptr, nullptr, (int)ctx->opt.pq_eager_trim};
    a.no_masks = sm.no_masks;
    dim3 grid((unsigned)nsplit, (unsigned)b);
    size_t sel_lds = BlockSelect<MDB_BLOCK>::lds_bytes((int)k);
    void* qcodes = nullptr;
    if (kind == MDB_QUANT_PQ) {
        MDB_TRY(mdb_scratch(ctx, b * (size_t)pq.m + 16, &qcodes));
        MDB_TRY(pq_quantize_device(ctx, pq, d_q, b, (uint8_t*)qcodes, qstride));  // Q::QuantizedT::process_vector, index.rs:193
    }
    {
    ProfScope prof(ctx);
    if (kind == MDB_QUANT_PQ) {
        DistPlan sp = make_plan(pq.subdim, MDB_METRIC_L2);
        size_t lut_bytes = (size_t)pq.m * pq.K * pq.subdim * 4;
        size_t lds_lut = ((sel_lds + 15) & ~(size_t)15) + lut_bytes;
        bool use_lut = lds_lut <= 150 * 1024;
        // two-phase scan (ivf_scan_pq3_kernel + ivf_pq3_refine_kernel) for batches of several one-phase blocks per CU: bounds at
        // four 512-thread blocks per CU, exact distances for the candidates only; the one-phase launch behind it is gated on the
        // candidate lists' overflow word.  (At batch 256 — one one-phase block per CU, C3 — the two extra launches and the second
        // pass over the candidates cost more than the table build they save: 0.113 vs 0.105 ms per step.)
        const size_t pq3_min_b = (size_t)std::max<long long>(0, ctx->opt.pq_two_phase_min_b);
        const bool pq3 = pq2 && metric == MDB_METRIC_L2 && direct && k <= 64 && b >= pq3_min_b && !ctx->opt.pq_no_two_phase;
        const float* sdc_tab = ctx->opt.pq_sdc_max_mb > 0 ? pq.sdc.p : nullptr;   // (MDB_PQ_SDC_MAX_MB=0 at search time: the in-block build)
        if (pq3) {
            const size_t tgt3 = (size_t)std::max<long long>(1, ctx->opt.pq3_blocks);
            const int ns3 = (int)std::min<size_t>(std::max<size_t>((tgt3 + b - 1) / b, 1), std::min<size_t>(16, (size_t)std::max(probe_stride, 1)));
            const uint32_t cap3 = (uint32_t)std::max<long long>(1, ctx->opt.pq3_cap);   // (tests force the overflow path)
            uint32_t *cand, *ccnt;
            MDB_TRY(mdb_scratch(ctx, b * (size_t)ns3 * cap3 * 4 * (1 + (size_t)mw), (void**)&cand));
            MDB_TRY(mdb_scratch(ctx, b * (size_t)ns3 * 4 + 512, (void**)&ccnt));
            uint32_t* ovf3 = ccnt + ((b * (size_t)ns3 + 63) / 64) * 64;   // own 256-byte line
            MDB_HIP(ctx, hipMemsetAsync(ovf3, 0, 4, ctx->stream));
            const Pq3Args c3{cand, ccnt, cap3, ovf3};
            const int blk3 = (int)ctx->opt.pq3_block;   // C5 shard: 1024 -> 0.76 ms, 512 -> 0.48, 256 -> 0.49
            const size_t sel3 = blk3 == 1024 ? BlockSelect<1024>::lds_bytes((int)k) : BlockSelect<512>::lds_bytes((int)k);
            const size_t lds3 = ((sel3 + 15) & ~(size_t)15) + (2 * PQ2_PCH + 16) * 4 + (size_t)pq.m * pq.subdim * 4 + (size_t)pq.m * pq.K * 4;
            const size_t ldsr = ((BlockSelect<256>::lds_bytes((int)k) + 15) & ~(size_t)15) + (size_t)pq.m * pq.subdim * 4;
            ScanArgs a3 = a;
            a3.counts_out = nullptr;
            a3.eager_trim = (a.eager_trim & 0xFF) | ((int)std::min<long long>(255, std::max<long long>(0, ctx->opt.pq3_warm_rounds)) << 8);
            MDB_TRY(mdb_pick<1, 2, 4, 8>(mw, [&](auto MW) {
                return mdb_pick<1024, 512>(blk3, [&](auto BLK) {
                    return mdb_pick_bool(pq_full, [&](auto FULL) {
                        return mdb_launch(ctx, ivf_scan_pq3_kernel<MW(), BLK(), FULL()>, dim3((unsigned)ns3, (unsigned)b), BLK(), lds3, a3, d_codes.p, pq.m,
                                          pq.num_bits, pq.subdim, pq.codebook.p, (uint8_t*)qcodes, c3, sdc_tab);
                    });
                });
            }));
            MDB_HIP(ctx, hipGetLastError());
            MDB_TRY(mdb_pick<1, 2, 4, 8>(mw, [&](auto MW) {
                return mdb_pick<4, 8, 16, 32>(pq.subdim, [&](auto SD) {
                    return mdb_pick_bool(pq_full, [&](auto FULL) {
                        if constexpr (!FULL() || SD() * MW() <= 32)   // (as the one-phase scan below: pq2, and so pq3, is off beyond)
                            return mdb_launch(ctx, ivf_pq3_refine_kernel<SD(), MW(), FULL()>, dim3((unsigned)b), 256, ldsr, a, d_codes.p, pq.m, pq.num_bits,
                                              pq.codebook.p, (uint8_t*)qcodes, c3, ns3);
                        else return MDB_OK;
                    });
                });
            }));
            MDB_HIP(ctx, hipGetLastError());
            a.gate = ovf3;
        }
        if (pq2) {
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(metric, [&](auto M) {
                return mdb_pick<1, 2, 4, 8>(mw, [&](auto MW) {
                    return mdb_pick<4, 8, 16, 32>(pq.subdim, [&](auto SD) {
                        return mdb_pick_bool(pq_full, [&](auto FULL) {
                            // (whole-word 8-bit codes mean K = 256 and m = 4 MW: a codebook of SD * MW * 4 KB, which fits pq2_lds up to SD * MW = 32 —
                            // the wider FULL instantiations could never be selected and are not compiled)
                            if constexpr (!FULL() || SD() * MW() <= 32) {
                                if (M() == MDB_METRIC_L2 && pq2_filt)
                                    return mdb_launch(ctx, ivf_scan_pq2_kernel<M(), SD(), MW(), M() == MDB_METRIC_L2, FULL()>, grid, PQ2_BLOCK, pq2_lds_f, a,
                                                      d_codes.p, pq.m, pq.num_bits, pq.codebook.p, (uint8_t*)qcodes);
                                return mdb_launch(ctx, ivf_scan_pq2_kernel<M(), SD(), MW(), false, FULL()>, grid, PQ2_BLOCK, pq2_lds, a, d_codes.p, pq.m,
                                                  pq.num_bits, pq.codebook.p, (uint8_t*)qcodes);
                            } else return MDB_OK;
                        });
                    });
                });
            }));
        } else {
            MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(metric, [&](auto M) {
                return mdb_pick_bool(use_lut, [&](auto LUT) {
                    return mdb_launch(ctx, ivf_scan_pq_kernel<M(), LUT()>, grid, MDB_BLOCK, use_lut ? lds_lut : sel_lds, a, d_codes.p, pq.m, mw, pq.K,
                                      pq.subdim, sp, pq.codebook.p, (uint8_t*)qcodes);
                });
            }));
        }
    } else {
        DistPlan p = make_plan((int)num_features, metric);
        const int fblk = (int)ctx->opt.scan_f32_blk == 64 ? 64 : (((int)ctx->opt.scan_f32_blk == 128 || (b <= 256 && !ctx->opt.scan_f32_blk)) ? 128 : MDB_BLOCK);
        const size_t fsel = fblk == 64 ? BlockSelect<64>::lds_bytes((int)k) : (fblk == 128 ? BlockSelect<128>::lds_bytes((int)k) : sel_lds);
        const size_t f32_lds = ((fsel + 15) & ~(size_t)15) + TileMap::lds_bytes();
        MDB_TRY(mdb_pick<MDB_METRIC_L2, MDB_METRIC_DOT>(metric, [&](auto M) {
            return mdb_pick<64, 128, MDB_BLOCK>(fblk, [&](auto BLK) {
                return mdb_launch(ctx, ivf_scan_f32_kernel<M(), BLK()>, grid, BLK(), f32_lds, a, (const float4*)d_tiles.p, p, d_q, qstride);
            });
        }));
    }
    }
    MDB_HIP(ctx, hipGetLastError());
    if (!direct) {   // the splits' rows are sorted: ranks by binary search when they fit LDS, the selector merge otherwise
        const size_t mr_lds = (size_t)nsplit * k * 8 + k * 28 + 16;
        if (rm && rm->doc_out && k > 0 && mr_lds <= 48 * 1024 && !ctx->opt.scan_no_fused_remap) {
            merge_rows_remap_kernel<<<dim3((unsigned)b), 256, mr_lds, ctx->stream>>>((const uint64_t*)partial, nsplit, (int)k, d_users.p, d_q_user, d_index.p,
                                                                                    d_keys, d_counts, rm->doc_out, rm->score_out, rm->counts_out,
                                                                                    rm->found_src, rm->found_dst, rm->save_counters ? ctx->d_counters : nullptr);
            MDB_HIP(ctx, hipGetLastError());
            rm->done = true;
        } else
        if (k > 0 && (size_t)nsplit * k * 8 <= 48 * 1024) MDB_TRY(merge_sorted_rows(ctx, (const uint64_t*)partial, (size_t)nsplit, k, b, d_keys, d_counts, nullptr, nullptr));
        else MDB_TRY(merge_keys(ctx, (const uint64_t*)partial, (size_t)nsplit * k, b, k, d_keys, d_counts));
    }
    return MDB_OK;
}

// The fused small-batch step (ivf_pq_fused_kernel): one index, L2 PQ with 8-bit codes in whole 4-byte words, k and probes
// within one wave, batches below the two-phase scan's range (from there on several blocks per CU pay off).
bool IvfSet::fused_ok(size_t b, size_t k, size_t num_probes, bool have_probes) const {
    if (ctx->opt.pq_no_fused || kind != MDB_QUANT_PQ || metric != MDB_METRIC_L2 || blobs.size() != 1) return false;
    if (pq.num_bits != 8 || pq.K != 256 || pq.m != 4 * mw || !(mw == 1 || mw == 2 || mw == 4 || mw == 8)) return false;
    if (!(pq.subdim == 4 || pq.subdim == 8 || pq.subdim == 16 || pq.subdim == 32)) return false;
    if (k < 1 || k > 64 || num_probes < 1 || num_probes > 64 || b == 0) return false;
    if (b >= (size_t)std::max<long long>(1, ctx->opt.pq_two_phase_min_b) && !ctx->opt.pq_no_two_phase) return false;
    if (!have_probes && (num_probes > blobs[0].num_clusters || blobs[0].num_clusters > 16384)) return false;
    return true;
}

mdb_status IvfSet::search_fused(const float* d_q, int qstride, size_t b, const uint32_t* d_probes, size_t num_probes, size_t k,
                                const ScanFilter* filter, uint64_t* d_keys, uint32_t* d_counts, mdb_u128* d_doc, float* d_score,
                                uint32_t* d_doc_counts) {
    ctx->counters_clean = false;   // this writes d_counters[0..3]: whoever relies on "still zero from the last call" (spann_search_impl) re-arms the flag AFTER it
    ScanMasks sm;
    MDB_TRY(scan_masks(filter, b, &sm));
    const int par = ctx->fused_parity;
    ctx->fused_parity ^= 1;
    ctx->counter_base = 16 + 4 * par;
    ScanArgs a{d_users.p, nullptr, d_list_tile_off.p, d_slot_ids.p, d_tomb.p, d_probes, nullptr, (int)num_probes,
               (int)k, d_keys, ctx->d_flags, ctx->d_counters + ctx->counter_base,
               sm.allow, sm.allow_stride, sm.allow_mask,
               d_counts, nullptr, 1};
    const IvfBlobInfo& bi = blobs[0];
    const int d4 = ((int)num_features + 3) / 4;
    const bool coarse_here = d_probes == nullptr;
    FusedArgs fa{};
    fa.q = d_q;
    fa.qstride = qstride;
    fa.cent_tiles = (const float4*)(d_cent_tiles.p + (size_t)h_users[0].cent_tile_base * MDB_TILE * d4 * 4);
    fa.num_clusters = bi.num_clusters;
    fa.cent_ntiles = (bi.num_clusters + MDB_TILE - 1) / MDB_TILE;
    fa.cp = make_plan((int)num_features, MDB_METRIC_L2);
    fa.sp = make_plan(pq.subdim, MDB_METRIC_L2);
    fa.num_probes = (int)num_probes;
    fa.index_bytes = d_index.p;
    fa.doc_out = d_doc;
    fa.score_out = d_score;
    fa.doc_counts_out = d_doc_counts;
    fa.zero4 = ctx->d_counters + 16 + 4 * (par ^ 1);
    fa.b = (uint32_t)b;
    fa.m = (uint32_t)pq.m;
    fa.tile_groups = (fa.cent_ntiles + 3) / 4;
    fa.no_masks = sm.no_masks;
    // coarse search of this step: 0 probes given, 1 every distance exactly (ivf_prep_kernel -> [B][L]), 2 matrix-core filter + candidates
    int coarse_mode = !coarse_here ? 0
                      : cm_usable(cmf, ctx, d_q, qstride, b, num_probes) ? 2 : 1;
    if (coarse_mode == 2 && ctx->opt.cm_split) {
        // the coarse search as its own two launches (filter + one small block per query: ivf_coarse_rank_kernel), the fused kernel takes the probes
        void* pr;
        MDB_TRY(mdb_scratch(ctx, b * num_probes * 4, &pr));
        MDB_TRY(cm_find_nearest(ctx, cmf, (const float4*)(d_cent_tiles.p + (size_t)h_users[0].cent_tile_base * MDB_TILE * d4 * 4), make_plan((int)num_features, MDB_METRIC_L2),
                                d_q, qstride, b, num_probes, (uint32_t*)pr, nullptr));
        a.probes = (const uint32_t*)pr;
        coarse_mode = 0;
    }
    fa.coarse_blocks = coarse_mode == 1 ? fa.tile_groups * (uint32_t)((b + PQF_QT - 1) / PQF_QT) : 0u;
    void *cdist = nullptr, *qcodes;
    if (coarse_mode == 1) MDB_TRY(mdb_scratch(ctx, b * (size_t)fa.cent_ntiles * MDB_TILE * 4, &cdist));
    CoarseShape csh{};
    if (coarse_mode == 2) {
        csh = cm_shape(cmf, b, num_probes, (uint32_t)PQF_CAP);
        void *cand, *ccnt;
        MDB_TRY(mdb_scratch(ctx, b * (size_t)csh.S * csh.caps * 8, &cand));
        MDB_TRY(mdb_scratch(ctx, b * (size_t)(csh.S + 1) * 4 + 16, &ccnt));
        fa.cm_global = ctx->opt.cm_global_bound ? 1u : 0u;
        fa.cm_kappa = cmf.kappa;
        fa.cm_xnmax = cmf.xnmax;
        fa.cm_cand = (const uint2*)cand;
        fa.cm_cnt = (const uint32_t*)ccnt;
        fa.cent_rows = cmf.rows.p;
        fa.cm_S = csh.S;
        fa.cm_caps = csh.caps;
    }
    MDB_TRY(mdb_scratch(ctx, b * (size_t)pq.m + 16, &qcodes));
    fa.cdist = (float*)cdist;
    fa.qcodes = (uint8_t*)qcodes;
    if (ctx->opt.pqf_dbg) {
        void* dbg;
        MDB_TRY(mdb_scratch(ctx, 256, &dbg));
        MDB_HIP(ctx, hipMemsetAsync(dbg, 0, 256, ctx->stream));
        fa.dbg = (unsigned long long*)dbg;
    }
    const uint32_t cap_max = mw == 8 ? 1024u : (uint32_t)PQF_CAP;   // (1 + MW) words per candidate: 8 code words leave room for 1 024
    fa.cap = (uint32_t)std::min<long long>(cap_max, std::max<long long>(1, ctx->opt.pqf_cap));
    fa.cand_words = (cap_max * (1u + (uint32_t)mw) + 1u) & ~1u;
    // launch 1: every (query, centroid) distance + the queries' codes
    const bool quant_in_prep = ctx->opt.pqf_quant_in_prep != 0;
    const unsigned quant_blocks = quant_in_prep ? (unsigned)((b * (size_t)pq.m + 3) / 4) : 0u;
    fa.quant_blocks = quant_blocks;
    // coarse search on the matrix cores: its launch also quantizes the queries (blocks behind the coarse ones, on the CUs those leave idle)
    const bool quant_in_coarse = coarse_mode == 2 && !quant_in_prep && !ctx->opt.pqf_no_quant_in_coarse && pq.K == 256 && (pq.subdim & 3) == 0;
    if (!quant_in_prep && !quant_in_coarse) fa.qcodes = nullptr;
    if (coarse_mode == 2) {
        CoarseQuant cq;
        if (quant_in_coarse) { cq.cb = pq.codebook.p; cq.qcodes = (uint8_t*)qcodes; cq.m = (uint32_t)pq.m; cq.sp = fa.sp; }
        MDB_TRY(cm_launch(ctx, cmf, d_q, qstride, b, num_probes, csh, const_cast<uint2*>(fa.cm_cand), const_cast<uint32_t*>(fa.cm_cnt), cq));
    }
    const size_t prep_lds = coarse_mode == 1 ? (size_t)PQF_QT * (d4 * 4 + 16) * 4 : 0;
    if (fa.coarse_blocks + quant_blocks)
        MDB_TRY(mdb_launch(ctx, ivf_prep_kernel, dim3(fa.coarse_blocks + quant_blocks), 256, prep_lds, fa, d_q, pq.codebook.p, fa.cdist, (uint8_t*)qcodes,
                           ctx->d_flags));
    MDB_HIP(ctx, hipGetLastError());
    // launch 2: one block per query
    const size_t sel_bytes = (BlockSelect<PQF_BLOCK>::lds_bytes((int)std::max(k, num_probes)) + 15) & ~(size_t)15;
    const size_t lds = (64 + 2 * (PQF_NB + 32) + 16 + 80 + 64 + 80 + 64 + 32) * 4 + (size_t)pq.m * pq.subdim * 4 + (size_t)pq.m * 256 * 4 + (size_t)fa.cand_words * 4 +
                       PQF_CAP * 8 + 64 * 8 * 3 + 64 * 4 + sel_bytes;
    const float* sdc_tab = ctx->opt.pq_sdc_max_mb > 0 ? pq.sdc.p : nullptr;   // (MDB_PQ_SDC_MAX_MB=0 at search time: the in-block build)
    {
    ProfScope prof(ctx);
    MDB_TRY(mdb_pick<1, 2, 4, 8>(mw, [&](auto MW) {
        return mdb_pick<4, 8, 16, 32>(pq.subdim, [&](auto SD) {
            return mdb_pick<1, 0, 2>(coarse_mode, [&](auto CO) {
                if constexpr (CO() != 2 || cm_dim_ok(SD() * 4 * MW()))   // (d = SD * 4 MW here: cm_build serves no other)
                    return mdb_launch(ctx, ivf_pq_fused_kernel<SD(), MW(), CO()>, dim3((unsigned)b), PQF_BLOCK, lds, a, fa, d_codes.p, pq.codebook.p, sdc_tab);
                else return MDB_OK;
            });
        });
    }));
    }
    MDB_HIP(ctx, hipGetLastError());
    if (fa.dbg) {
        unsigned long long h[16];
        MDB_HIP(ctx, hipMemcpyAsync(h, fa.dbg, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
        MDB_HIP(ctx, hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[pqf] b=%zu P=%zu k=%zu cycles: quantize %llu probes %llu (load %llu kth %llu append %llu rank %llu) table %llu bounds %llu (fetch %llu tomb %llu lookup %llu kth %llu "
                "append %llu) exact %llu rank %llu remap %llu total %llu\n", b, num_probes, k,
                h[7] - h[0], h[1] - h[0], h[8] - h[0], h[9] - h[8], h[10] - h[9], h[1] - h[10], h[2] - h[1], h[3] - h[2], h[11] - h[2], h[12] - h[11], h[13] - h[12], h[14] - h[13], h[3] - h[14],
                h[4] - h[3], h[5] - h[4], h[6] - h[5], h[6] - h[0]);
    }
    return MDB_OK;
}

mdb_status IvfSet::remap(const uint64_t* d_keys, const uint32_t* d_counts, size_t b, size_t k, const uint32_t* d_q_user,
                         mdb_u128* d_doc, float* d_score, uint32_t* d_counts_out) {
    if (b == 0) return MDB_OK;
    size_t lds = std::max<size_t>(k, 1) * 20 + 16;
    remap_kernel<<<dim3((unsigned)b), 256, lds, ctx->stream>>>(d_keys, d_counts, (int)k, d_users.p, d_q_user, d_index.p, d_doc,
                                                              d_score, d_counts_out);
    MDB_HIP(ctx, hipGetLastError());
    return MDB_OK;
}

size_t mdb_points_block_bytes_impl(size_t b, size_t k) { return align_up(b * k * 8 + b * 4 + b, 16); }

mdb_status IvfSet::pack_points(const uint64_t* d_keys, const uint32_t* d_counts, const uint8_t* d_found, size_t b, size_t k, void* d_block) {
    if (b == 0) return MDB_OK;
    char* p = (char*)d_block;
    const size_t total = b * std::max<size_t>(k, 1);
    pack_points_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, ctx->stream>>>(
        d_keys, d_counts, d_found, (int)k, b, (uint32_t*)p, (float*)(p + b * k * 4), (uint32_t*)(p + b * k * 8), (uint8_t*)(p + b * k * 8 + b * 4));
    MDB_HIP(ctx, hipGetLastError());
    return MDB_OK;
}

mdb_status IvfSet::pack_points_to_host(const uint64_t* d_keys, const uint32_t* d_counts, const uint8_t* d_found, size_t b, size_t k, void* h_block) {
    const size_t nb = mdb_points_block_bytes_impl(b, k), used = b * k * 8 + b * 5;
    void* dblk;
    MDB_TRY(mdb_scratch(ctx, nb, &dblk));
    if (nb > used) MDB_HIP(ctx, hipMemsetAsync((char*)dblk + used, 0, nb - used, ctx->stream));
    MDB_TRY(pack_points(d_keys, d_counts, d_found, b, k, dblk));
    const HostCopy back[1] = {{h_block, dblk, nb}};
    return mdb_return_to_host(ctx, back, 1);
}

mdb_status IvfSet::merge_points(const void* d_blocks, size_t world, size_t b, size_t k, const uint32_t* d_q_user, mdb_u128* d_doc,
                                float* d_score, uint32_t* d_counts_out, uint8_t* d_found_out) {
    if (b == 0) return MDB_OK;
    const size_t stride = mdb_points_block_bytes_impl(b, k);
    if (k == 0) {
        if (d_counts_out) MDB_HIP(ctx, hipMemsetAsync(d_counts_out, 0, b * 4, ctx->stream));
        if (d_found_out) MDB_HIP(ctx, hipMemcpyAsync(d_found_out, (const char*)d_blocks + b * 4, b, hipMemcpyDeviceToDevice, ctx->stream));
        return MDB_OK;
    }
    const size_t lds = world * k * 8 + k * 20 + (world + 1) * 4 + 16;
    if (lds > 150 * 1024) return mdb_fail(ctx, MDB_ERR_UNSUPPORTED, "world*k=%zu rows exceed the on-chip merge capacity", world * k);
    MDB_TRY(mdb_launch(ctx, merge_points_kernel, dim3((unsigned)b), 256, lds, (const char*)d_blocks, stride, (int)world, b, (int)k, d_users.p, d_q_user,
                       d_index.p, d_doc, d_score, d_counts_out, d_found_out));
    MDB_HIP(ctx, hipGetLastError());
    return MDB_OK;
}

// find_nearest_centroids (index.rs:147-163) for user `ui`: sqrt-L2 to every centroid, the
// num_probes nearest ordered by (distance, index) [ties: the reference's select_nth_unstable +
// stable sort leave equal distances implementation-defined; this path orders them by index]
mdb_status IvfSet::coarse(size_t ui, const float* d_q, int qstride, size_t b, size_t num_probes, uint32_t* d_probes, bool zero_counters,
                          size_t bpad) {
    ctx->counters_clean = false;   // this writes d_counters[0..3]: whoever relies on "still zero from the last call" (spann_search_impl) re-arms the flag AFTER it
    const IvfBlobInfo& bi = blobs[ui];
    if (num_probes == 0 || num_probes > bi.num_clusters)
        return mdb_fail(ctx, MDB_ERR_OUT_OF_RANGE, "num_probes=%zu out of range (num_clusters=%u): the reference panics in select_nth_unstable_by",
                        num_probes, bi.num_clusters);
    int d4 = ((int)num_features + 3) / 4;
    TileView cv{d_cent_tiles.p + (size_t)h_users[ui].cent_tile_base * MDB_TILE * d4 * 4, bi.num_clusters,
                (bi.num_clusters + MDB_TILE - 1) / MDB_TILE, (int)num_features, d4};
    void* keys;
    MDB_TRY(mdb_scratch(ctx, b * num_probes * 8, &keys));
    if (ui == 0 && cm_usable(cmf, ctx, d_q, qstride, b, num_probes)) {
        // mid-sized coarse quantizer of one L2 PQ index: matrix-core filter + exact candidates (mdb_ivf_coarse.hip.h), the same ids
        return cm_find_nearest(ctx, cmf, (const float4*)cv.data, make_plan((int)num_features, MDB_METRIC_L2), d_q, qstride, b, num_probes, d_probes,
                               zero_counters ? ctx->d_counters : nullptr);
    }
    if (ui == 0 && cent_aux.sample.n && bpad >= (b + 63) / 64 * 64 && flat_mfma_applicable(ctx, cv, cent_aux, b, num_probes)) {
        // the path's last merge writes the probe (centroid) ids itself and clears the context's device counters
        const UnpackOut up{d_probes, nullptr, nullptr, zero_counters ? ctx->d_counters : nullptr};
        MDB_TRY(flat_topk_keys_mfma(ctx, cv, cent_aux, MDB_METRIC_L2, d_q, qstride, b, bpad, num_probes, (uint64_t*)keys, nullptr, false, &up));
        return MDB_OK;
    }
    // always L2 (:155); the merge kernel writes the probe (centroid) ids itself: num_probes <= num_clusters, so every row is full
    const UnpackOut up{d_probes, nullptr, nullptr, zero_counters ? ctx->d_counters : nullptr};
    MDB_TRY(flat_topk_keys(ctx, cv, MDB_METRIC_L2, d_q, qstride, b, num_probes, (uint64_t*)keys, nullptr, false, nullptr, &up));
    return MDB_OK;
}

// ============================================================================================
// C ABI: single IVF
// ============================================================================================
struct mdb_ivf {
    IvfSet set;
    mdb_ivf* parent = nullptr;   // attached handle: the owner of the device arrays
    std::atomic<int> refs{1};    // this handle + the handles attached to it
};

static void ivf_release(mdb_ivf* h) {
    if (h->refs.fetch_sub(1) != 1) return;
    mdb_ctx* ctx = h->set.ctx;
    mdb_ivf* parent = h->parent;
    (void)hipSetDevice(ctx->device);
    delete h;
    mdb_ctx_release(ctx);
    if (parent) ivf_release(parent);
}

struct FilterArg { const uint32_t* allow; size_t n_bitmaps, words; };

// mode: OUT_POINTS = point ids + distances (search_with_centroids), OUT_DOCS = doc ids + scores (.._and_remap),
// OUT_BLOCK = this rank's points block for the exact sharded merge (ids_out = the block, scores_out / counts_out unused)
enum { OUT_POINTS = 0, OUT_DOCS = 1, OUT_BLOCK = 2 };
static mdb_status ivf_search_impl(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes,
                                  size_t k, mdb_mem mem, int mode, void* ids_out, float* scores_out, uint32_t* counts_out,
                                  const FilterArg* fa = nullptr, bool submit = false) {
    IvfSet& s = ivf->set;
    mdb_ctx* ctx = s.ctx;
    MDB_ENTER(ctx);
    MDB_TRY(mdb_require_idle(ctx, mem));
    const bool remap = mode == OUT_DOCS;
    if (b == 0) return MDB_OK;
    if (k > MDB_MAX_K) return mdb_fail(ctx, MDB_ERR_UNSUPPORTED, "k=%zu exceeds MDB_MAX_K=%d", k, MDB_MAX_K);
    SubmitScope submit_scope(ctx, submit && mem == MDB_MEM_HOST);
    IvfSet::ScanFilter filt;
    if (fa) MDB_TRY(s.stage_filter(fa->allow, fa->n_bitmaps, fa->words, mem, b, &filt));
    float* dq;
    int qstride;
    const size_t bpad = probes ? (b + 3) / 4 * 4 : s.coarse_bpad(b);
    // small batches of an L2 PQ index: the whole step is ONE kernel (ivf_pq_fused_kernel), device-resident queries are read in place
    const bool fused = s.fused_ok(b, k, num_probes, probes != nullptr);
    if (fused && mem == MDB_MEM_DEVICE) { dq = const_cast<float*>(queries); qstride = (int)s.num_features; }
    else MDB_TRY(stage_queries(ctx, queries, b, (int)s.num_features, mem, bpad, &dq, &qstride));
    void* dprobes;
    MDB_TRY(mdb_scratch(ctx, b * std::max<size_t>(num_probes, 1) * 4, &dprobes));
    if (probes) {
        if (num_probes == 0) { /* empty centroid list: empty results */ }
        else if (mem == MDB_MEM_HOST) {  // through pinned staging: the caller's buffer is free when the call returns
            void* pin;
            MDB_TRY(mdb_pinned(ctx, MDB_PIN_AUX, b * num_probes * 4, &pin));
            memcpy(pin, probes, b * num_probes * 4);
            MDB_HIP(ctx, hipMemcpyAsync(dprobes, pin, b * num_probes * 4, hipMemcpyHostToDevice, ctx->stream));
        } else MDB_HIP(ctx, hipMemcpyAsync(dprobes, probes, b * num_probes * 4, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (!fused) {
        MDB_TRY(s.coarse(0, dq, qstride, b, num_probes, (uint32_t*)dprobes, true, bpad));  // also clears the device counters
    }
    void *keys, *cnts;
    MDB_TRY(mdb_scratch(ctx, b * std::max<size_t>(k, 1) * 8, &keys));
    MDB_TRY(mdb_scratch(ctx, b * 4 + 16, &cnts));
    if (probes && !fused) MDB_HIP(ctx, hipMemsetAsync(ctx->d_counters, 0, 32, ctx->stream));
    ctx->dev_counters = true;
    ctx->stats = mdb_stats{};
    ctx->counter_base = 0;
    ctx->counters_clean = false;
    ctx->stat_bytes_per_eval = 0; ctx->stat_bytes_per_scored = s.bytes_per_scored(); ctx->stat_fixed_bytes = 0;
    size_t total = b * k;
    if (fused) {
        const uint32_t* fp = probes ? (const uint32_t*)dprobes : nullptr;
        if (mode != OUT_DOCS) {
            MDB_TRY(s.search_fused(dq, qstride, b, fp, num_probes, k, &filt, (uint64_t*)keys, (uint32_t*)cnts, nullptr, nullptr, nullptr));
        } else if (mem == MDB_MEM_DEVICE) {   // doc ids, scores and counts straight into the caller's buffers
            return s.search_fused(dq, qstride, b, fp, num_probes, k, &filt, nullptr, nullptr, (mdb_u128*)ids_out, scores_out, counts_out);
        } else {
            void *dids, *dsc;
            MDB_TRY(mdb_scratch(ctx, total * 16 + 16, &dids));
            MDB_TRY(mdb_scratch(ctx, total * 4 + 16, &dsc));
            MDB_TRY(s.search_fused(dq, qstride, b, fp, num_probes, k, &filt, nullptr, nullptr, (mdb_u128*)dids, (float*)dsc, (uint32_t*)cnts));
            const HostCopy back[3] = {{ids_out, dids, total * 16}, {scores_out, dsc, total * 4}, {counts_out, cnts, b * 4}};
            return mdb_return_to_host(ctx, back, 3);
        }
    } else
    MDB_TRY(s.scan(dq, qstride, b, nullptr, (uint32_t*)dprobes, nullptr, (int)num_probes, k, (uint64_t*)keys, (uint32_t*)cnts, &filt));
    if (mode == OUT_BLOCK) {
        if (mem == MDB_MEM_DEVICE) return s.pack_points((uint64_t*)keys, (uint32_t*)cnts, nullptr, b, k, ids_out);
        return s.pack_points_to_host((uint64_t*)keys, (uint32_t*)cnts, nullptr, b, k, ids_out);
    }
    if (mem == MDB_MEM_DEVICE) {
        if (remap) MDB_TRY(s.remap((uint64_t*)keys, (uint32_t*)cnts, b, k, nullptr, (mdb_u128*)ids_out, scores_out, counts_out));
        else {
            if (total) unpack_keys(ctx, (uint64_t*)keys, total, (uint32_t*)ids_out, scores_out);
            if (counts_out) MDB_HIP(ctx, hipMemcpyAsync(counts_out, cnts, b * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
        return MDB_OK;
    }
    void *dids, *dsc;
    MDB_TRY(mdb_scratch(ctx, total * 16 + 16, &dids));
    MDB_TRY(mdb_scratch(ctx, total * 4 + 16, &dsc));
    if (remap) MDB_TRY(s.remap((uint64_t*)keys, (uint32_t*)cnts, b, k, nullptr, (mdb_u128*)dids, (float*)dsc, nullptr));
    else if (total) unpack_keys(ctx, (uint64_t*)keys, total, (uint32_t*)dids, (float*)dsc);
    const HostCopy back[3] = {{ids_out, dids, total * (remap ? 16 : 4)}, {scores_out, dsc, total * 4}, {counts_out, cnts, b * 4}};
    return mdb_return_to_host(ctx, back, 3);
}

extern "C" {

mdb_status mdb_ivf_load(mdb_ctx* ctx, const void* index_bytes, size_t index_len, size_t index_offset,
                        const void* vectors_bytes, size_t vectors_len, size_t vectors_offset, const mdb_quant_desc* quant,
                        uint32_t shard_rank, uint32_t shard_world, mdb_ivf** out) {
    if (!ctx || !index_bytes || !vectors_bytes || !out) return MDB_ERR_INVALID_ARG;
    *out = nullptr;
    MDB_ENTER(ctx);
    mdb_ivf* ivf = new mdb_ivf();
    mdb_status st = ivf->set.load(ctx, (const uint8_t*)index_bytes, index_len, (const uint8_t*)vectors_bytes, vectors_len,
                                  {{index_offset, vectors_offset}}, quant, shard_rank, shard_world);
    if (st != MDB_OK) { delete ivf; return st; }
    mdb_ctx_retain(ctx);
    *out = ivf;
    return MDB_OK;
}

void mdb_ivf_free(mdb_ivf* ivf) {
    if (!ivf) return;
    (void)hipSetDevice(ivf->set.ctx->device);
    (void)hipStreamSynchronize(ivf->set.ctx->stream);
    ivf_release(ivf);
}

mdb_status mdb_ivf_attach(mdb_ctx* ctx, mdb_ivf* src, mdb_ivf** out) {
    if (!ctx || !src || !out) return MDB_ERR_INVALID_ARG;
    *out = nullptr;
    if (ctx->device != src->set.ctx->device) return mdb_fail(ctx, MDB_ERR_INVALID_ARG, "mdb_ivf_attach: the index lives on device %d", src->set.ctx->device);
    mdb_ivf* owner = src->parent ? src->parent : src;
    mdb_ivf* h = new mdb_ivf();
    h->set.view_of(owner->set, ctx);
    h->parent = owner;
    owner->refs.fetch_add(1);
    mdb_ctx_retain(ctx);
    *out = h;
    return MDB_OK;
}

size_t mdb_ivf_num_clusters(const mdb_ivf* ivf) { return ivf ? ivf->set.blobs[0].num_clusters : 0; }
size_t mdb_ivf_num_vectors(const mdb_ivf* ivf) { return ivf ? (size_t)ivf->set.blobs[0].vec_num_vectors : 0; }
size_t mdb_ivf_num_features(const mdb_ivf* ivf) { return ivf ? ivf->set.num_features : 0; }
size_t mdb_ivf_num_resident_vectors(const mdb_ivf* ivf) { return ivf ? ivf->set.total_slots_valid : 0; }

mdb_status mdb_ivf_find_nearest_centroids(mdb_ivf* ivf, const float* queries, size_t b, size_t num_probes, mdb_mem mem,
                                          uint32_t* out) {
    if (!ivf || (!queries && b) || !out) return MDB_ERR_INVALID_ARG;
    IvfSet& s = ivf->set;
    mdb_ctx* ctx = s.ctx;
    MDB_ENTER(ctx);
    if (num_probes == 0 || num_probes > s.blobs[0].num_clusters)
        return mdb_fail(ctx, MDB_ERR_OUT_OF_RANGE, "num_probes=%zu out of range (num_clusters=%u)", num_probes, s.blobs[0].num_clusters);
    if (b == 0) return MDB_OK;
    float* dq;
    int qstride;
    const size_t bpad = s.coarse_bpad(b);
    MDB_TRY(stage_queries(ctx, queries, b, (int)s.num_features, mem, bpad, &dq, &qstride));
    if (mem == MDB_MEM_DEVICE) return s.coarse(0, dq, qstride, b, num_probes, out, false, bpad);
    void* dprobes;
    MDB_TRY(mdb_scratch(ctx, b * num_probes * 4, &dprobes));
    MDB_TRY(s.coarse(0, dq, qstride, b, num_probes, (uint32_t*)dprobes, false, bpad));
    MDB_HIP(ctx, hipMemcpyAsync(out, dprobes, b * num_probes * 4, hipMemcpyDeviceToHost, ctx->stream));
    return mdb_check_flags(ctx);
}

__global__ void keys_add_id_offset_kernel(uint64_t* __restrict__ keys, size_t total, uint32_t add) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < total && keys[t] != MDB_KEY_MAX) keys[t] += add;  // id = low word; first + row < 2^32
}

mdb_status mdb_ivf_coarse_keys(mdb_ivf* ivf, const float* queries, size_t b, size_t num_probes, size_t first, size_t count,
                               mdb_mem mem, uint64_t* keys_out) {
    if (!ivf || (!queries && b) || !keys_out) return MDB_ERR_INVALID_ARG;
    IvfSet& s = ivf->set;
    mdb_ctx* ctx = s.ctx;
    MDB_ENTER(ctx);
    const size_t L = s.blobs[0].num_clusters;
    if (num_probes == 0 || num_probes > MDB_MAX_K || (first % MDB_TILE) != 0 || first > L || count > L - first)
        return mdb_fail(ctx, MDB_ERR_OUT_OF_RANGE, "coarse_keys: num_probes=%zu, centroid range [%zu, %zu) of %zu", num_probes, first, first + count, L);
    if (b == 0) return MDB_OK;
    const size_t total = b * num_probes;
    void* dkeys = keys_out;
    if (mem == MDB_MEM_HOST) MDB_TRY(mdb_scratch(ctx, total * 8, &dkeys));
    if (count == 0) {
        MDB_HIP(ctx, hipMemsetAsync(dkeys, 0xFF, total * 8, ctx->stream));
    } else {
        float* dq;
        int qstride;
        const int d4 = ((int)s.num_features + 3) / 4;
        TileView cv{s.d_cent_tiles.p + ((size_t)s.h_users[0].cent_tile_base + first / MDB_TILE) * MDB_TILE * d4 * 4, count,
                    (count + MDB_TILE - 1) / MDB_TILE, (int)s.num_features, d4};
        // a slice of a LARGE coarse quantizer (a rank's share of C5's 65 536 centroids) takes the batched path too — sample bound,
        // matrix-core filter, exact refine over the slice — through a view of the index's filter operands
        bool batched = false;
        if (s.cent_aux.sample.n && count % MDB_TILE == 0 && b >= 8) {
            if (s.slice_first != first || s.slice_count != count) {
                s.slice_first = ~(size_t)0;
                if (flat_aux_subrange(s.cent_aux, first / MDB_TILE, count / MDB_TILE, d4, s.cent_slice)) { s.slice_first = first; s.slice_count = count; }
            }
            batched = s.slice_first == first && flat_mfma_applicable(ctx, cv, s.cent_slice, b, num_probes);
        }
        const size_t bpad = batched ? (b + 255) / 256 * 256 : (b + 3) / 4 * 4;
        MDB_TRY(stage_queries(ctx, queries, b, (int)s.num_features, mem, bpad, &dq, &qstride));
        if (batched) MDB_TRY(flat_topk_keys_mfma(ctx, cv, s.cent_slice, MDB_METRIC_L2, dq, qstride, b, bpad, num_probes, (uint64_t*)dkeys, nullptr));
        else MDB_TRY(flat_topk_keys(ctx, cv, MDB_METRIC_L2, dq, qstride, b, num_probes, (uint64_t*)dkeys, nullptr));
        if (first) keys_add_id_offset_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, ctx->stream>>>((uint64_t*)dkeys, total, (uint32_t)first);
        MDB_HIP(ctx, hipGetLastError());
    }
    if (mem == MDB_MEM_DEVICE) return MDB_OK;
    const HostCopy back[1] = {{keys_out, dkeys, total * 8}};
    return mdb_return_to_host(ctx, back, 1);
}

mdb_status mdb_ivf_merge_coarse_keys(mdb_ivf* ivf, const uint64_t* keys, size_t b, size_t parts, size_t num_probes, mdb_mem mem,
                                     uint32_t* probes_out) {
    if (!ivf || (!keys && b) || !probes_out || parts == 0 || num_probes == 0) return MDB_ERR_INVALID_ARG;
    mdb_ctx* ctx = ivf->set.ctx;
    MDB_ENTER(ctx);
    if (num_probes > MDB_MAX_K) return mdb_fail(ctx, MDB_ERR_UNSUPPORTED, "num_probes=%zu exceeds MDB_MAX_K=%d", num_probes, MDB_MAX_K);
    if (b == 0) return MDB_OK;
    const size_t per = parts * num_probes, total = b * num_probes;
    const uint64_t* din = keys;
    void *stage, *merged, *dist, *dids = probes_out;
    if (mem == MDB_MEM_HOST) {
        void* pin;
        MDB_TRY(mdb_pinned(ctx, MDB_PIN_IN, b * per * 8, &pin));
        memcpy(pin, keys, b * per * 8);
        MDB_TRY(mdb_scratch(ctx, b * per * 8, &stage));
        MDB_HIP(ctx, hipMemcpyAsync(stage, pin, b * per * 8, hipMemcpyHostToDevice, ctx->stream));
        din = (const uint64_t*)stage;
        MDB_TRY(mdb_scratch(ctx, total * 4, &dids));
    }
    if (per * 8 <= 48 * 1024) {
        MDB_TRY(merge_sorted_rows(ctx, din, parts, num_probes, b, nullptr, nullptr, (uint32_t*)dids, nullptr));
    } else {
        MDB_TRY(mdb_scratch(ctx, total * 8, &merged));
        MDB_TRY(mdb_scratch(ctx, total * 4 + 16, &dist));
        MDB_TRY(merge_keys(ctx, din, per, b, num_probes, (uint64_t*)merged, nullptr));
        MDB_TRY(unpack_keys(ctx, (const uint64_t*)merged, total, (uint32_t*)dids, (float*)dist));
    }
    if (mem == MDB_MEM_DEVICE) return MDB_OK;
    const HostCopy back[1] = {{probes_out, dids, total * 4}};
    return mdb_return_to_host(ctx, back, 1);
}

mdb_status mdb_ivf_search(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes, size_t k,
                          mdb_mem mem, mdb_u128* doc_ids_out, float* scores_out, uint32_t* counts_out) {
    if (!ivf || (!queries && b) || !doc_ids_out || !scores_out) return MDB_ERR_INVALID_ARG;
    return ivf_search_impl(ivf, queries, b, probes, num_probes, k, mem, OUT_DOCS, doc_ids_out, scores_out, counts_out);
}

mdb_status mdb_ivf_search_points(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes,
                                 size_t k, mdb_mem mem, uint32_t* point_ids_out, float* scores_out, uint32_t* counts_out) {
    if (!ivf || (!queries && b) || !point_ids_out || !scores_out) return MDB_ERR_INVALID_ARG;
    return ivf_search_impl(ivf, queries, b, probes, num_probes, k, mem, OUT_POINTS, point_ids_out, scores_out, counts_out);
}

mdb_status mdb_ivf_search_filtered(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes, size_t k,
                                   mdb_mem mem, const uint32_t* allow, size_t n_bitmaps, size_t words_per_bitmap,
                                   mdb_u128* doc_ids_out, float* scores_out, uint32_t* counts_out) {
    if (!ivf || (!queries && b) || !doc_ids_out || !scores_out) return MDB_ERR_INVALID_ARG;
    const FilterArg fa{allow, n_bitmaps, words_per_bitmap};
    return ivf_search_impl(ivf, queries, b, probes, num_probes, k, mem, OUT_DOCS, doc_ids_out, scores_out, counts_out, &fa);
}

mdb_status mdb_ivf_search_submit(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes, size_t k,
                                 const uint32_t* allow, size_t n_bitmaps, size_t words_per_bitmap, mdb_u128* doc_ids_out,
                                 float* scores_out, uint32_t* counts_out) {
    if (!ivf || (!queries && b) || !doc_ids_out || !scores_out) return MDB_ERR_INVALID_ARG;
    const FilterArg fa{allow, n_bitmaps, words_per_bitmap};
    return ivf_search_impl(ivf, queries, b, probes, num_probes, k, MDB_MEM_HOST, OUT_DOCS, doc_ids_out, scores_out, counts_out, &fa, true);
}

// ---- exact list-sharded search
size_t mdb_points_block_bytes(size_t b, size_t k) { return mdb_points_block_bytes_impl(b, k); }

mdb_status mdb_points_block_views(void* block, size_t b, size_t k, uint32_t** point_ids, float** scores, uint32_t** counts, uint8_t** found) {
    if (!block) return MDB_ERR_INVALID_ARG;
    char* p = (char*)block;
    if (point_ids) *point_ids = (uint32_t*)p;
    if (scores) *scores = (float*)(p + b * k * 4);
    if (counts) *counts = (uint32_t*)(p + b * k * 8);
    if (found) *found = (uint8_t*)(p + b * k * 8 + b * 4);
    return MDB_OK;
}

mdb_status mdb_ivf_search_shard(mdb_ivf* ivf, const float* queries, size_t b, const uint32_t* probes, size_t num_probes, size_t k,
                                mdb_mem mem, const uint32_t* allow, size_t n_bitmaps, size_t words_per_bitmap, void* block_out) {
    if (!ivf || (!queries && b) || !block_out) return MDB_ERR_INVALID_ARG;
    const FilterArg fa{allow, n_bitmaps, words_per_bitmap};
    return ivf_search_impl(ivf, queries, b, probes, num_probes, k, mem, OUT_BLOCK, block_out, nullptr, nullptr, &fa);
}

mdb_status mdb_ivf_merge_shards(mdb_ivf* ivf, const void* blocks, size_t world, size_t b, size_t k, mdb_u128* doc_ids_out,
                                float* scores_out, uint32_t* counts_out) {
    if (!ivf || !blocks || !doc_ids_out || !scores_out || world == 0) return MDB_ERR_INVALID_ARG;
    IvfSet& s = ivf->set;
    MDB_ENTER(s.ctx);
    if (k > MDB_MAX_K) return mdb_fail(s.ctx, MDB_ERR_UNSUPPORTED, "k=%zu exceeds MDB_MAX_K=%d", k, MDB_MAX_K);
    return s.merge_points(blocks, world, b, k, nullptr, doc_ids_out, scores_out, counts_out, nullptr);
}


mdb_status mdb_ivf_invalidate(mdb_ivf* ivf, const mdb_u128* doc_ids, size_t n, uint8_t* flags_out) {
    if (!ivf || (!doc_ids && n) || !flags_out) return MDB_ERR_INVALID_ARG;
    MDB_ENTER(ivf->set.ctx);
    return ivf->set.invalidate(0, doc_ids, n, flags_out, false);
}

mdb_status mdb_ivf_is_invalidated(mdb_ivf* ivf, const mdb_u128* doc_ids, size_t n, uint8_t* flags_out) {
    if (!ivf || (!doc_ids && n) || !flags_out) return MDB_ERR_INVALID_ARG;
    MDB_ENTER(ivf->set.ctx);
    return ivf->set.invalidate(0, doc_ids, n, flags_out, true);
}

}  // extern "C"

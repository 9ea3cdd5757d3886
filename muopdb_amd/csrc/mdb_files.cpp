// mdb_files.cpp — the host halves of HnswSet::load, IvfSet::load, mdb_spann_load and mdb_multi_spann_load (mdb_files.h), and the
// mdb_*_check_files entries of the C ABI over them.  Plain C++: no HIP header, no mdb_ctx, no environment.
//
// Every refusal is `return fail(why, status, "message", ...)`; tests/test_file_refusal.py collects these literals and requires a
// file of tests/file_mutations.py behind each of them.  Lengths and counts come from the files: every sum is formed only after its
// terms have been bounded by the file's length, and nothing is allocated from a field before the field has been bounded.
#include "mdb_files.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

static mdb_status fail(std::string& why, mdb_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    why = buf;
    return st;
}

#define FILES_TRY(...)                   \
    do {                                 \
        mdb_status _s = (__VA_ARGS__);   \
        if (_s != MDB_OK) return _s;     \
    } while (0)

mdb_status pq_shape(const mdb_quant_desc* q, PqShape& o, std::string& why) {
    if (!q || q->kind != MDB_QUANT_PQ) return fail(why, MDB_ERR_INVALID_ARG, "not a product quantizer");
    if (q->subvector_dimension == 0 || q->dimension % q->subvector_dimension != 0)
        return fail(why, MDB_ERR_INVALID_ARG, "Vector dimension needs to be divisible by the subvector dimension.");
    if (q->num_bits == 0 || q->num_bits > 8)
        return fail(why, MDB_ERR_UNSUPPORTED, "PQ codes are u8: num_bits must be 1..8");
    o.metric = q->metric; o.dimension = q->dimension; o.subdim = q->subvector_dimension; o.num_bits = q->num_bits;
    o.m = o.dimension / o.subdim; o.K = 1 << o.num_bits;
    o.need = (size_t)o.m * o.K * o.subdim;
    if (!q->codebook || q->codebook_len < o.need) return fail(why, MDB_ERR_FORMAT, "codebook too short");
    return MDB_OK;
}

// ------------------------------------------------------------------------------------------ HNSW
static mdb_status parse_hnsw_blob(const uint8_t* b, size_t len, size_t data_offset, HnswBlobInfo& o, std::string& why) {
    if (!fits(data_offset, 49, len)) return fail(why, MDB_ERR_FORMAT, "HNSW index: header out of bounds");
    const uint8_t* h = b + data_offset;
    if (h[0] != 0) return fail(why, MDB_ERR_FORMAT, "HNSW index: Unknown version: %d", (int)h[0]);
    o.quantized_dimension = rd_u32(h + 1);
    o.num_layers = rd_u32(h + 5);
    o.edges_len = rd_u64(h + 9);
    o.points_len = rd_u64(h + 17);
    o.edge_offsets_len = rd_u64(h + 25);
    o.level_offsets_len = rd_u64(h + 33);
    o.doc_id_mapping_len = rd_u64(h + 41);
    // section lengths come from the file: reject any that cannot fit before forming offsets (overflow-safe)
    if (o.edges_len > len || o.points_len > len || o.edge_offsets_len > len || o.level_offsets_len > len || o.doc_id_mapping_len > len)
        return fail(why, MDB_ERR_FORMAT, "HNSW index: a section is longer than the file");
    size_t off = data_offset + 49;  // calculate_offsets, graph_storage.rs:170-196
    o.edges_offset = off + (4 - (off % 4)) % 4;
    o.points_offset = o.edges_offset + o.edges_len;
    size_t pe = o.points_offset + o.points_len;
    o.edge_offsets_offset = pe + (8 - (pe % 8)) % 8;
    o.level_offsets_offset = o.edge_offsets_offset + o.edge_offsets_len;
    size_t le = o.level_offsets_offset + o.level_offsets_len;
    o.doc_id_mapping_offset = le + (16 - (le % 16)) % 16;
    if (o.doc_id_mapping_offset + o.doc_id_mapping_len > len) return fail(why, MDB_ERR_FORMAT, "HNSW index: sections out of bounds");
    if (o.num_layers > MDB_HNSW_MAX_LAYERS) return fail(why, MDB_ERR_UNSUPPORTED, "more than 255 HNSW layers");
    // No layers and yet a graph: the reference's reader takes level_offsets[0] and a point from such a file whatever num_layers
    // says (rs/index/src/hnsw/block_based/graph_storage.rs:549-553) and returns that point, where the kernels' `num_layers == 0`
    // answer is the empty result of an empty index.  The writer never produces it; it is refused.
    if (o.num_layers == 0 && (o.edges_len || o.points_len || o.edge_offsets_len || o.level_offsets_len))
        return fail(why, MDB_ERR_FORMAT, "HNSW index: num_layers is 0 but the graph sections are not empty");
    if (o.level_offsets_len / 8 < (uint64_t)o.num_layers + 1 && o.num_layers > 0)
        return fail(why, MDB_ERR_FORMAT, "HNSW index: level_offsets too short");
    return MDB_OK;
}

mdb_status hnsw_file_dimension(const uint8_t* index, size_t index_len, size_t index_offset, const mdb_quant_desc* quant, uint32_t* dim,
                               std::string& why) {
    if (!fits(index_offset, 9, index_len)) return fail(why, MDB_ERR_FORMAT, "HNSW index: header out of bounds (offset %zu of %zu bytes)", index_offset, index_len);
    *dim = quant && quant->dimension ? quant->dimension : rd_u32(index + index_offset + 1);
    return MDB_OK;
}

mdb_status hnsw_plan_files(const uint8_t* index, size_t index_len, const uint8_t* vectors, size_t vectors_len,
                           const std::vector<std::pair<size_t, size_t>>& offsets, const mdb_quant_desc* quant, uint32_t dim,
                           const HnswPlanOpts& opts, HnswPlan& P, std::string& why) {
    P = HnswPlan{};
    const int kind = P.kind = quant ? (int)quant->kind : MDB_QUANT_NONE;
    P.metric = quant ? quant->metric : MDB_METRIC_L2;
    if (kind == MDB_QUANT_PQ) {
        FILES_TRY(pq_shape(quant, P.pq, why));
        if ((uint32_t)P.pq.dimension != dim) return fail(why, MDB_ERR_INVALID_ARG, "PQ dimension %d != %u", P.pq.dimension, dim);
    }
    // bytes of one stored vector in the file: f32 row, or m u8 codes (BlockBasedHnsw<ProductQuantizer>)
    const size_t file_row = P.file_row = kind == MDB_QUANT_PQ ? (size_t)P.pq.m : (size_t)dim * 4;
    const uint32_t file_qdim = kind == MDB_QUANT_PQ ? (uint32_t)P.pq.m : dim;
    if (file_row == 0) return fail(why, MDB_ERR_FORMAT, "HNSW index: the vectors have no dimension");
    P.dimension = dim;
    const int dpad = P.dpad = (int)(((uint64_t)dim + 3) / 4 * 4);
    const size_t U = offsets.size();
    P.blobs.resize(U);
    P.users.assign(U + 1, HnswUserDev{});  // [U] = sentinel (valid = 0): unknown user => None
    std::vector<uint32_t>&h_adj = P.adj, &h_upper_first = P.upper_first;
    std::vector<uint8_t>& h_level = P.level;
    std::vector<uint64_t>& row_src = P.row_src;
    for (size_t ui = 0; ui < U; ++ui) {
        HnswBlobInfo& bi = P.blobs[ui];
        FILES_TRY(parse_hnsw_blob(index, index_len, offsets[ui].first, bi, why));
        if (bi.quantized_dimension != file_qdim) return fail(why, MDB_ERR_FORMAT, "HNSW quantized_dimension %u != %u", bi.quantized_dimension, file_qdim);
        size_t voff = offsets[ui].second;
        if (!fits(voff, 8, vectors_len)) return fail(why, MDB_ERR_FORMAT, "HNSW vector file: header out of bounds");
        uint64_t nv = rd_u64(vectors + voff);
        if (nv > (vectors_len - voff - 8) / file_row) return fail(why, MDB_ERR_FORMAT, "vector file truncated");
        if (kind != MDB_QUANT_PQ && (voff + 8) % 4 != 0) return fail(why, MDB_ERR_FORMAT, "HNSW f32 vector file is not 4-byte aligned");
        if (nv > 0xFFFFFFFEull) return fail(why, MDB_ERR_UNSUPPORTED, "HNSW point ids are u32");
        // the remap kernels read doc id `p` of every point p < num_vectors from the section (get_doc_id, graph_storage.rs:556-560,
        // reads past a short one and fails there)
        if (bi.doc_id_mapping_len / 16 < nv)
            return fail(why, MDB_ERR_FORMAT, "HNSW doc-id section holds %llu ids for %llu vectors", (unsigned long long)(bi.doc_id_mapping_len / 16),
                        (unsigned long long)nv);
        bi.num_vectors = nv;
        bi.vec_data_offset = voff + 8;
        HnswUserDev& u = P.users[ui];
        u.valid = 1;
        u.n = (uint32_t)nv;
        u.num_layers = bi.num_layers;
        u.doc_ids_off = bi.doc_id_mapping_offset;
        u.vec_off = (uint64_t)row_src.size() * dpad;
        for (uint64_t r = 0; r < nv; ++r) row_src.push_back(bi.vec_data_offset + r * file_row);
        u.upper_off = h_level.size();
        h_level.resize(h_level.size() + nv, 0);
        h_upper_first.resize(h_upper_first.size() + nv, 0xFFFFFFFFu);
        if (bi.num_layers == 0) continue;
        const uint32_t nl = bi.num_layers;
        auto lvl = [&](size_t i) { return rd_u64(index + bi.level_offsets_offset + i * 8); };
        auto eo = [&](size_t i) { return rd_u64(index + bi.edge_offsets_offset + i * 8); };
        auto pt = [&](size_t i) { return rd_u32(index + bi.points_offset + i * 4); };
        auto ed = [&](size_t i) { return rd_u32(index + bi.edges_offset + i * 4); };
        const size_t n_eo = bi.edge_offsets_len / 8, n_pts = bi.points_len / 4, n_edges = bi.edges_len / 4;
        for (uint32_t i = 0; i <= nl; ++i) {
            if (lvl(i) > n_eo) return fail(why, MDB_ERR_FORMAT, "HNSW level offset out of bounds");
            if (i && lvl(i) < lvl(i - 1)) return fail(why, MDB_ERR_FORMAT, "HNSW level offsets decrease");
        }
        // layer 0: slots s0 .. e0 (the last one is the sentinel)
        const size_t s0 = lvl(nl - 1), e0 = lvl(nl);
        // every upper-layer slot i reads edge offsets i and i + 1, and point i: the layers end below both sections' ends
        if (s0 > n_pts || (s0 > 0 && s0 >= n_eo)) return fail(why, MDB_ERR_FORMAT, "HNSW points section too short");
        // entry point (graph_storage.rs:527-558)
        if (nl == 1) {
            size_t num_points = n_eo ? n_eo - 1 : 0;
            u.entry_point = 0;
            for (size_t i = 0; i < num_points; ++i)
                if (eo(i + 1) > eo(i)) { u.entry_point = (uint32_t)i; break; }
        } else {
            if (lvl(1) <= lvl(0)) return fail(why, MDB_ERR_FORMAT, "HNSW top layer is empty");
            u.entry_point = pt(lvl(0));
        }
        // the entry point is the first row the traversal reads: a slot past the vector file (more layer-0 slots than vectors and
        // none of the first num_vectors has an edge) or a point id the layers' own check below never sees
        if (nv && u.entry_point >= nv)
            return fail(why, MDB_ERR_FORMAT, "HNSW entry point %u is outside the vector storage (%llu vectors)", u.entry_point, (unsigned long long)nv);
        const size_t n0 = e0 > s0 ? e0 - s0 - 1 : 0;
        u.n0 = (uint32_t)std::min<size_t>(n0, nv);
        uint32_t S0 = 1;
        for (size_t p = 0; p < u.n0; ++p) {
            uint64_t a0 = eo(s0 + p), a1 = eo(s0 + p + 1);
            if (a1 < a0 || a1 > n_edges) return fail(why, MDB_ERR_FORMAT, "HNSW edge offsets corrupt");
            S0 = std::max<uint32_t>(S0, (uint32_t)std::min<uint64_t>(a1 - a0, 1u << 20));
        }
        // upper layers: per point level + rows
        uint32_t SU = 1;
        for (uint32_t layer = 1; layer < nl; ++layer) {
            size_t s = lvl(nl - 1 - layer), e = lvl(nl - layer);
            for (size_t i = s; i < e; ++i) {
                uint32_t p = pt(i);
                if (p >= nv) return fail(why, MDB_ERR_FORMAT, "HNSW upper-layer point id out of range");
                h_level[u.upper_off + p] = std::max<uint8_t>(h_level[u.upper_off + p], (uint8_t)layer);
                uint64_t a0 = eo(i), a1 = eo(i + 1);
                if (a1 < a0 || a1 > n_edges) return fail(why, MDB_ERR_FORMAT, "HNSW upper-layer edge offsets corrupt");
                SU = std::max<uint32_t>(SU, (uint32_t)std::min<uint64_t>(a1 - a0, 1u << 20));
            }
        }
        if (S0 > MDB_HNSW_MAX_DEGREE || SU > MDB_HNSW_MAX_DEGREE)
            return fail(why, MDB_ERR_UNSUPPORTED, "node degree %u exceeds %d", std::max(S0, SU), MDB_HNSW_MAX_DEGREE);
        u.S0 = S0;
        u.SU = SU;
        P.max_stride = std::max(P.max_stride, std::max(S0, SU));
        u.adj0_off = h_adj.size();
        h_adj.resize(h_adj.size() + (size_t)u.n0 * S0, 0xFFFFFFFFu);
        for (size_t p = 0; p < u.n0; ++p) {
            uint64_t a0 = eo(s0 + p), a1 = eo(s0 + p + 1);
            for (uint64_t x = a0; x < a1; ++x) {
                const uint32_t e = ed(x);
                if (e >= nv) return fail(why, MDB_ERR_FORMAT, "HNSW edge %u of point %zu is outside the vector storage (%llu vectors)", e, p, (unsigned long long)nv);
                h_adj[u.adj0_off + p * S0 + (x - a0)] = e;
            }
        }
        // rows of the upper layers
        uint32_t rows = 0;
        for (uint64_t p = 0; p < nv; ++p)
            if (h_level[u.upper_off + p]) { h_upper_first[u.upper_off + p] = rows; rows += h_level[u.upper_off + p]; }
        u.adjU_off = h_adj.size();
        h_adj.resize(h_adj.size() + (size_t)rows * SU, 0xFFFFFFFFu);
        std::vector<uint8_t> filled((size_t)rows, 0);
        for (uint32_t layer = 1; layer < nl; ++layer) {
            size_t s = lvl(nl - 1 - layer), e = lvl(nl - layer);
            for (size_t i = s; i < e; ++i) {
                uint32_t p = pt(i);
                size_t r = (size_t)h_upper_first[u.upper_off + p] + (layer - 1);
                const bool keep = !filled[r];  // find_point_in_range returns the FIRST match: a later slot of the same point is never read
                filled[r] = 1;                 // ... by a search; its edges are still range-checked (the small-layer test below walks them)
                uint64_t a0 = eo(i), a1 = eo(i + 1);
                for (uint64_t x = a0; x < a1; ++x) {
                    const uint32_t e = ed(x);
                    if (e >= nv) return fail(why, MDB_ERR_FORMAT, "HNSW upper-layer edge %u is outside the vector storage", e);
                    if (keep) h_adj[u.adjU_off + r * SU + (x - a0)] = e;
                }
            }
        }
        // dense upper layers (hnsw_upper_row): every (layer, point) gets a row slot — affordable up to 1 GiB per graph
        u.adjD_off = ~0ull;
        if (nl > 1 && !opts.no_dense && (uint64_t)(nl - 1) * nv * SU * 4 <= ((uint64_t)1 << 30)) {
            u.adjD_off = h_adj.size();
            h_adj.resize(h_adj.size() + (size_t)(nl - 1) * nv * SU, 0xFFFFFFFFu);
            for (uint64_t p = 0; p < nv; ++p) {
                const uint32_t lv = h_level[u.upper_off + p];
                for (uint32_t layer = 1; layer <= lv && layer < nl; ++layer) {
                    const size_t r = (size_t)h_upper_first[u.upper_off + p] + (layer - 1);
                    std::copy(h_adj.begin() + u.adjU_off + r * SU, h_adj.begin() + u.adjU_off + (r + 1) * SU,
                              h_adj.begin() + u.adjD_off + ((size_t)(layer - 1) * nv + p) * SU);
                }
            }
        }
        // tiny top layers (hnsw_beam_kernel expands them frontier-wise): <= 64 points, every edge inside the layer
        {
            std::vector<uint64_t> cnt(nl + 1, 0);
            for (uint64_t p = 0; p < nv; ++p) cnt[std::min<uint32_t>(h_level[u.upper_off + p], nl)] += 1;
            for (int l = (int)nl - 1; l >= 0; --l) cnt[l] += cnt[l + 1];  // cnt[l] = points with level >= l
            uint32_t small = nl;
            for (uint32_t layer = nl; layer-- > 1;) {
                bool ok = cnt[layer] <= 64;
                if (ok) {
                    size_t s = lvl(nl - 1 - layer), e = lvl(nl - layer);
                    for (size_t i = s; i < e && ok; ++i) {
                        uint64_t a0 = eo(i), a1 = eo(i + 1);
                        for (uint64_t x = a0; x < a1; ++x)
                            if (h_level[u.upper_off + ed(x)] < layer) { ok = false; break; }
                    }
                }
                if (!ok) break;
                small = layer;
            }
            u.small_layer = small;
        }
        P.max_n = std::max(P.max_n, u.n);
        P.max_rows0 = std::max<uint64_t>(P.max_rows0, std::min<uint64_t>((uint64_t)u.n0 * u.S0, 0xFFFFFFFFull));
        if (u.num_layers > 1) {
            if (u.adjD_off == ~0ull) P.all_dense = false;
            P.max_rowsU = std::max<uint64_t>(P.max_rowsU, std::min<uint64_t>((uint64_t)(u.num_layers - 1) * u.n * u.SU, 0xFFFFFFFFull));
        }
    }
    // ---- the table path's compact upper layers (mdb_hnsw_upper.hip): one graph, >= 2 layers, f32 rows, rows of <= 64 edges
    std::vector<uint32_t>&h_cids = P.cids, &h_crows = P.crows, &h_crows2 = P.crows2, &h_map21 = P.map21;
    std::vector<float>&h_cvecs = P.cvecs, &h_cvecs2 = P.cvecs2;
    if (U == 1 && kind != MDB_QUANT_PQ && !opts.no_table && P.users[0].num_layers >= 2 && P.users[0].SU <= 64 && P.users[0].n > 0) {
        const HnswUserDev& u = P.users[0];
        const HnswBlobInfo& bi = P.blobs[0];
        const uint32_t nl = u.num_layers, SU = u.SU;
        // compact set: every point on a layer >= 1 and every target of an upper-layer edge (a target that is not on the layer
        // itself has an empty row there, as in the dense form)
        std::vector<uint8_t> in_set(u.n, 0);
        for (uint64_t p = 0; p < u.n; ++p)
            if (h_level[u.upper_off + p]) in_set[p] = 1;
        for (uint64_t p = 0; p < u.n; ++p) {
            const uint32_t lv = h_level[u.upper_off + p];
            for (uint32_t layer = 1; layer <= lv && layer < nl; ++layer) {
                const size_t r = (size_t)h_upper_first[u.upper_off + p] + (layer - 1);
                for (uint32_t t = 0; t < SU; ++t) {
                    const uint32_t e = h_adj[u.adjU_off + r * SU + t];
                    if (e != 0xFFFFFFFFu) in_set[e] = 1;
                }
            }
        }
        std::vector<uint32_t> cidx(u.n, 0xFFFFFFFFu);
        for (uint64_t p = 0; p < u.n; ++p)
            if (in_set[p]) { cidx[p] = (uint32_t)h_cids.size(); h_cids.push_back((uint32_t)p); }
        const size_t nu = h_cids.size();
        // affordable: rows (nl-1) * nu * SU words, vectors nu * d floats — a small fraction of the graph unless it is degenerate
        if (nu > 0 && nu <= ((size_t)1 << 22) && nu * 4 <= (size_t)u.n + 4096 && in_set[u.entry_point]) {
            h_crows.assign((size_t)(nl - 1) * nu * SU, 0xFFFFFFFFu);
            for (size_t c = 0; c < nu; ++c) {
                const uint32_t p = h_cids[c];
                const uint32_t lv = h_level[u.upper_off + p];
                for (uint32_t layer = 1; layer <= lv && layer < nl; ++layer) {
                    const size_t r = (size_t)h_upper_first[u.upper_off + p] + (layer - 1);
                    for (uint32_t t = 0; t < SU; ++t) {
                        const uint32_t e = h_adj[u.adjU_off + r * SU + t];
                        h_crows[((size_t)(layer - 1) * nu + c) * SU + t] = e == 0xFFFFFFFFu ? e : cidx[e];
                    }
                }
            }
            h_cvecs.resize(nu * (size_t)dim);
            for (size_t c = 0; c < nu; ++c)
                memcpy(&h_cvecs[c * (size_t)dim], vectors + bi.vec_data_offset + (size_t)h_cids[c] * file_row, (size_t)dim * 4);
            P.nu = (uint32_t)nu;
            P.su = SU;
            P.layers = nl - 1;
            P.small_layer = u.small_layer;
            P.entry_c = cidx[u.entry_point];
            // the TOP set: points on a layer >= 2 and the targets of those layers' edges
            P.nu2 = 0;
            if (nl >= 3) {
                std::vector<uint8_t> in2(nu, 0);
                for (size_t c = 0; c < nu; ++c) {
                    const uint32_t lv = h_level[u.upper_off + h_cids[c]];
                    if (lv >= 2) in2[c] = 1;
                    for (uint32_t layer = 2; layer <= lv && layer < nl; ++layer)
                        for (uint32_t t = 0; t < SU; ++t) {
                            const uint32_t e = h_crows[((size_t)(layer - 1) * nu + c) * SU + t];
                            if (e != 0xFFFFFFFFu) in2[e] = 1;
                        }
                }
                std::vector<uint32_t> c2of(nu, 0xFFFFFFFFu);
                for (size_t c = 0; c < nu; ++c)
                    if (in2[c]) { c2of[c] = (uint32_t)h_map21.size(); h_map21.push_back((uint32_t)c); }
                const size_t nu2 = h_map21.size();
                if (nu2 > 0 && nu2 <= 16384 && in2[P.entry_c]) {
                    h_crows2.assign((size_t)(nl - 2) * nu2 * SU, 0xFFFFFFFFu);
                    for (size_t c2 = 0; c2 < nu2; ++c2)
                        for (uint32_t layer = 2; layer < nl; ++layer)
                            for (uint32_t t = 0; t < SU; ++t) {
                                const uint32_t e = h_crows[((size_t)(layer - 1) * nu + h_map21[c2]) * SU + t];
                                h_crows2[((size_t)(layer - 2) * nu2 + c2) * SU + t] = e == 0xFFFFFFFFu ? e : c2of[e];
                            }
                    h_cvecs2.resize(nu2 * (size_t)dim);
                    for (size_t c2 = 0; c2 < nu2; ++c2)
                        memcpy(&h_cvecs2[c2 * (size_t)dim], &h_cvecs[(size_t)h_map21[c2] * dim], (size_t)dim * 4);
                    P.nu2 = (uint32_t)nu2;
                    P.entry_c2 = c2of[P.entry_c];
                }
            }
        }
    }
    return MDB_OK;
}

// ------------------------------------------------------------------------------------------ IVF
static mdb_status parse_ivf_blob(const uint8_t* b, size_t len, size_t offset, IvfBlobInfo& o, std::string& why) {
    if (!fits(offset, 45, len)) return fail(why, MDB_ERR_FORMAT, "IVF index: header out of bounds");
    const uint8_t* h = b + offset;
    if (h[0] != 0) return fail(why, MDB_ERR_FORMAT, "IVF index: Unknown version: %d", (int)h[0]);
    o.num_features = rd_u32(h + 1);
    o.quantized_dimension = rd_u32(h + 5);
    o.num_clusters = rd_u32(h + 9);
    o.num_vectors = rd_u64(h + 13);
    uint64_t doc_len = rd_u64(h + 21), cent_len = rd_u64(h + 29);
    o.doc_id_mapping_offset = offset + align_up(45, 16);                 // storage.rs:66-67
    // every section length comes from the file: all sums below are overflow-checked against the blob length
    if (!fits(o.doc_id_mapping_offset, doc_len, len - 8)) return fail(why, MDB_ERR_FORMAT, "IVF index: doc-id section out of bounds");
    o.centroid_offset = align_up(o.doc_id_mapping_offset + doc_len, 8);  // :69-72
    if (!fits(o.centroid_offset, cent_len, len - 8)) return fail(why, MDB_ERR_FORMAT, "IVF index: centroid section out of bounds");
    size_t meta = align_up(o.centroid_offset + cent_len, 8);             // :74-75
    if (!fits(meta, 8, len)) return fail(why, MDB_ERR_FORMAT, "IVF index: metadata out of bounds");
    o.num_posting_lists = rd_u64(b + meta);
    o.pl_metadata_offset = meta + 8;
    if (o.num_posting_lists > (len - o.pl_metadata_offset) / 16) return fail(why, MDB_ERR_FORMAT, "IVF index: posting lists out of bounds");
    o.pl_start_offset = o.pl_metadata_offset + o.num_posting_lists * 16;  // :80-82
    // the sections hold a count (u128 / u64) and then one doc id per vector / one row per centroid: the kernels index them by
    // point id < num_vectors and centroid < num_clusters
    if (doc_len < 16 || (doc_len - 16) / 16 < o.num_vectors)
        return fail(why, MDB_ERR_FORMAT, "IVF index: doc-id section of %llu bytes is too short for %llu vectors", (unsigned long long)doc_len,
                    (unsigned long long)o.num_vectors);
    if (cent_len < 8 || (cent_len - 8) / 4 < (uint64_t)o.num_clusters * o.num_features)
        return fail(why, MDB_ERR_FORMAT, "IVF index: centroid section of %llu bytes is too short for %u x %u floats", (unsigned long long)cent_len,
                    o.num_clusters, o.num_features);
    if (o.num_vectors > 0xFFFFFFFEull) return fail(why, MDB_ERR_UNSUPPORTED, "IVF point ids are u32");   // (a doc-id section of 64 GiB)
    return MDB_OK;
}

mdb_status ivf_plan_files(const uint8_t* index, size_t index_len, const uint8_t* vectors, size_t vectors_len,
                          const std::vector<std::pair<size_t, size_t>>& offsets, const mdb_quant_desc* quant, uint32_t shard_rank,
                          uint32_t shard_world, const IvfPlanOpts& opts, IvfPlan& P, std::string& why) {
    P = IvfPlan{};
    if (shard_world == 0) shard_world = 1;
    if (shard_rank >= shard_world) return fail(why, MDB_ERR_INVALID_ARG, "shard_rank >= shard_world");
    const int kind = P.kind = quant ? (int)quant->kind : MDB_QUANT_NONE;
    P.metric = quant ? quant->metric : MDB_METRIC_L2;
    if (kind == MDB_QUANT_PQ) FILES_TRY(pq_shape(quant, P.pq, why));
    const size_t U = offsets.size();
    P.blobs.resize(U);
    P.users.assign(U + 1, IvfUserDev{});  // [U] = sentinel (valid = 0): unknown user => None
    P.list_tile_off.assign(1, 0);
    const bool units = P.units = kind != MDB_QUANT_PQ;   // f32 lists: list_tile_off counts 16-slot units
    const uint32_t pad_units = std::min<uint32_t>(MDB_UPT, std::max<uint32_t>(1, opts.pad_units));
    // list ownership for the multi-GPU path.  Multi-user collections: list l of every user -> rank l % world
    // (a user's ~150 lists spread evenly whatever their sizes).  ONE index (C5: 65 536 lists of very different lengths):
    // size-balanced — lists taken longest first (ties: lower index), each to the least loaded rank (ties: lower rank);
    // every rank parses the same file, so every rank computes the same map.
    std::vector<uint32_t> balanced_owner;
    if (U == 1 && shard_world > 1) {
        IvfBlobInfo b0;
        FILES_TRY(parse_ivf_blob(index, index_len, offsets[0].first, b0, why));
        std::vector<std::pair<uint64_t, uint32_t>> order;  // (num_elem, list)
        for (uint32_t l = 0; l < b0.num_clusters && l < b0.num_posting_lists; ++l) {
            const uint8_t* md = index + b0.pl_metadata_offset + (size_t)l * 16;
            const uint64_t rel = rd_u64(md + 8);
            uint64_t ne = 0;
            if (fits(b0.pl_start_offset, rel, index_len) && fits(b0.pl_start_offset + rel, 32, index_len)) ne = rd_u64(index + b0.pl_start_offset + rel);
            order.push_back({ne, l});
        }
        std::stable_sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        std::vector<uint64_t> load(shard_world, 0);
        balanced_owner.assign(order.size(), 0);
        for (auto& e : order) {
            uint32_t r = 0;
            for (uint32_t i = 1; i < shard_world; ++i) if (load[i] < load[r]) r = i;
            balanced_owner[e.second] = r;
            load[r] += e.first;
        }
    }
    for (size_t ui = 0; ui < U; ++ui) {
        IvfBlobInfo& bi = P.blobs[ui];
        FILES_TRY(parse_ivf_blob(index, index_len, offsets[ui].first, bi, why));
        if (ui == 0) {
            P.num_features = bi.num_features;
            P.quantized_dimension = bi.quantized_dimension;
            // the header against the quantizer the caller opens the index with
            if (kind == MDB_QUANT_PQ) {
                if ((uint32_t)P.pq.m != bi.quantized_dimension) return fail(why, MDB_ERR_FORMAT, "quantized_dimension != dimension / subvector_dimension");
                if ((uint32_t)P.pq.dimension != bi.num_features) return fail(why, MDB_ERR_FORMAT, "PQ dimension != num_features");
            } else {
                if (quant && quant->dimension && quant->dimension != bi.num_features)
                    return fail(why, MDB_ERR_FORMAT, "quantizer dimension != num_features");
                if (bi.quantized_dimension != bi.num_features) return fail(why, MDB_ERR_FORMAT, "NoQuantizer: quantized_dimension != num_features");
            }
        }
        if (bi.num_features != P.num_features || bi.quantized_dimension != P.quantized_dimension)
            return fail(why, MDB_ERR_FORMAT, "users disagree on num_features / quantized_dimension");
        if (bi.num_posting_lists != bi.num_clusters)
            return fail(why, MDB_ERR_FORMAT, "Mismatch between number of clusters (%u) and number of posting lists (%zu)",
                        bi.num_clusters, (size_t)bi.num_posting_lists);
        const size_t esz = kind == MDB_QUANT_PQ ? 1 : 4;
        size_t voff = offsets[ui].second;
        if (!fits(voff, 8, vectors_len)) return fail(why, MDB_ERR_FORMAT, "IVF vector file: header out of bounds");
        if (kind != MDB_QUANT_PQ && (voff + 8) % 4 != 0) return fail(why, MDB_ERR_FORMAT, "IVF f32 vector file is not 4-byte aligned");
        uint64_t nv = rd_u64(vectors + voff);  // async_storage.rs:83-87
        const uint64_t row_bytes = (uint64_t)P.quantized_dimension * esz;
        if (row_bytes == 0 || nv > (vectors_len - voff - 8) / row_bytes)
            return fail(why, MDB_ERR_FORMAT, "vector file: %zu vectors of %u x %zu B exceed the file", (size_t)nv,
                        P.quantized_dimension, esz);
        // The reference bounds a doc-id lookup by the header's count (rs/index/src/ivf/block_based/storage.rs:161, :195) and a vector
        // lookup by the vector file's (vector/async_storage.rs:83-87) and never compares the two: with different counts a posting
        // list may name an id one of them does not cover, and the search fails there.  The writer emits one count; a file with two is
        // refused here, so that point ids, doc ids, tombstone words and filter bitmaps all range over ONE num_vectors.
        if (bi.num_vectors != nv)
            return fail(why, MDB_ERR_FORMAT, "IVF header counts %llu vectors, the vector file %llu", (unsigned long long)bi.num_vectors,
                        (unsigned long long)nv);
        bi.vec_num_vectors = nv;
        bi.vec_data_offset = voff + 8;
        IvfUserDev& u = P.users[ui];
        u.valid = 1;
        u.list_base = (uint32_t)P.list_len.size();
        u.num_lists = bi.num_clusters;
        u.num_vectors = (uint32_t)bi.num_vectors;
        u.doc_ids_off = bi.doc_id_mapping_offset + 16;
        u.tomb_base = (uint32_t)P.tomb_words;
        P.tomb_words += (nv + 31) / 32 + 1;
        P.max_user_vectors = std::max<uint64_t>(P.max_user_vectors, nv);
        P.user_points.push_back(nv);
        u.cent_tile_base = (uint32_t)P.cent_tile_src.size();
        for (uint32_t c0 = 0; c0 < bi.num_clusters; c0 += MDB_TILE) {
            P.cent_tile_src.push_back(bi.centroid_offset + 8);
            P.cent_tile_first.push_back(c0);
            P.cent_tile_limit.push_back(bi.num_clusters);
        }
        for (uint32_t l = 0; l < bi.num_clusters; ++l) {
            const uint8_t* md = index + bi.pl_metadata_offset + (size_t)l * 16;
            const uint64_t rel = rd_u64(md + 8);
            if (!fits(bi.pl_start_offset, rel, index_len)) return fail(why, MDB_ERR_FORMAT, "posting list %u out of bounds", l);
            size_t pl_off = rel + bi.pl_start_offset;  // storage.rs:293-294
            if (pl_off % 8 != 0) return fail(why, MDB_ERR_FORMAT, "posting list %u is not 8-byte aligned", l);
            if (const char* bad = ef_header_error(index + pl_off, index_len - pl_off, nv))
                return fail(why, MDB_ERR_FORMAT, "posting list %u: %s", l, bad);
            uint64_t ne = rd_u64(index + pl_off);
            bool owned = balanced_owner.empty() ? (l % shard_world) == shard_rank : balanced_owner[l] == shard_rank;
            if (!owned) ne = 0;
            P.list_byte_off.push_back(ne ? pl_off : ~0ull);
            P.list_len.push_back((uint32_t)ne);   // (ne <= num_vectors <= 2^32 - 2: ef_header_error)
            uint32_t nt = (uint32_t)((ne + MDB_TILE - 1) / MDB_TILE);
            P.wave_tiles += nt;
            if (units) {   // ceil(ne / 16) units: whole tiles of four, then a narrow tail of 1..3
                nt = (uint32_t)((ne + MDB_UNIT - 1) / MDB_UNIT);
                nt = (nt + pad_units - 1) / pad_units * pad_units;   // MDB_IVF_LIST_PAD_UNITS: 1 (16 slots) | 2 | 4 (= the 64-slot tiles of rounds 1-5)
                const uint32_t u0 = P.list_tile_off.back(), whole = nt & ~(uint32_t)(MDB_UPT - 1), tail = nt - whole;
                for (uint32_t t = 0; t < nt; ++t)
                    P.unit_desc.push_back(((u0 + (t & ~(uint32_t)(MDB_UPT - 1))) << 4) | ((t & (MDB_UPT - 1)) << 2) | (t >= whole ? tail : 0u));
            }
            for (uint32_t t = 0; t < nt; ++t) { P.tile_src.push_back(bi.vec_data_offset); P.tile_limit.push_back((uint32_t)nv); }
            P.list_tile_off.push_back(P.list_tile_off.back() + nt);
            P.total_slots_valid += ne;
            if (P.list_tile_off.back() > (units ? 0x0FFFFFFFull : 0x7FFFFFFFull / MDB_TILE))
                return fail(why, MDB_ERR_UNSUPPORTED, "too many posting-list slots");
        }
    }
    return MDB_OK;
}

// ------------------------------------------------------------------------------------------ multi-user SPANN
mdb_status multi_spann_offsets(const mdb_user_index_info* users, size_t n_users, std::vector<std::pair<size_t, size_t>>& hoff,
                               std::vector<std::pair<size_t, size_t>>& ioff, std::string& why) {
    if (n_users == 0) return fail(why, MDB_ERR_INVALID_ARG, "no users");
    hoff.clear();
    ioff.clear();
    for (size_t i = 0; i < n_users; ++i) {
        hoff.push_back({(size_t)users[i].centroid_index_offset, (size_t)users[i].centroid_vector_offset});
        ioff.push_back({(size_t)users[i].ivf_index_offset, (size_t)users[i].ivf_vectors_offset});
    }
    return MDB_OK;
}

// The host half of mdb_spann_load and mdb_multi_spann_load: the posting lists' plan, then the centroid graphs' — always
// NoQuantizer<L2> over the IVF's num_features (spann/index.rs:19) — BEFORE either is uploaded.  num_features: the argument of
// mdb_multi_spann_load (nullptr: single index).
mdb_status spann_plan_files(const std::vector<std::pair<size_t, size_t>>& hoff, const std::vector<std::pair<size_t, size_t>>& ioff,
                            const uint32_t* num_features, const uint8_t* hnsw_index, size_t hnsw_index_len, const uint8_t* hnsw_vectors,
                            size_t hnsw_vectors_len, const uint8_t* ivf_index, size_t ivf_index_len, const uint8_t* ivf_vectors,
                            size_t ivf_vectors_len, const mdb_quant_desc* quant, uint32_t shard_rank, uint32_t shard_world,
                            const IvfPlanOpts& iopts, const HnswPlanOpts& hopts, IvfPlan& ivf, HnswPlan& hnsw, std::string& why) {
    FILES_TRY(ivf_plan_files(ivf_index, ivf_index_len, ivf_vectors, ivf_vectors_len, ioff, quant, shard_rank, shard_world, iopts, ivf, why));
    if (num_features && ivf.num_features != *num_features)
        return fail(why, MDB_ERR_FORMAT, "num_features %u != index header %u", *num_features, ivf.num_features);
    mdb_quant_desc noq{};
    noq.kind = MDB_QUANT_NONE;
    noq.metric = MDB_METRIC_L2;
    noq.dimension = ivf.num_features;
    return hnsw_plan_files(hnsw_index, hnsw_index_len, hnsw_vectors, hnsw_vectors_len, hoff, &noq, ivf.num_features, hopts, hnsw, why);
}

// ------------------------------------------------------------------------------------------ C ABI: the checkers
static mdb_status report(mdb_status st, const std::string& msg, char* why, size_t why_cap) {
    if (why && why_cap) {
        size_t n = st == MDB_OK ? 0 : std::min(msg.size(), why_cap - 1);
        memcpy(why, msg.data(), n);
        why[n] = 0;
    }
    return st;
}

extern "C" {

mdb_status mdb_hnsw_check_files(const void* index_bytes, size_t index_len, size_t index_offset, const void* vectors_bytes,
                                size_t vectors_len, size_t vectors_offset, const mdb_quant_desc* quant, char* why, size_t why_cap) {
    if (!index_bytes || !vectors_bytes) return report(MDB_ERR_INVALID_ARG, "null file", why, why_cap);
    std::string msg;
    uint32_t dim = 0;
    mdb_status st = hnsw_file_dimension((const uint8_t*)index_bytes, index_len, index_offset, quant, &dim, msg);
    HnswPlan plan;
    if (st == MDB_OK)
        st = hnsw_plan_files((const uint8_t*)index_bytes, index_len, (const uint8_t*)vectors_bytes, vectors_len,
                             {{index_offset, vectors_offset}}, quant, dim, HnswPlanOpts{}, plan, msg);
    return report(st, msg, why, why_cap);
}

mdb_status mdb_ivf_check_files(const void* index_bytes, size_t index_len, size_t index_offset, const void* vectors_bytes,
                               size_t vectors_len, size_t vectors_offset, const mdb_quant_desc* quant, uint32_t shard_rank,
                               uint32_t shard_world, char* why, size_t why_cap) {
    if (!index_bytes || !vectors_bytes) return report(MDB_ERR_INVALID_ARG, "null file", why, why_cap);
    std::string msg;
    IvfPlan plan;
    mdb_status st = ivf_plan_files((const uint8_t*)index_bytes, index_len, (const uint8_t*)vectors_bytes, vectors_len,
                                   {{index_offset, vectors_offset}}, quant, shard_rank, shard_world, IvfPlanOpts{}, plan, msg);
    return report(st, msg, why, why_cap);
}

mdb_status mdb_spann_check_files(const void* hnsw_index, size_t hnsw_index_len, size_t hnsw_index_offset, const void* hnsw_vectors,
                                 size_t hnsw_vectors_len, size_t hnsw_vectors_offset, const void* ivf_index, size_t ivf_index_len,
                                 size_t ivf_index_offset, const void* ivf_vectors, size_t ivf_vectors_len, size_t ivf_vectors_offset,
                                 const mdb_quant_desc* quant, char* why, size_t why_cap) {
    if (!hnsw_index || !hnsw_vectors || !ivf_index || !ivf_vectors) return report(MDB_ERR_INVALID_ARG, "null file", why, why_cap);
    std::string msg;
    IvfPlan ivf;
    HnswPlan hnsw;
    mdb_status st = spann_plan_files({{hnsw_index_offset, hnsw_vectors_offset}}, {{ivf_index_offset, ivf_vectors_offset}}, nullptr,
                                     (const uint8_t*)hnsw_index, hnsw_index_len, (const uint8_t*)hnsw_vectors, hnsw_vectors_len,
                                     (const uint8_t*)ivf_index, ivf_index_len, (const uint8_t*)ivf_vectors, ivf_vectors_len, quant, 0, 1,
                                     IvfPlanOpts{}, HnswPlanOpts{}, ivf, hnsw, msg);
    return report(st, msg, why, why_cap);
}

mdb_status mdb_multi_spann_check_files(const mdb_user_index_info* users, size_t n_users, uint32_t num_features, const void* hnsw_index,
                                       size_t hnsw_index_len, const void* hnsw_vectors, size_t hnsw_vectors_len, const void* ivf_index,
                                       size_t ivf_index_len, const void* ivf_vectors, size_t ivf_vectors_len, const mdb_quant_desc* quant,
                                       uint32_t shard_rank, uint32_t shard_world, char* why, size_t why_cap) {
    if ((!users && n_users) || !hnsw_index || !hnsw_vectors || !ivf_index || !ivf_vectors)
        return report(MDB_ERR_INVALID_ARG, "null file", why, why_cap);
    std::string msg;
    std::vector<std::pair<size_t, size_t>> hoff, ioff;
    mdb_status st = multi_spann_offsets(users, n_users, hoff, ioff, msg);
    IvfPlan ivf;
    HnswPlan hnsw;
    if (st == MDB_OK)
        st = spann_plan_files(hoff, ioff, &num_features, (const uint8_t*)hnsw_index, hnsw_index_len, (const uint8_t*)hnsw_vectors,
                              hnsw_vectors_len, (const uint8_t*)ivf_index, ivf_index_len, (const uint8_t*)ivf_vectors, ivf_vectors_len, quant,
                              shard_rank, shard_world, IvfPlanOpts{}, HnswPlanOpts{}, ivf, hnsw, msg);
    return report(st, msg, why, why_cap);
}

}  // extern "C"

// mdb_files.h — the HOST halves of the loaders: everything *_load decides from the bytes of the on-disk files before its first
// device call.  Each function takes host mappings of the files and produces the PLAN its loader uploads (blob infos, adjacency,
// levels, compact upper layers, list tables) or a status and a message.  No mdb_ctx, no HIP call, no environment: this header and
// mdb_files.cpp compile with a plain C++ compiler (tests/host/check_files_main.cpp runs them under the sanitizers), and the
// mdb_*_check_files entries of the C ABI are these functions with the plan dropped.  One set of rules: what a checker accepts is
// what the loader uploads.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/muopdb_hip.h"

#define MDB_TILE 64          // vectors per tile of the list-contiguous SoA layout (one per lane)
#define MDB_UNIT 16          // f32 posting lists: slots per unit (a tile = four units 64 wide; a list's tail tile is 1-3 units, 16-48 wide: mdb_ivf.hip)
#define MDB_UPT (MDB_TILE / MDB_UNIT)   // units per whole tile
#define MDB_HNSW_MAX_DEGREE 256  // largest node degree a graph may have: HNSW_MAX_STRIDE of mdb_hnsw.hip (static_assert there)
#define MDB_HNSW_MAX_LAYERS 255  // levels are u8 on the device (HnswSet::d_level)
#define MDB_MAX_K 2048       // largest top-k / ef served by the on-chip selectors

// ------------------------------------------------------------------------------------------
// exact-association distance plan (host computed, passed by value to kernels)
//   L2  : rs/utils/src/distance/l2.rs:32-67   passes where len/16>0, len/8>0, len/4>0, tail
//   dot : rs/utils/src/distance/dot_product.rs:38-71  passes where len>16, len>8, len>4, tail
// all pass offsets are multiples of 4, so every chunk is a whole number of float4s.
// ------------------------------------------------------------------------------------------
struct DistPlan {
    int d;            // true dimension
    int d4;           // float4s per vector (ceil(d/4))
    int n16, n8, n4;  // chunks per pass
    int off8, off4, offt;  // element offsets of the 8-pass, 4-pass and scalar tail
    int ntail;
};

inline DistPlan make_plan(int d, int metric) {
    DistPlan p{};
    p.d = d;
    p.d4 = (d + 3) / 4;
    int rem = d, off = 0;
    if (metric != MDB_METRIC_DOT) {
        p.n16 = rem / 16; off += p.n16 * 16; rem -= p.n16 * 16;
        p.off8 = off; p.n8 = rem / 8; off += p.n8 * 8; rem -= p.n8 * 8;
        p.off4 = off; p.n4 = rem / 4; off += p.n4 * 4; rem -= p.n4 * 4;
    } else {
        p.n16 = rem > 16 ? rem / 16 : 0; off += p.n16 * 16; rem -= p.n16 * 16;
        p.off8 = off; p.n8 = rem > 8 ? rem / 8 : 0; off += p.n8 * 8; rem -= p.n8 * 8;
        p.off4 = off; p.n4 = rem > 4 ? rem / 4 : 0; off += p.n4 * 4; rem -= p.n4 * 4;
    }
    p.offt = off;
    p.ntail = rem;
    return p;
}

// host-side byte readers (little-endian files)
static inline uint32_t rd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static inline uint64_t rd_u64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) & ~(a - 1); }
// overflow-checked a + b <= limit
static inline bool fits(uint64_t a, uint64_t b, uint64_t limit) { return a <= limit && b <= limit - a; }
// Host-side validation of one serialized Elias-Fano list (ef.rs:197-215 header: n, L, lower_words, upper_words) of `avail`
// bytes BEFORE the device decoder trusts it: a corrupt header would otherwise make ef_low_bits read lower[w + 1] past the
// blob, or shift by >= 64.  The encoder writes lower_words == ceil(n * L / 64) and at least n upper bits.
static inline const char* ef_header_error(const uint8_t* p, uint64_t avail, uint64_t max_n) {
    if (avail < 32) return "Not enough metadata for EliasFano encoded data";
    const uint64_t n = rd_u64(p), L = rd_u64(p + 8), lw = rd_u64(p + 16), uw = rd_u64(p + 24);
    const uint64_t words = (avail - 32) / 8;
    if (lw > words || uw > words - lw) return "EliasFano list truncated (word counts exceed the blob)";
    if (L >= 64) return "EliasFano lower_bit_length >= 64";
    if (n > max_n) return "EliasFano num_elem exceeds the number of vectors";
    if (n && L && (n > (~0ull) / L || lw < (n * L + 63) / 64)) return "EliasFano lower_words < ceil(num_elem * lower_bit_length / 64)";
    if (uw > (~0ull) / 64 || uw * 64 < n) return "EliasFano upper stream shorter than num_elem bits";
    return nullptr;
}

// the shape of a product quantizer (pq/mod.rs:23-39) once its descriptor has been accepted; `need` floats of codebook are read
struct PqShape {
    int metric = 0, dimension = 0, subdim = 0, num_bits = 0, m = 0, K = 0;
    size_t need = 0;
};
mdb_status pq_shape(const mdb_quant_desc* q, PqShape& o, std::string& why);

// ------------------------------------------------------------------------------------------ HNSW
// per-user (per-graph) descriptor read by the traversal kernel
struct HnswUserDev {
    uint32_t valid;
    uint32_t n;            // number of vectors (point ids are < n)
    uint32_t n0;           // number of layer-0 adjacency rows
    uint32_t num_layers;
    uint32_t entry_point;  // graph_storage.rs:527-558
    uint32_t S0, SU;       // fixed row strides of the layer-0 / upper-layer adjacency
    uint32_t small_layer;  // every layer >= small_layer (> 0) holds <= 64 points and only edges among them; else num_layers
    uint64_t adj0_off;     // u32 index into the adjacency arena
    uint64_t adjU_off;
    uint64_t adjD_off;     // DENSE upper layers: row of (layer, point) at adjD_off + ((layer-1) * n + point) * SU — ~0 when not built
    uint64_t upper_off;    // index into upper_first[] / level[] (per point)
    uint64_t vec_off;      // float index into the vector arena (row stride dpad)
    uint64_t doc_ids_off;  // byte offset of doc id 0 inside the uploaded index bytes
};

struct HnswBlobInfo {
    uint32_t quantized_dimension = 0, num_layers = 0;
    uint64_t edges_len = 0, points_len = 0, edge_offsets_len = 0, level_offsets_len = 0, doc_id_mapping_len = 0;
    size_t edges_offset = 0, points_offset = 0, edge_offsets_offset = 0, level_offsets_offset = 0, doc_id_mapping_offset = 0;
    uint64_t num_vectors = 0;
    size_t vec_data_offset = 0;
};

// the load-time switches the plan depends on (mdb_options: MDB_HNSW_NO_DENSE, MDB_HNSW_NO_TABLE)
struct HnswPlanOpts {
    bool no_dense = false, no_table = false;
};

// what HnswSet::load uploads
struct HnswPlan {
    int kind = MDB_QUANT_NONE, metric = MDB_METRIC_L2;
    PqShape pq;                    // kind == MDB_QUANT_PQ
    uint32_t dimension = 0;
    int dpad = 0;
    size_t file_row = 0;           // bytes of one stored vector in the file: f32 row, or m u8 codes (BlockBasedHnsw<ProductQuantizer>)
    std::vector<HnswBlobInfo> blobs;
    std::vector<HnswUserDev> users;   // [U] = sentinel (valid = 0): unknown user => None
    uint32_t max_n = 0, max_stride = 0, max_rows0 = 0, max_rowsU = 0;
    bool all_dense = true;
    std::vector<uint32_t> adj, upper_first;
    std::vector<uint8_t> level;
    std::vector<uint64_t> row_src;    // per stored row: its byte offset in the vector file
    // the table path's compact upper layers (HnswUpper): nu == 0 when not built
    uint32_t nu = 0, su = 0, layers = 0, small_layer = 0, entry_c = 0, nu2 = 0, entry_c2 = 0;
    std::vector<uint32_t> cids, crows, crows2, map21;
    std::vector<float> cvecs, cvecs2;
};
// offsets[u] = (byte offset of user u's graph in `index`, of its vector file in `vectors`)
mdb_status hnsw_plan_files(const uint8_t* index, size_t index_len, const uint8_t* vectors, size_t vectors_len,
                           const std::vector<std::pair<size_t, size_t>>& offsets, const mdb_quant_desc* quant, uint32_t dim,
                           const HnswPlanOpts& opts, HnswPlan& plan, std::string& why);
// the dimension mdb_hnsw_load searches with: the descriptor's, else the header's quantized_dimension
mdb_status hnsw_file_dimension(const uint8_t* index, size_t index_len, size_t index_offset, const mdb_quant_desc* quant, uint32_t* dim,
                               std::string& why);

// ------------------------------------------------------------------------------------------ IVF
// per-user (per-blob) descriptor read by the kernels
struct IvfUserDev {
    uint32_t valid;           // 0 for an unknown user (search returns None)
    uint32_t list_base;       // global index of the user's list 0
    uint32_t num_lists;       // = num_clusters
    uint32_t num_vectors;
    uint32_t tomb_base;       // word offset into the tombstone arena
    uint32_t cent_tile_base;  // first tile of the user's centroids in the centroid tile arena
    uint64_t doc_ids_off;     // byte offset of doc id 0 inside the uploaded index bytes
};

// host-side parse of one blob (rs/index/src/ivf/block_based/storage.rs:52-138)
struct IvfBlobInfo {
    uint32_t num_features = 0, quantized_dimension = 0, num_clusters = 0;
    uint64_t num_vectors = 0, num_posting_lists = 0;
    size_t doc_id_mapping_offset = 0, centroid_offset = 0, pl_metadata_offset = 0, pl_start_offset = 0;
    uint64_t vec_num_vectors = 0;
    size_t vec_data_offset = 0;
};

struct IvfPlanOpts {
    uint32_t pad_units = 1;   // MDB_IVF_LIST_PAD_UNITS, clamped to 1 .. MDB_UPT
};

// what IvfSet::load uploads
struct IvfPlan {
    int kind = MDB_QUANT_NONE, metric = MDB_METRIC_L2;
    PqShape pq;                            // kind == MDB_QUANT_PQ
    uint32_t num_features = 0, quantized_dimension = 0;
    bool units = true;                     // f32 lists: list_tile_off counts 16-slot units
    std::vector<IvfBlobInfo> blobs;
    std::vector<IvfUserDev> users;         // [U] = sentinel (valid = 0): unknown user => None
    std::vector<uint64_t> list_byte_off;   // per global list (or ~0 when not owned / empty)
    std::vector<uint32_t> list_len;
    std::vector<uint32_t> list_tile_off;
    std::vector<uint64_t> tile_src;        // per tile (f32 lists: per 16-slot unit): byte offset of the user's vector 0
    std::vector<uint32_t> tile_limit;      // per tile (unit): user's num_vectors
    std::vector<uint32_t> unit_desc;       // f32 lists: gather_f32_units_kernel's unit descriptors
    std::vector<uint64_t> cent_tile_src;
    std::vector<uint32_t> cent_tile_first, cent_tile_limit;
    size_t wave_tiles = 0, tomb_words = 0, total_slots_valid = 0;
    uint64_t max_user_vectors = 0;
    std::vector<uint64_t> user_points;
};
mdb_status ivf_plan_files(const uint8_t* index, size_t index_len, const uint8_t* vectors, size_t vectors_len,
                          const std::vector<std::pair<size_t, size_t>>& offsets, const mdb_quant_desc* quant, uint32_t shard_rank,
                          uint32_t shard_world, const IvfPlanOpts& opts, IvfPlan& plan, std::string& why);

// ------------------------------------------------------------------------------------------ SPANN
// the (graph, vector file) and (IVF index, vector file) offsets of every user record, and the multi-user rules that need no file
mdb_status multi_spann_offsets(const mdb_user_index_info* users, size_t n_users, std::vector<std::pair<size_t, size_t>>& hoff,
                               std::vector<std::pair<size_t, size_t>>& ioff, std::string& why);
// the host half of mdb_spann_load / mdb_multi_spann_load: both plans, before either half is uploaded (num_features: the argument of
// mdb_multi_spann_load, nullptr for a single index)
mdb_status spann_plan_files(const std::vector<std::pair<size_t, size_t>>& hoff, const std::vector<std::pair<size_t, size_t>>& ioff,
                            const uint32_t* num_features, const uint8_t* hnsw_index, size_t hnsw_index_len, const uint8_t* hnsw_vectors,
                            size_t hnsw_vectors_len, const uint8_t* ivf_index, size_t ivf_index_len, const uint8_t* ivf_vectors,
                            size_t ivf_vectors_len, const mdb_quant_desc* quant, uint32_t shard_rank, uint32_t shard_world,
                            const IvfPlanOpts& iopts, const HnswPlanOpts& hopts, IvfPlan& ivf, HnswPlan& hnsw, std::string& why);

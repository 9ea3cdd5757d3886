"""Field-aware mutations of the on-disk index files, one case per way a loader's host half can be handed a malformed file.

The loaders (`mdb_hnsw_load`, `mdb_ivf_load`, `mdb_spann_load`, `mdb_multi_spann_load`) turn host mappings of files into device offsets
the kernels trust; what their host halves (muopdb_amd/csrc/mdb_files.cpp) let through, a kernel later dereferences.  Each case here is

    Case(name, loader, files, args, status, aim)

`files` are the bytes AFTER the mutation, `args` the remaining arguments of the loader (offsets, quantizer descriptor, user records),
`status` the expected return (MDB_ERR_FORMAT unless the limits table of include/muopdb_hip.h names another; MDB_OK for the benign
mutations, which must be accepted and served), `aim` a fragment of the refusal's message: the check the case was written for.

No random bytes: the base files are written with muopdb_amd.formats from fixed seeds — the smallest that still have every section
non-trivial — and every mutation names a field, a boundary or an element.  tests/test_file_refusal.py runs the table through the
host-only checkers (no GPU) and through a stand-alone sanitizer build; tests/test_gpu_file_refusal.py runs the loaders."""
import collections
import ctypes as C
import struct

import numpy as np

from muopdb_amd import formats as F

OK, INVALID_ARG, FORMAT, UNSUPPORTED = 0, 1, 2, 7
U64 = (1 << 64) - 1

Case = collections.namedtuple("Case", "name loader files args status aim")

DIM, SUBDIM, BITS = 8, 2, 4          # PQ: m = 4 codes per vector, 16 codewords per subspace
M = DIM // SUBDIM


# ----------------------------------------------------------------------------------- base files
def _knn(x, k):
    d = ((x[:, None, :].astype(np.float64) - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def _graph_layers(x, upper_sizes, k0, ku, seed):
    """A hand-made layered graph over the rows of x: layer 0 = every point to its k0 nearest; upper layer i = a seeded subset (nested:
    each a subset of the one below) to its ku nearest inside the subset.  Upper layers list their points in ascending id, the top
    layer's first point is the entry point (the reader's rule).  Any graph of the format serves: searches are compared on the same bytes."""
    rng = np.random.default_rng(seed)
    n = x.shape[0]
    layers = [{p: [int(e) for e in nb] for p, nb in enumerate(_knn(x, min(k0, n - 1)))}]
    pts = np.arange(n)
    for size in upper_sizes:
        pts = np.sort(rng.choice(pts, size=size, replace=False))
        nb = _knn(x[pts], min(ku, size - 1)) if size > 1 else np.zeros((1, 0), np.int64)
        layers.append({int(p): [int(pts[e]) for e in nb[i]] for i, p in enumerate(pts)})
    return layers


def _codebook(seed):
    return np.random.default_rng(seed).standard_normal(M * (1 << BITS) * SUBDIM).astype(np.float32)


def _quantize(x, cb):
    cb = cb.reshape(M, 1 << BITS, SUBDIM)
    sub = x.reshape(x.shape[0], M, 1, SUBDIM)
    return ((sub - cb[None]) ** 2).sum(-1).argmin(-1).astype(np.uint8)


def noq(dimension=DIM):
    return dict(kind=0, metric=0, dimension=dimension, subvector_dimension=0, num_bits=0, codebook=None)


def pq(cb, dimension=DIM, subvector_dimension=SUBDIM, num_bits=BITS):
    return dict(kind=1, metric=0, dimension=dimension, subvector_dimension=subvector_dimension, num_bits=num_bits, codebook=cb)


def _ivf_files(x, doc_ids, lists, seed, codes_of=None):
    """`lists` centroids of which the LAST gets no vector (an empty posting list): it sits far from every row"""
    rng = np.random.default_rng(seed)
    cent = x[rng.choice(x.shape[0], lists - 1, replace=False)].copy()
    a = ((x[:, None, :] - cent[None]) ** 2).sum(-1).argmin(1)
    cent = np.concatenate([cent, np.full((1, x.shape[1]), 1000.0, np.float32)]).astype(np.float32)
    pls = [np.flatnonzero(a == c).astype(np.uint64) for c in range(lists)]
    stored = x if codes_of is None else codes_of(x)
    return F.write_ivf_index(cent, doc_ids, pls, quantized_dimension=stored.shape[1]), F.write_vector_file(stored), cent


def _spann_files(n, lists, seed, codes_of=None):
    x = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    iidx, ivec, cent = _ivf_files(x, [1000 * seed + i for i in range(n)], lists, seed, codes_of)
    layers = _graph_layers(cent, (3,), 4, 2, seed)
    return dict(hnsw_index=F.write_hnsw_index(layers, list(range(lists)), DIM), hnsw_vectors=F.write_vector_file(cent),
                ivf_index=iidx, ivf_vectors=ivec)


_BASE = {}


def base():
    """{name: (loader, files, args)} — built once"""
    if _BASE:
        return _BASE
    rng = np.random.default_rng(20)
    x = rng.standard_normal((200, DIM)).astype(np.float32)
    layers = _graph_layers(x, (24, 4), 6, 4, 21)
    docs = [(7 << 64) + 3 * i for i in range(200)]
    cb = _codebook(22)
    _BASE["hnsw"] = ("hnsw", dict(index=F.write_hnsw_index(layers, docs, DIM), vectors=F.write_vector_file(x)),
                     dict(quant=noq()))
    _BASE["hnsw_pq"] = ("hnsw", dict(index=F.write_hnsw_index(layers, docs, M), vectors=F.write_vector_file(_quantize(x, cb))),
                        dict(quant=pq(cb)))
    y = rng.standard_normal((300, DIM)).astype(np.float32)
    idocs = [(1 << 70) + 5 * i for i in range(300)]
    iidx, ivec, _ = _ivf_files(y, idocs, 7, 23)
    _BASE["ivf"] = ("ivf", dict(index=iidx, vectors=ivec), dict(quant=noq()))
    pidx, pvec, _ = _ivf_files(y, idocs, 7, 23, lambda v: _quantize(v, cb))
    _BASE["ivf_pq"] = ("ivf", dict(index=pidx, vectors=pvec), dict(quant=pq(cb)))
    _BASE["spann"] = ("spann", _spann_files(300, 7, 24), dict(quant=noq()))
    _BASE["spann_pq"] = ("spann", _spann_files(300, 7, 25, lambda v: _quantize(v, cb)), dict(quant=pq(cb)))
    users = {11: _spann_files(120, 5, 26), (1 << 64) + 2: _spann_files(90, 4, 27), 12: _spann_files(150, 6, 28)}
    cat = F.concat_multi_spann(users)
    _BASE["multi"] = ("multi", {k: cat[k] for k in ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors", "user_table")},
                      dict(quant=noq(), num_features=DIM))
    return _BASE


# ----------------------------------------------------------------------------------- layouts
HNSW_FIELDS = dict(quantized_dimension=(1, "<I"), num_layers=(5, "<I"), edges_len=(9, "<Q"), points_len=(17, "<Q"),
                   edge_offsets_len=(25, "<Q"), level_offsets_len=(33, "<Q"), doc_id_mapping_len=(41, "<Q"))
IVF_FIELDS = dict(num_features=(1, "<I"), quantized_dimension=(5, "<I"), num_clusters=(9, "<I"), num_vectors=(13, "<Q"),
                  doc_id_mapping_len=(21, "<Q"), centroids_len=(29, "<Q"), posting_lists_and_metadata_len=(37, "<Q"))


def get(buf, fields, name, off=0):
    o, fmt = fields[name]
    return struct.unpack_from(fmt, buf, off + o)[0]


def put(buf, fields, name, value, off=0):
    """a copy of `buf` with the header field set (values are taken modulo the field's width)"""
    o, fmt = fields[name]
    out = bytearray(buf)
    struct.pack_into(fmt, out, off + o, value & ((1 << (8 * struct.calcsize(fmt))) - 1))
    return bytes(out)


def poke(buf, at, fmt, value):
    out = bytearray(buf)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def _up(x, a):
    return (x + a - 1) // a * a


def hnsw_layout(buf, off=0):
    """section offsets of a graph file as the reader computes them (graph_storage.rs:170-196)"""
    h = {k: get(buf, HNSW_FIELDS, k, off) for k in HNSW_FIELDS}
    h["edges"] = _up(off + 49, 4)
    h["points"] = h["edges"] + h["edges_len"]
    h["edge_offsets"] = _up(h["points"] + h["points_len"], 8)
    h["level_offsets"] = h["edge_offsets"] + h["edge_offsets_len"]
    h["doc_ids"] = _up(h["level_offsets"] + h["level_offsets_len"], 16)
    h["end"] = h["doc_ids"] + h["doc_id_mapping_len"]
    inside = h["level_offsets"] + h["level_offsets_len"] <= len(buf)
    h["levels"] = list(struct.unpack_from("<%dQ" % (h["level_offsets_len"] // 8), buf, h["level_offsets"])) if inside else []
    return h


def ivf_layout(buf, off=0):
    """section offsets of an IVF index file (ivf/block_based/storage.rs:52-91)"""
    h = {k: get(buf, IVF_FIELDS, k, off) for k in IVF_FIELDS}
    h["doc_ids"] = off + 48
    h["centroids"] = _up(h["doc_ids"] + h["doc_id_mapping_len"], 8)
    h["meta"] = _up(h["centroids"] + h["centroids_len"], 8)
    h["num_posting_lists"] = struct.unpack_from("<Q", buf, h["meta"])[0]
    h["pl_meta"] = h["meta"] + 8
    h["pl_start"] = h["pl_meta"] + 16 * h["num_posting_lists"]
    h["lists"] = [h["pl_start"] + struct.unpack_from("<Q", buf, h["pl_meta"] + 16 * l + 8)[0] for l in range(h["num_posting_lists"])]
    return h


# ----------------------------------------------------------------------------------- the table
def _with(files, **changed):
    out = dict(files)
    out.update(changed)
    return out


def _cuts(length, boundaries):
    """0, inside the header, every boundary and one byte to either side — strictly shorter than the file"""
    at = {0, 20}
    for b in boundaries:
        at.update((b - 1, b, b + 1))
    return sorted(c for c in at if 0 <= c < length)


def _field_values(cur, elem):
    """-1 element, +1 element, 0, len + 1, 2^63, 2^64 - 1 (a value equal to the field is no mutation)"""
    vals = [("minus1", cur - elem), ("plus1", cur + elem), ("zero", 0), ("len_plus1", cur + 1), ("2p63", 1 << 63), ("max", U64)]
    return [(n, v) for n, v in vals if v != cur and v >= 0]


def _absorbed(index, mutated, off, field, delta):
    """A LONGER section length that the format itself cannot tell from a well-formed file: the growth is swallowed by the alignment
    padding behind the section (or, for a graph inside a collection, by the next user's bytes that follow its doc ids), so that the
    sections that hold the graph's structure — edge offsets, level offsets — stay where they were and the file still holds every
    section.  What the reader then sees: the same graph with trailing elements nothing indexes (points_len, level_offsets_len,
    doc_id_mapping_len: every index into them comes from level_offsets / edge_offsets / point ids < num_vectors, all unchanged);
    for edges_len grown by whole elements, the points section read one element later and closed by the padding's zero bytes, i.e.
    point id 0; for level_offsets_len inside a collection, the doc ids read 16 bytes later (any 16 bytes are a doc id).  Each is
    another well-formed file — the writers pad with zeros — and is accepted and served like any other.  A single graph file ends
    with its doc ids, so there only the padding can absorb anything."""
    if delta <= 0 or (field == "edges_len" and delta % 4):
        return False
    a, b = hnsw_layout(index, off), hnsw_layout(mutated, off)
    return b["end"] <= len(mutated) and all(a[s] == b[s] for s in ("edge_offsets", "level_offsets"))


def _hnsw_cases(tag, loader_files_args):
    """mutations of one graph file + vector file: `mk(index=..., vectors=...)` puts them back into the loader's file set"""
    cases = []
    loader, files, args, ikey, vkey, off, voff = loader_files_args
    index, vectors = files[ikey], files[vkey]
    lay = hnsw_layout(index, off)
    nl, nv = lay["num_layers"], struct.unpack_from("<Q", vectors, voff)[0]

    def add(name, status, aim, index_=None, vectors_=None, args_=None):
        f = dict(files)
        if index_ is not None:
            f[ikey] = index_
        if vectors_ is not None:
            f[vkey] = vectors_
        cases.append(Case("%s.%s" % (tag, name), loader, f, dict(args, **(args_ or {})), status, aim))

    whole = off == 0 and lay["end"] == len(index)
    if whole:   # truncations: the graph file, then its vector file
        for c in _cuts(len(index), [lay[s] for s in ("edges", "points", "edge_offsets", "level_offsets", "doc_ids")] + [49]):
            add("index_cut_%d" % c, FORMAT, "header out of bounds" if c < 49 else "", index_=index[:c])
        for c in _cuts(len(vectors), [8, len(vectors)]):
            add("vectors_cut_%d" % c, FORMAT, "vector file: header out of bounds" if c < 8 else "vector file truncated", vectors_=vectors[:c])
    # every length field of the header
    for name, elem in (("edges_len", 4), ("points_len", 4), ("edge_offsets_len", 8), ("level_offsets_len", 8), ("doc_id_mapping_len", 16)):
        for vn, v in _field_values(lay[name], elem):
            mutated = put(index, HNSW_FIELDS, name, v, off)
            aim = "a section is longer than the file" if vn in ("2p63", "max") else ""   # (the other values shift what follows: which check sees it first depends on the bytes)
            add("%s_%s" % (name, vn), OK if _absorbed(index, mutated, off, name, v - lay[name]) else FORMAT, aim, index_=mutated)
    add("version_1", FORMAT, "Unknown version", index_=poke(index, off, "<B", 1))
    # num_layers == 0 over a non-empty graph: refused, see parse_hnsw_blob (rs/index/src/hnsw/block_based/graph_storage.rs:549-553)
    add("num_layers_0_nonempty", FORMAT, "num_layers is 0", index_=put(index, HNSW_FIELDS, "num_layers", 0, off))
    add("num_layers_plus1", FORMAT, "level_offsets too short", index_=put(index, HNSW_FIELDS, "num_layers", nl + 1, off))
    add("num_layers_256", UNSUPPORTED, "more than 255", index_=put(index, HNSW_FIELDS, "num_layers", 256, off))
    add("num_layers_2p32m1", UNSUPPORTED, "more than 255", index_=put(index, HNSW_FIELDS, "num_layers", (1 << 32) - 1, off))
    add("quantized_dimension_0", FORMAT, "quantized_dimension", index_=put(index, HNSW_FIELDS, "quantized_dimension", 0, off))
    add("quantized_dimension_plus1", FORMAT, "quantized_dimension",
        index_=put(index, HNSW_FIELDS, "quantized_dimension", lay["quantized_dimension"] + 1, off))
    # level_offsets
    lo, levels = lay["level_offsets"], lay["levels"]
    n_eo, n_pts = lay["edge_offsets_len"] // 8, lay["points_len"] // 4
    if nl >= 3:
        add("level_offsets_not_monotone", FORMAT, "decrease", index_=poke(index, lo + 8, "<Q", levels[2] + 1))
    add("level_offsets_last_past_edge_offsets", FORMAT, "level offset out of bounds", index_=poke(index, lo + 8 * nl, "<Q", n_eo + 1))
    add("level_offsets_last_2p63", FORMAT, "level offset out of bounds", index_=poke(index, lo + 8 * nl, "<Q", 1 << 63))
    if nl >= 2:
        add("level_offsets_first_past_points", FORMAT, "", index_=poke(index, lo, "<Q", n_pts))
        add("top_layer_empty", FORMAT, "top layer is empty", index_=poke(index, lo + 8, "<Q", levels[0]))
        add("layer0_starts_past_points", FORMAT, "points section too short", index_=poke(index, lo + 8 * (nl - 1), "<Q", n_pts + 1))
    # edge_offsets
    eo, s0 = lay["edge_offsets"], levels[nl - 1]
    n_edges = lay["edges_len"] // 4
    add("edge_offsets_decreasing_layer0", FORMAT, "edge offsets corrupt", index_=poke(index, eo + 8 * (s0 + 3), "<Q", 0))
    add("edge_offsets_last_past_edges", FORMAT, "edge offsets corrupt", index_=poke(index, eo + 8 * (n_eo - 1), "<Q", n_edges + 1))
    add("edge_offsets_last_max", FORMAT, "edge offsets corrupt", index_=poke(index, eo + 8 * (n_eo - 1), "<Q", U64))
    if nl >= 2:
        add("edge_offsets_decreasing_upper", FORMAT, "upper-layer edge offsets corrupt", index_=poke(index, eo + 8, "<Q", U64))
    # points: an id >= num_vectors on each upper layer; the first of the top layer is the entry point
    pts = lay["points"]
    for layer in range(1, nl):
        first = levels[nl - 1 - layer]
        add("point_out_of_range_layer%d%s" % (layer, "_entry" if layer == nl - 1 else ""), FORMAT,
            "entry point" if layer == nl - 1 else "upper-layer point id out of range", index_=poke(index, pts + 4 * first, "<I", nv))
        add("point_2p32m1_layer%d" % layer, FORMAT, "", index_=poke(index, pts + 4 * (first + 1), "<I", (1 << 32) - 1))
    # edges: num_vectors, 2^32 - 2 and 2^32 - 1 (the in-memory empty-slot value) on layer 0 and on an upper layer
    ed = lay["edges"]
    e0 = struct.unpack_from("<Q", index, eo + 8 * s0)[0]          # first edge of layer 0's point 0
    for vn, v in (("nv", nv), ("2p32m2", (1 << 32) - 2), ("2p32m1", (1 << 32) - 1)):
        add("edge_%s_layer0" % vn, FORMAT, "is outside the vector storage", index_=poke(index, ed + 4 * e0, "<I", v))
        if nl >= 2:
            add("edge_%s_upper" % vn, FORMAT, "upper-layer edge", index_=poke(index, ed, "<I", v))
    return cases, lay, nv


def _single_layer_graph(x, slots, docs, edges_from=0):
    """a one-layer graph file with `slots` layer-0 rows over x.shape[0] vectors; rows below `edges_from` have no edge"""
    n = x.shape[0]
    nb = _knn(x, 4)
    layer = {p: ([int(e) for e in nb[p]] if edges_from <= p < n else []) for p in range(slots)}
    if slots > n and edges_from >= n:
        layer[slots - 1] = [0, 1]
    return F.write_hnsw_index([layer], docs, x.shape[1])


def _ivf_cases(out, tag, loader, files, args, ikey, vkey, off=0, voff=0):
    """mutations of one IVF blob + its vector file at (off, voff) inside files[ikey] / files[vkey], for the loader that opens them: alone
    (mdb_ivf_load), as the posting lists of a SPANN pair, or as one user's blob inside a collection's shared files"""
    index, vectors = files[ikey], files[vkey]
    lay = ivf_layout(index, off)
    nv, nc, nf = lay["num_vectors"], lay["num_clusters"], lay["num_features"]
    assert struct.unpack_from("<Q", vectors, voff)[0] == nv
    standalone = loader == "ivf"                                  # the loader takes offsets, a descriptor of its own and a shard
    whole = off == 0 and voff == 0 and lay["lists"][-1] + 32 == len(index)   # the blob is the file: cuts and insertions are its own
    pq_codes = args["quant"]["kind"] == 1

    def add(name, status, aim, index=None, vectors=None, args_=None):
        f = dict(files)
        if index is not None:
            f[ikey] = index
        if vectors is not None:
            f[vkey] = vectors
        out.append(Case("%s.%s" % (tag, name), loader, f, dict(args, **(args_ or {})), status, aim))
    for c in [] if not whole else _cuts(len(index), [45, 48, lay["centroids"], lay["meta"], lay["pl_meta"], lay["pl_start"]] + lay["lists"][1:] + [len(index)]):
        add("index_cut_%d" % c, FORMAT, "IVF index: header out of bounds" if c < 45 else "", index=index[:c])
    for c in [] if not whole else _cuts(len(vectors), [8, len(vectors)]):
        add("vectors_cut_%d" % c, FORMAT, "vector file: header out of bounds" if c < 8 else "exceed the file", vectors=vectors[:c])
    for name, elem in (("num_clusters", 1), ("num_vectors", 1), ("doc_id_mapping_len", 16), ("centroids_len", 4)):
        for vn, v in _field_values(lay[name], elem):
            add("%s_%s" % (name, vn), FORMAT, "", index=put(index, IVF_FIELDS, name, v, off))
    for vn, v in _field_values(lay["num_posting_lists"], 1):
        add("num_posting_lists_%s" % vn, FORMAT, "", index=poke(index, lay["meta"], "<Q", v & U64))
    # benign: the header's posting_lists_and_metadata_len is parsed and never consulted, here as in the reference
    # (rs/index/src/ivf/block_based/storage.rs:121: the field is read into the header; the list table is located from the two
    # section lengths before it, :72-80)
    add("ok_posting_lists_and_metadata_len_ignored", OK, "", index=put(index, IVF_FIELDS, "posting_lists_and_metadata_len", 1 << 63, off))
    add("version_1", FORMAT, "Unknown version", index=poke(index, off, "<B", 1))
    add("num_features_0", FORMAT, "", index=put(index, IVF_FIELDS, "num_features", 0, off))
    add("quantized_dimension_0", FORMAT, "", index=put(index, IVF_FIELDS, "quantized_dimension", 0, off))
    add("num_features_plus1", FORMAT, "", index=put(index, IVF_FIELDS, "num_features", nf + 1, off))
    add("quantized_dimension_plus1", FORMAT, "", index=put(index, IVF_FIELDS, "quantized_dimension", lay["quantized_dimension"] + 1, off))
    # the header's count against the vector file's: refused, see ivf_plan_files (rs/index/src/ivf/block_based/storage.rs:161, :195
    # bound doc ids by the header's count, vector/async_storage.rs:83-87 the rows by the file's; nothing compares them)
    if whole:
        one_more = put(index, IVF_FIELDS, "num_vectors", nv + 1)
        one_more = put(one_more[:lay["centroids"]] + b"\0" * 16 + one_more[lay["centroids"]:], IVF_FIELDS, "doc_id_mapping_len",
                       lay["doc_id_mapping_len"] + 16)
        add("header_counts_one_more_vector", FORMAT, "vectors, the vector file", index=one_more)
    add("header_counts_one_fewer_vector", FORMAT, "vectors, the vector file", index=put(index, IVF_FIELDS, "num_vectors", nv - 1, off))
    add("vector_file_counts_one_fewer", FORMAT, "vectors, the vector file", vectors=poke(vectors, voff, "<Q", nv - 1))
    add("doc_ids_too_short_for_num_vectors", FORMAT, "doc-id section of",
        index=put(index, IVF_FIELDS, "num_vectors", nv + 5, off))
    add("centroids_too_short_for_num_clusters", FORMAT, "centroid section of",
        index=put(index, IVF_FIELDS, "num_clusters", nc + 2, off))
    # a centroid section that ends 4 bytes before the file's last 8: the list count behind the alignment does not fit
    if whole:
        add("metadata_count_past_file", FORMAT, "metadata out of bounds",
            index=put(index[:lay["meta"] + 12], IVF_FIELDS, "centroids_len", lay["meta"] + 4 - lay["centroids"]))
    add("clusters_differ_from_posting_lists", FORMAT, "Mismatch between number of clusters",
        index=put(index, IVF_FIELDS, "num_clusters", nc - 1, off))
    # (inside a collection the next user's rows follow: one more row is in the file, and the two counts differ)
    add("vectors_count_plus1", FORMAT, "exceed the file" if whole else "vectors, the vector file", vectors=poke(vectors, voff, "<Q", nv + 1))
    add("vectors_count_2p61", FORMAT, "exceed the file", vectors=poke(vectors, voff, "<Q", 1 << 61))
    if whole:
        add("vectors_one_byte_short", FORMAT, "exceed the file", vectors=vectors[:-1])
    if standalone:
        add("vectors_offset_max", FORMAT, "vector file: header out of bounds", args_=dict(vectors_offset=U64))
        add("index_offset_max", FORMAT, "IVF index: header out of bounds", args_=dict(index_offset=U64 - 20))
        add("shard_rank_past_world", INVALID_ARG, "shard_rank", args_=dict(shard_rank=2, shard_world=2))
    if standalone and not pq_codes:
        add("vectors_offset_unaligned", FORMAT, "not 4-byte aligned", vectors=b"\0" + vectors, args_=dict(vectors_offset=1))
        add("descriptor_dimension_differs", FORMAT, "quantizer dimension != num_features", args_=dict(quant=noq(DIM + 4)))
        add("quantized_differs_from_features", FORMAT, "NoQuantizer",
            index=put(index, IVF_FIELDS, "quantized_dimension", nf // 2), args_=dict(quant=noq(0)))
    elif standalone:
        cb = args["quant"]["codebook"]
        add("descriptor_subvectors_differ", FORMAT, "dimension / subvector_dimension", args_=dict(quant=pq(cb, subvector_dimension=4)))
        add("descriptor_dimension_differs", FORMAT, "PQ dimension != num_features",
            args_=dict(quant=pq(np.concatenate([cb, cb]), dimension=2 * DIM, subvector_dimension=2 * SUBDIM)))
        add("descriptor_num_bits_9", UNSUPPORTED, "num_bits must be 1..8", args_=dict(quant=pq(cb, num_bits=9)))
        add("descriptor_codebook_short", FORMAT, "codebook too short", args_=dict(quant=pq(cb[:-1])))
    # posting-list metadata: an offset past the file, one that wraps, one that is not 8-byte aligned
    m1 = lay["pl_meta"] + 16 + 8
    add("list_offset_past_file", FORMAT, "posting list 1 out of bounds", index=poke(index, m1, "<Q", len(index) - lay["pl_start"] + 8))
    add("list_offset_max", FORMAT, "posting list 1 out of bounds", index=poke(index, m1, "<Q", U64))
    add("list_offset_unaligned", FORMAT, "is not 8-byte aligned", index=poke(index, m1, "<Q", struct.unpack_from("<Q", index, m1)[0] + 4))
    if standalone:   # the size-balanced ownership pass reads the same metadata first (one index, world > 1)
        add("list_offset_max_sharded", FORMAT, "posting list 1 out of bounds", index=poke(index, m1, "<Q", U64),
            args_=dict(shard_rank=1, shard_world=2))
    # list headers: the cases of test_corrupt_posting_list_headers_are_refused (tests/test_gpu_boundary.py), on the first list
    pl0 = lay["lists"][0]
    n0, L0, lw0, uw0 = struct.unpack_from("<QQQQ", index, pl0)
    assert n0 > 0
    for vn, field, v, aim in (("L_64", 8, 64, "lower_bit_length"), ("L_77", 8, 77, "lower_bit_length"), ("L_200", 8, 200, "lower_bit_length"),
                              ("lower_words_2p60", 16, 1 << 60, "truncated"), ("lower_words_2p61", 16, 1 << 61, "truncated"),
                              ("upper_words_0", 24, 0, "upper stream shorter"), ("upper_words_2p62", 24, 1 << 62, "truncated"),
                              ("num_elem_2p33", 0, 1 << 33, "num_elem exceeds"), ("num_elem_2p40", 0, 1 << 40, "num_elem exceeds"),
                              ("num_elem_nv_plus1", 0, nv + 1, "num_elem exceeds")):
        add("list_header_%s" % vn, FORMAT, aim, index=poke(index, pl0 + field, "<Q", v))
    if L0 and lw0:
        add("list_header_lower_words_0", FORMAT, "lower_words <", index=poke(index, pl0 + 16, "<Q", 0))
    if whole:   # the empty list closes the file: its 32-byte header cut short (ef_header_error's own length test)
        add("list_header_cut", FORMAT, "Not enough metadata", index=index[:lay["lists"][-1] + 16])
    # benign: garbage in the alignment padding runs
    pad = bytearray(index)
    for a, b in ((off + 45, off + 48), (lay["doc_ids"] + lay["doc_id_mapping_len"], lay["centroids"]),
                 (lay["centroids"] + lay["centroids_len"], lay["meta"])):
        pad[a:b] = b"\xa5" * (b - a)
    add("ok_padding_garbage", OK, "", index=bytes(pad))


def cases():
    """the whole table, built once: a list of Case"""
    if _CASES:
        return _CASES
    B = base()
    out = []
    # ------------------------------------------------------------------ HNSW (f32 and PQ)
    for tag in ("hnsw", "hnsw_pq"):
        loader, files, args = B[tag]
        cs, lay, nv = _hnsw_cases(tag, (loader, files, args, "index", "vectors", 0, 0))
        out += cs
        index, vectors = files["index"], files["vectors"]
        row = DIM * 4 if tag == "hnsw" else M

        def add(name, status, aim, tag=tag, loader=loader, files=files, args=args, **changed):
            a = changed.pop("args_", None)
            out.append(Case("%s.%s" % (tag, name), loader, _with(files, **changed), dict(args, **(a or {})), status, aim))
        # doc-id section: one id short, and empty (the remap kernels read id p of every p < num_vectors)
        ids = index[lay["doc_ids"]:]
        add("doc_ids_one_short", FORMAT, "doc-id section holds", index=put(index[:len(index) - 16], HNSW_FIELDS, "doc_id_mapping_len", len(ids) - 16))
        add("doc_ids_empty", FORMAT, "doc-id section holds", index=put(index[:lay["doc_ids"]], HNSW_FIELDS, "doc_id_mapping_len", 0))
        # vector file: count + 1, 2^61, one byte short, (f32) an offset that is not 4-byte aligned
        add("vectors_count_plus1", FORMAT, "vector file truncated", vectors=poke(vectors, 0, "<Q", nv + 1))
        add("vectors_count_2p61", FORMAT, "vector file truncated", vectors=poke(vectors, 0, "<Q", 1 << 61))
        add("vectors_count_max", FORMAT, "vector file truncated", vectors=poke(vectors, 0, "<Q", U64))
        add("vectors_one_byte_short", FORMAT, "vector file truncated", vectors=vectors[:-1])
        add("vectors_offset_past_file", FORMAT, "vector file: header out of bounds", args_=dict(vectors_offset=len(vectors) - 7))
        add("vectors_offset_max", FORMAT, "vector file: header out of bounds", args_=dict(vectors_offset=U64))
        add("index_offset_past_file", FORMAT, "header out of bounds", args_=dict(index_offset=len(index) - 8))
        add("index_offset_max", FORMAT, "header out of bounds", args_=dict(index_offset=U64 - 3))
        if tag == "hnsw":
            add("vectors_offset_unaligned", FORMAT, "not 4-byte aligned", vectors=b"\0" + vectors, args_=dict(vectors_offset=1))
            add("descriptor_dimension_differs", FORMAT, "quantized_dimension", args_=dict(quant=noq(DIM + 4)))
            add("no_dimension_anywhere", FORMAT, "no dimension", index=put(index, HNSW_FIELDS, "quantized_dimension", 0),
                args_=dict(quant=None))
        else:
            cb = args["quant"]["codebook"]
            add("descriptor_subvectors_differ", FORMAT, "quantized_dimension", args_=dict(quant=pq(cb, subvector_dimension=4)))
            add("descriptor_num_bits_9", UNSUPPORTED, "num_bits must be 1..8", args_=dict(quant=pq(cb, num_bits=9)))
            add("descriptor_num_bits_0", UNSUPPORTED, "num_bits must be 1..8", args_=dict(quant=pq(cb, num_bits=0)))
            add("descriptor_codebook_short", FORMAT, "codebook too short", args_=dict(quant=pq(cb[:-1])))
            add("descriptor_dimension_not_divisible", INVALID_ARG, "divisible", args_=dict(quant=pq(cb, dimension=DIM + 1)))
        # benign: garbage in every alignment padding run
        pad = bytearray(index)
        for a, b in ((49, lay["edges"]), (lay["points"] + lay["points_len"], lay["edge_offsets"]),
                     (lay["level_offsets"] + lay["level_offsets_len"], lay["doc_ids"])):
            pad[a:b] = b"\xa5" * (b - a)
        assert bytes(pad) != index, "the base graph has no padding run"
        add("ok_padding_garbage", OK, "", index=bytes(pad))
        # The entry point taken from a point no layer lists: points_len grown over the 4 bytes of padding behind it (absorbed, see
        # _absorbed), those bytes an id past the vectors, and level_offsets[0] on that element.  With the top layer's range empty
        # and decreasing the per-layer id check never sees the element, and the compact upper layers indexed a host array with it.
        pe = lay["points"] + lay["points_len"]
        if lay["edge_offsets"] - pe >= 4 and lay["num_layers"] >= 3:
            n_pts = lay["points_len"] // 4
            stray = poke(put(index, HNSW_FIELDS, "points_len", lay["points_len"] + 4), pe, "<I", nv + 7)
            add("entry_point_from_padding_decreasing", FORMAT, "", index=poke(stray, lay["level_offsets"], "<Q", n_pts))
            flat = stray
            for i in range(lay["num_layers"]):
                flat = poke(flat, lay["level_offsets"] + 8 * i, "<Q", n_pts)
            add("entry_point_from_padding_no_upper_points", FORMAT, "", index=flat)
        # benign: an upper-layer point listed twice — the loader keeps the first, as find_point_in_range does (graph_storage.rs:423-449)
        first1 = lay["levels"][lay["num_layers"] - 2]
        twice = poke(index, lay["points"] + 4 * (first1 + 1), "<I", struct.unpack_from("<I", index, lay["points"] + 4 * first1)[0])
        add("ok_upper_point_twice", OK, "", index=twice)
        # ... and the second, never-read occurrence with an edge out of range is still refused (its edges are walked at load)
        a1 = struct.unpack_from("<Q", twice, lay["edge_offsets"] + 8 * (first1 + 1))[0]
        add("upper_point_twice_bad_edge", FORMAT, "upper-layer edge", index=poke(twice, lay["edges"] + 4 * a1, "<I", nv + 5))
    # ------------------------------------------------------------------ HNSW: degenerate graphs written whole
    rng = np.random.default_rng(30)
    x = rng.standard_normal((40, DIM)).astype(np.float32)
    docs40, vec40 = list(range(500, 540)), F.write_vector_file(x)

    def hn(name, status, aim, index, vectors=vec40, quant=noq()):
        out.append(Case("hnsw." + name, "hnsw", dict(index=index, vectors=vectors), dict(quant=quant), status, aim))
    hn("ok_num_layers_0_empty", OK, "", F.write_hnsw_index([], docs40, DIM))
    hn("ok_zero_vectors", OK, "", F.write_hnsw_index([], [], DIM), F.write_vector_file(np.zeros((0, DIM), np.float32)))
    # slot counts: the rows of layer 0 are clamped to the vector file's count, and a point without a row has no neighbours (the
    # reference never reads a slot no edge leads to, and reads past the sentinel for a point beyond the slots: graph_storage.rs:486-503)
    hn("ok_more_layer0_slots_than_vectors", OK, "", _single_layer_graph(x, 44, docs40))
    hn("ok_fewer_layer0_slots_than_vectors", OK, "", _single_layer_graph(x[:36], 36, docs40))
    # one layer, the first slot with an edge lies past the vector file: that slot is the entry point (graph_storage.rs:528-546)
    hn("entry_slot_past_vectors", FORMAT, "entry point", _single_layer_graph(x, 44, docs40, edges_from=40))
    wide = {p: [] for p in range(300)}
    wide[0] = list(range(1, 258))
    y = rng.standard_normal((300, DIM)).astype(np.float32)
    hn("degree_257", UNSUPPORTED, "node degree 257 exceeds 256", F.write_hnsw_index([wide], list(range(300)), DIM), F.write_vector_file(y))
    up = _graph_layers(y, (3,), 4, 2, 31)
    top = list(up[1])
    up[1][top[0]] = [top[1]] * 257
    hn("degree_257_upper", UNSUPPORTED, "node degree 257 exceeds 256", F.write_hnsw_index(up, list(range(300)), DIM), F.write_vector_file(y))
    # ------------------------------------------------------------------ IVF (f32 and PQ)
    for tag in ("ivf", "ivf_pq"):
        loader, files, args = B[tag]
        _ivf_cases(out, tag, loader, files, args, "index", "vectors")
    z = np.zeros((0, DIM), np.float32)
    out.append(Case("ivf.ok_zero_vectors", "ivf", dict(index=F.write_ivf_index(np.ones((2, DIM), np.float32), [], [np.zeros(0, np.uint64)] * 2),
                                                       vectors=F.write_vector_file(z)), dict(quant=noq()), OK, ""))
    # ------------------------------------------------------------------ SPANN pair
    for tag in ("spann", "spann_pq"):
        loader, files, args = B[tag]

        def add(name, status, aim, tag=tag, loader=loader, files=files, args=args, **changed):
            out.append(Case("%s.%s" % (tag, name), loader, _with(files, **changed), dict(args), status, aim))
        hi, hv = files["hnsw_index"], files["hnsw_vectors"]
        add("ok", OK, "")
        # a centroid graph whose dimension differs from the IVF's num_features (the graph half is refused after the IVF half passed)
        add("graph_dimension_differs", FORMAT, "HNSW quantized_dimension", hnsw_index=put(hi, HNSW_FIELDS, "quantized_dimension", DIM // 2))
        add("graph_edge_out_of_range", FORMAT, "outside the vector storage", hnsw_index=poke(hi, hnsw_layout(hi)["edges"], "<I", 7))
        add("graph_vectors_cut", FORMAT, "vector file truncated", hnsw_vectors=hv[:-4])
        add("ivf_version_1", FORMAT, "Unknown version", ivf_index=poke(files["ivf_index"], 0, "<B", 9))
        add("ivf_vectors_cut", FORMAT, "exceed the file", ivf_vectors=files["ivf_vectors"][:-1])
        # every mutation of a graph file and of an IVF file again on the pair's own four files: truncations at every section boundary,
        # every length and count field, offset tables, points, edges, list metadata and headers
        cs, _, _ = _hnsw_cases(tag + ".graph", (loader, files, args, "hnsw_index", "hnsw_vectors", 0, 0))
        out += cs
        _ivf_cases(out, tag + ".lists", loader, files, args, "ivf_index", "ivf_vectors")
    # ------------------------------------------------------------------ multi-user collection
    loader, files, args = B["multi"]
    table = files["user_table"]
    recs = [F.unpack_user_index_info(table[i:i + 112]) for i in range(0, len(table), 112)]

    def repack(rs):
        return b"".join(F.pack_user_index_info(r["user_id"], **{k: r[k] for k in F.USER_INDEX_INFO_FIELDS}) for r in rs)

    def madd(name, status, aim, args_=None, **changed):
        out.append(Case("multi.%s" % name, loader, _with(files, **changed), dict(args, **(args_ or {})), status, aim))
    madd("ok", OK, "")
    for field, fkey in (("centroid_index_offset", "hnsw_index"), ("centroid_vector_offset", "hnsw_vectors"),
                        ("ivf_index_offset", "ivf_index"), ("ivf_vectors_offset", "ivf_vectors")):
        for vn, v in (("past_file", len(files[fkey])), ("max", U64)):
            rs = [dict(r) for r in recs]
            rs[1][field] = v
            madd("%s_%s" % (field, vn), FORMAT, "header out of bounds", user_table=repack(rs))
    # one corrupt user among valid ones: the load is refused as a whole — the LAST user's graph (every earlier blob has passed)
    last = recs[-1]
    lay = hnsw_layout(files["hnsw_index"], last["centroid_index_offset"])
    madd("last_user_graph_edge_out_of_range", FORMAT, "outside the vector storage",
         hnsw_index=poke(files["hnsw_index"], lay["edges"], "<I", 1 << 20))
    madd("last_user_ivf_version", FORMAT, "Unknown version", ivf_index=poke(files["ivf_index"], last["ivf_index_offset"], "<B", 3))
    mid = recs[1]
    madd("users_disagree_on_num_features", FORMAT, "users disagree",
         ivf_index=put(put(files["ivf_index"], IVF_FIELDS, "num_features", DIM // 2, mid["ivf_index_offset"]), IVF_FIELDS,
                       "quantized_dimension", DIM // 2, mid["ivf_index_offset"]))
    madd("num_features_argument_differs", FORMAT, "!= index header", args_=dict(num_features=DIM + 1, quant=noq(0)))
    madd("no_users", INVALID_ARG, "no users", user_table=b"")
    # The `*_len` fields of a user record are not consulted — the reference passes only the four offsets to the reader
    # (rs/index/src/multi_spann/index.rs:110-116) — so a record with every length zeroed, or absurd, opens the same index
    for vn, v in (("zero", 0), ("max", U64)):
        rs = [dict(r, **{k: v for k in F.USER_INDEX_INFO_FIELDS if k.endswith("_len")}) for r in recs]
        madd("ok_record_lengths_%s_ignored" % vn, OK, "", user_table=repack(rs))
    # every per-graph mutation again on the middle user's graph, inside the shared files
    cs, _, _ = _hnsw_cases("multi.user1_graph", (loader, files, args, "hnsw_index", "hnsw_vectors", mid["centroid_index_offset"],
                                                        mid["centroid_vector_offset"]))
    out += [c for c in cs if "quantized_dimension" not in c.name or c.name.endswith("_0")]
    # ... and every per-blob IVF mutation on the middle user's posting lists, at a non-zero offset in both shared files
    _ivf_cases(out, "multi.user1_lists", loader, files, args, "ivf_index", "ivf_vectors", mid["ivf_index_offset"], mid["ivf_vectors_offset"])
    # truncations of the four shared files: at every user's blob (one byte before it — inside the padding between two users —, at it
    # and one byte in), at every section boundary of the LAST user's graph and lists, and one byte before the end.  Whatever is cut
    # belongs to some user's blob, and one refused user refuses the load.
    hl = hnsw_layout(files["hnsw_index"], last["centroid_index_offset"])
    il = ivf_layout(files["ivf_index"], last["ivf_index_offset"])
    bounds = dict(hnsw_index=[r["centroid_index_offset"] for r in recs] + [hl[k] for k in ("edges", "points", "edge_offsets", "level_offsets", "doc_ids")],
                  hnsw_vectors=[r["centroid_vector_offset"] for r in recs] + [last["centroid_vector_offset"] + 8],
                  ivf_index=[r["ivf_index_offset"] for r in recs] + [il[k] for k in ("doc_ids", "centroids", "meta", "pl_meta", "pl_start")] + il["lists"][1:],
                  ivf_vectors=[r["ivf_vectors_offset"] for r in recs] + [last["ivf_vectors_offset"] + 8])
    for fkey, bs in bounds.items():
        for c in _cuts(len(files[fkey]), bs + [len(files[fkey])]):
            madd("%s_cut_%d" % (fkey, c), FORMAT, "", **{fkey: files[fkey][:c]})
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    _CASES.extend(out)
    return _CASES


_CASES = []


# ----------------------------------------------------------------------------------- running a case through the checkers (ctypes)
def quant_desc(q):
    """(QuantDesc or None, keepalive)"""
    from muopdb_amd import lib as L
    if q is None:
        return None, None
    d = L.QuantDesc()
    d.kind, d.metric, d.dimension, d.subvector_dimension, d.num_bits = q["kind"], q["metric"], q["dimension"], q["subvector_dimension"], q["num_bits"]
    cb = np.ascontiguousarray(q["codebook"], np.float32) if q["codebook"] is not None else np.zeros(1, np.float32)
    d.codebook = L.ptr(cb, C.c_float)
    d.codebook_len = cb.size if q["codebook"] is not None else 0
    return d, cb


def user_records(table):
    from muopdb_amd import lib as L
    n = len(table) // 112
    arr = (L.UserIndexInfoC * max(n, 1))()
    C.memmove(arr, table, n * 112)
    return arr, n


def file_args(case, keys):
    """(pointer, length) pairs of the case's files: every file in a buffer of exactly its length"""
    bufs = [C.create_string_buffer(case.files[k], max(len(case.files[k]), 1)) for k in keys]
    flat = []
    for k, b in zip(keys, bufs):
        flat.append((C.cast(b, C.c_void_p), C.c_size_t(len(case.files[k]))))
    return flat, bufs


def check(case):
    """(status, message) of the case through its host-only checker"""
    from muopdb_amd import lib as L
    lib = L.load()
    a = case.args
    q, keep = quant_desc(a.get("quant"))
    qp = C.byref(q) if q is not None else None
    why = C.create_string_buffer(600)
    sz = C.c_size_t
    if case.loader in ("hnsw", "ivf"):
        bufs = file_args(case, ("index", "vectors"))
        (ip, il), (vp, vl) = bufs[0]
        common = (ip, il, sz(a.get("index_offset", 0)), vp, vl, sz(a.get("vectors_offset", 0)), qp)
        if case.loader == "hnsw":
            st = lib.mdb_hnsw_check_files(*common, why, sz(600))
        else:
            st = lib.mdb_ivf_check_files(*common, C.c_uint32(a.get("shard_rank", 0)), C.c_uint32(a.get("shard_world", 1)), why, sz(600))
    else:
        bufs = file_args(case, ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors"))
        (hp, hl), (hvp, hvl), (ip, il), (vp, vl) = bufs[0]
        if case.loader == "spann":
            st = lib.mdb_spann_check_files(hp, hl, sz(0), hvp, hvl, sz(0), ip, il, sz(0), vp, vl, sz(0), qp, why, sz(600))
        else:
            users, n = user_records(case.files["user_table"])
            st = lib.mdb_multi_spann_check_files(users, sz(n), C.c_uint32(a["num_features"]), hp, hl, hvp, hvl, ip, il, vp, vl, qp,
                                                 C.c_uint32(a.get("shard_rank", 0)), C.c_uint32(a.get("shard_world", 1)), why, sz(600))
    del bufs, keep
    return int(st), why.value.decode()


# ----------------------------------------------------------------------------------- the bundle tests/host/check_files_main.cpp reads
LOADER_IDS = dict(hnsw=0, ivf=1, spann=2, multi=3)
BLOB_KEYS = ("index", "vectors", "hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors", "user_table")


def write_bundle(path, table):
    """u32 count; per case: u32 name length, name, u32 loader, 16 x u64 arguments { index_offset, vectors_offset, has_quant, kind, metric,
    dimension, subvector_dimension, num_bits, has_codebook, num_features, shard_rank, shard_world }, then 8 blobs { u64 length, bytes }:
    the seven files of BLOB_KEYS (absent: length 0) and the codebook (f32)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(table)))
        for c in table:
            a, q = c.args, c.args.get("quant")
            name = c.name.encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<I", LOADER_IDS[c.loader]))
            cb = b"" if q is None or q["codebook"] is None else np.ascontiguousarray(q["codebook"], np.float32).tobytes()
            words = [a.get("index_offset", 0), a.get("vectors_offset", 0), int(q is not None)] + \
                    ([q["kind"], q["metric"], q["dimension"], q["subvector_dimension"], q["num_bits"], int(q["codebook"] is not None)]
                     if q is not None else [0] * 6) + [a.get("num_features", 0), a.get("shard_rank", 0), a.get("shard_world", 1)]
            f.write(struct.pack("<16Q", *(words + [0] * (16 - len(words)))))
            for k in BLOB_KEYS:
                b = c.files.get(k, b"")
                f.write(struct.pack("<Q", len(b)) + b)
            f.write(struct.pack("<Q", len(cb)) + cb)

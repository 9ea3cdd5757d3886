"""Pins the CPU oracle (oracle/) and the format producers (muopdb_amd/formats.py) against the
reference's own known-answer tests — SURVEY.md §8c K1..K13 — re-encoded here as data.
Each test names the reference test (file:line) it restates.  CPU only.
"""
import struct

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H


# ----------------------------------------------------------------------------- K1/K2/K3/K4: Elias-Fano
def test_k1_ef_bits(oracle):
    # rs/compression/src/elias_fano/ef.rs:230-259 test_elias_fano_encoding
    L, lower, upper = F.ef_bits([5, 8, 8, 15, 32], 36)
    assert L == 2
    assert lower == [1, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert upper == [0, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1]
    blob, L2, lb, ub = oracle.ef_encode([5, 8, 8, 15, 32], 36)
    assert (L2, lb, ub) == (2, 10, 13)
    assert blob == F.ef_encode([5, 8, 8, 15, 32], 36)
    # unsorted / exceeding the universe are errors (ef.rs:251-258)
    with pytest.raises(ValueError):
        oracle.ef_encode([5, 8, 7, 15, 32], 36)
    with pytest.raises(ValueError):
        oracle.ef_encode([5, 8, 8, 15, 32], 31)
    with pytest.raises(ValueError):
        F.ef_encode([5, 8, 7, 15, 32], 36)


def test_k2_ef_file_layout(oracle):
    # ef.rs:329-373 test_elias_fano_write: header words then lower then upper, all LE u64
    blob = F.ef_encode([5, 8, 8, 15, 32], 36)
    n, L, lw, uw = struct.unpack_from("<QQQQ", blob, 0)
    assert (n, L, lw, uw) == (5, 2, 1, 1)
    assert len(blob) == (4 + lw + uw) * 8


def test_k3_ivf_posting_list_bytes(oracle):
    # rs/index/src/ivf/writer.rs:678-762 test_write_posting_lists_and_metadata
    meta, pls = F.write_posting_lists_and_metadata([np.array([5, 8, 8, 15, 32], np.uint64)])
    assert meta == bytes([1, 0, 0, 0, 0, 0, 0, 0, 48, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    expected = bytes([
        5, 0, 0, 0, 0, 0, 0, 0,
        2, 0, 0, 0, 0, 0, 0, 0,
        1, 0, 0, 0, 0, 0, 0, 0,
        1, 0, 0, 0, 0, 0, 0, 0,
        0b11000001, 0, 0, 0, 0, 0, 0, 0,
        0b01011010, 0b00010000, 0, 0, 0, 0, 0, 0])
    assert pls == expected
    assert oracle.ef_encode([5, 8, 8, 15, 32], 32)[0] == expected


@pytest.mark.parametrize("values,universe", [
    ([5, 8, 8, 15, 32], 36), ([0, 1, 2, 3, 4], 5), ([10], 20), ([1000, 2000, 3000, 4000, 5000], 6000),
    ([2, 4, 6, 8, 10], 10), ([1, 5, 10, 15, 20, 25, 30], 100), (list(range(1, 201)), 500),
    (list(range(1, 101)), 9999), ([42], 100), ([10, 20, 30, 40, 50], 100)])
def test_k4_ef_decode_sequences(oracle, values, universe):
    # block_based_decoder.rs:346-590 + ef.rs:294-327 decoding cases
    blob = F.ef_encode(values, universe)
    assert oracle.ef_decode(blob).tolist() == values
    assert oracle.ef_encode(values, universe)[0] == blob


def test_ef_empty_and_random(oracle):
    assert oracle.ef_decode(F.ef_encode([])).tolist() == []
    assert len(F.ef_encode([])) == 32
    rng = np.random.default_rng(3)
    for _ in range(100):
        n = int(rng.integers(1, 400))
        v = np.sort(rng.integers(0, 1 << int(rng.integers(1, 33)), n)).astype(np.uint64)
        blob = F.ef_encode(v)
        assert blob == oracle.ef_encode(v, int(v[-1]))[0]
        assert np.array_equal(oracle.ef_decode(blob), v)


# ----------------------------------------------------------------------------- K5/K6: PQ quantize
def test_k5_pq_quantize_and_vector_files(oracle):
    # ivf/writer.rs:511-676 test_quantize_and_write_vectors
    pq = oracle.ProductQuantizer(3, 1, 1, [1.5, 4.5, 2.3, 5.3, 3.1, 6.1])
    raw = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], np.float32)
    codes = pq.quantize(raw)
    assert codes.tolist() == [[0, 0, 0], [1, 1, 1]]
    vf = F.write_vector_file(codes)
    assert len(vf) == 14 and vf[:8] == struct.pack("<Q", 2) and vf[8:] == bytes([0, 0, 0, 1, 1, 1])
    rf = F.write_vector_file(raw)
    assert rf[:8] == struct.pack("<Q", 2)
    assert np.frombuffer(rf[8:], "<f4").tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]


def test_k6_pq_quantize(oracle):
    # rs/quantization/src/pq/mod.rs:321-371: codebook cb[s][i] = (2s+i, 2s+i), d=10, subdim 2, 1 bit
    cb = []
    for s in range(5):
        for i in range(2):
            cb += [2 * s + i, 2 * s + i]
    pq = oracle.ProductQuantizer(10, 2, 1, cb)
    assert pq.quantize([1, 1, 3, 3, 5, 5, 7, 7, 9, 9]).tolist() == [[1, 1, 1, 1, 1]]
    assert pq.original_vector([1, 1, 1, 1, 1]).tolist() == [1, 1, 3, 3, 5, 5, 7, 7, 9, 9]
    cfg = F.parse_simple_yaml(F.product_quantizer_config_yaml(10, 2, 1))
    assert cfg == {"dimension": 10, "subvector_dimension": 2, "num_bits": 1}
    with pytest.raises(ValueError):
        oracle.ProductQuantizer(10, 3, 1, cb)


def test_pq_impls_agree(oracle):
    # rs/quantization/src/pq/pq_builder.rs:150-188: Scalar / SIMD / StreamingSIMD within 1e-5
    rng = np.random.default_rng(5)
    for d, sub, bits in [(128, 8, 8), (128, 4, 4), (256, 16, 8), (128, 32, 4), (64, 8, 1)]:
        m, K = d // sub, 1 << bits
        pq = oracle.ProductQuantizer(d, sub, bits, rng.random(m * K * sub, dtype=np.float32))
        a = rng.integers(0, K, (50, m)).astype(np.uint8)
        b = rng.integers(0, K, (50, m)).astype(np.uint8)
        ds = pq.distance(a, b, oracle.PQ_SCALAR)
        dv = pq.distance(a, b, oracle.PQ_SIMD)
        dst = pq.distance(a, b, oracle.PQ_STREAMING)
        assert np.allclose(ds, dst, rtol=1e-5, atol=1e-5) and np.allclose(dv, dst, rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------- distances (property pins)
@pytest.mark.parametrize("d", [128, 30, 16, 3, 1, 17, 9, 5, 768, 100])
def test_distance_simd_vs_scalar(oracle, d):
    # rs/utils/src/distance/l2.rs:108-130, dot_product.rs:106-124, lane_conforming.rs:36-57
    rng = np.random.default_rng(d)
    a, b = rng.random(d, dtype=np.float32), rng.random(d, dtype=np.float32)
    # the reference pins 1e-5 / 2e-5 absolute at d<=128; scale the tolerance for the larger dims added here
    scale = max(1.0, d / 128.0)
    assert abs(oracle.l2(a, b) - oracle.l2_scalar(a, b)) < 1e-5 * scale
    assert abs(oracle.dot(a, b) - oracle.dot_scalar(a, b)) < 2e-5 * scale * scale
    ref = float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum()))
    assert abs(oracle.l2(a, b) - ref) < 1e-4 * max(1.0, ref)
    assert abs(oracle.l2_squared(a, b) - ref * ref) < 1e-4 * max(1.0, ref * ref)


@pytest.mark.parametrize("lanes", [4, 8, 16])
def test_lane_conforming_matches_cascade(oracle, lanes):
    # lane_conforming.rs:36-57: LaneConforming<4, D>::calculate_squared vs D::calculate_squared on d=16, eps 1e-5;
    # also pinned structurally: with d == lanes the single pass IS the cascade's pass, so the bits agree
    rng = np.random.default_rng(lanes)
    a, b = rng.random(16, dtype=np.float32), rng.random(16, dtype=np.float32)
    assert abs(oracle.lane_conforming(0, lanes, a, b) - oracle.l2_squared(a, b)) < 1e-5
    assert abs(oracle.lane_conforming(1, lanes, a, b) - oracle.dot(a, b)) < 1e-5
    a, b = a[:lanes], b[:lanes]
    assert np.float32(oracle.lane_conforming(0, lanes, a, b)).tobytes() == np.float32(oracle.l2_squared(a, b)).tobytes()
    # independent numpy float32 restatement of accumulate_lanes + ordered reduce_sum
    a, b = rng.random(16 * 6, dtype=np.float32) * 50, rng.random(16 * 6, dtype=np.float32) * 50
    acc = np.zeros(lanes, np.float32)
    for c in range(0, a.size, lanes):
        df = a[c:c + lanes] - b[c:c + lanes]
        acc = acc + df * df
    r = np.float32(0)
    for v in acc:
        r = np.float32(r + v)
    assert np.float32(oracle.lane_conforming(0, lanes, a, b)).tobytes() == r.tobytes()


def test_distance_association_is_lanewise(oracle):
    # The cascade is lane-wise partial sums then an ordered horizontal sum (l2.rs:37-67, 77-89):
    # restate it independently in numpy float32 and require bit equality.
    rng = np.random.default_rng(11)
    for d in (16, 128, 100, 768, 31):
        a = (rng.random(d, dtype=np.float32) * 100).astype(np.float32)
        b = (rng.random(d, dtype=np.float32) * 100).astype(np.float32)
        ret = np.float32(0)
        pos = 0
        for lanes in (16, 8, 4):
            n = (d - pos) // lanes
            if n > 0:
                acc = np.zeros(lanes, np.float32)
                for c in range(n):
                    diff = a[pos + c * lanes: pos + (c + 1) * lanes] - b[pos + c * lanes: pos + (c + 1) * lanes]
                    acc = acc + diff * diff
                s = np.float32(0)
                for j in range(lanes):
                    s = np.float32(s + acc[j])
                ret = np.float32(ret + s)
                pos += n * lanes
        for i in range(pos, d):
            diff = np.float32(a[i] - b[i])
            ret = np.float32(ret + np.float32(diff * diff))
        assert np.float32(oracle.l2_squared(a, b)) == ret


# ----------------------------------------------------------------------------- K7: IVF container
def test_k7_ivf_index_file(oracle):
    # rs/index/src/posting_list/combined_file.rs:172-300 (hand-assembled file, plain u64 PLs there;
    # the block-based reader decodes EF, so the PLs here are EF-encoded — header/sections identical)
    header = bytes([0, 4, 0, 0, 0, 4, 0, 0, 0, 2, 0, 0, 0]) + struct.pack("<QQQQ", 4, 80, 40, 9)
    assert F.write_ivf_header(4, 4, 2, 4, 80, 40, 9) == header
    centroids = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    pls = [np.array([0, 1], np.uint64), np.array([2, 3], np.uint64)]
    index = F.write_ivf_index(centroids, [100, 200, 300, 400], pls)
    assert index[:45] == header[:37] + struct.pack("<Q", len(index) - 48 - 80 - 40)
    assert index[45:48] == b"\0\0\0"
    assert index[48:64] == struct.pack("<QQ", 4, 0)              # u128 count
    assert index[64:80] == struct.pack("<QQ", 100, 0)
    assert index[128:136] == struct.pack("<Q", 2)                 # centroid count
    vec = F.write_vector_file(np.zeros((4, 4), np.float32))
    ivf = oracle.BlockBasedIvf(index, vec)
    assert (ivf.num_features, ivf.quantized_dimension, ivf.num_clusters, ivf.num_vectors) == (4, 4, 2, 4)
    assert (ivf.doc_id_mapping_len, ivf.centroids_len) == (80, 40)
    assert [ivf.get_doc_id(i) for i in range(4)] == [100, 200, 300, 400]
    with pytest.raises(IndexError):
        ivf.get_doc_id(4)
    assert ivf.get_centroid(0).tolist() == [1, 2, 3, 4] and ivf.get_centroid(1).tolist() == [5, 6, 7, 8]
    with pytest.raises(IndexError):
        ivf.get_centroid(2)
    assert ivf.get_posting_list(0).tolist() == [0, 1] and ivf.get_posting_list(1).tolist() == [2, 3]
    with pytest.raises(IndexError):
        ivf.get_posting_list(2)
    # ivf/writer.rs:382-470 test_combine_files: padding rules (16 after header, 8 before metadata)
    c3 = np.arange(3, dtype=np.float32).reshape(1, 3)
    idx3 = F.write_ivf_index(c3, [7], [np.array([0], np.uint64)])
    doc_end = 48 + 32
    cent_end = doc_end + 8 + 12
    assert idx3[cent_end:cent_end + 4] == b"\0\0\0\0"             # pad to 8
    assert struct.unpack_from("<Q", idx3, cent_end + 4)[0] == 1  # num posting lists
    ivf3 = oracle.BlockBasedIvf(idx3, F.write_vector_file(np.zeros((1, 3), np.float32)))
    assert ivf3.get_posting_list(0).tolist() == [0]


def test_u128_doc_ids_roundtrip(oracle):
    big = [(1 << 100) + 5, (1 << 64), 3]
    index = F.write_ivf_index(np.zeros((1, 2), np.float32), big, [np.array([0, 1, 2], np.uint64)])
    ivf = oracle.BlockBasedIvf(index, F.write_vector_file(np.zeros((3, 2), np.float32)))
    assert [ivf.get_doc_id(i) for i in range(3)] == big


# ----------------------------------------------------------------------------- K12: ordering
def test_k12_ordering(oracle):
    # rs/index/src/utils.rs:183-297 (IdWithScore: score, then id, NaN last); traverse_state.rs:31-52
    scores = [1.0, float("nan"), 0.5, 1.0, float("nan")]
    ids = [7, 2, 9, 3, 1]
    perm = oracle.sort_id_with_score(scores, ids).tolist()
    assert [ids[i] for i in perm] == [9, 3, 7, 1, 2]
    assert oracle.heap_pop_order([0.0, -2.0, -1.0], [0, 2, 1]).tolist() == [0, 1, 2]
    # ties: max-heap on (distance, id) pops the larger id first
    assert oracle.heap_pop_order([1.0, 1.0, 1.0], [4, 9, 2]).tolist() == [9, 4, 2]


# ----------------------------------------------------------------------------- K13: HNSW container
def _k13_layers():
    l2 = {1: []}
    l1 = {1: [4, 5], 4: [1, 5], 5: [1, 4]}
    l0 = {1: [4, 5], 4: [1, 5], 5: [1, 4], 2: [1, 3], 3: [2, 4], 0: [1, 2]}
    return [l0, l1, l2]


def test_k13_hnsw_file(oracle):
    # rs/index/src/hnsw/writer.rs:269-618 construct_layers + test_write
    index = F.write_hnsw_index(_k13_layers(), [1, 2, 3, 4, 5, 6], 16)
    assert len(struct.pack("<BIIQQQQQ", 0, 0, 0, 0, 0, 0, 0, 0)) == 49 and index[0] == 0
    vec = F.write_vector_file(np.zeros((6, 16), np.float32))
    h = oracle.BlockBasedHnsw(index, vec, 16)
    assert h.num_layers == 3 and h.quantized_dimension == 16
    assert h.get_edges_for_point(1, 2) is None                    # no edges in the top layer
    assert sorted(h.get_edges_for_point(1, 1).tolist()) == [4, 5]
    assert sorted(h.get_edges_for_point(0, 0).tolist()) == [1, 2]
    assert h.get_edges_for_point(0, 1) is None                    # point 0 is not in layer 1
    assert h.get_edges_for_point(3, 0).tolist() == [2, 4]
    assert h.entry_point == 1
    # header lengths: edges 4B each, points for upper layers, edge_offsets incl. sentinel, level offsets nl+1
    assert h.edges_len == 4 * (0 + 6 + 12) and h.points_len == 4 * (1 + 3)
    assert h.edge_offsets_len == 8 * (1 + 3 + 6 + 1) and h.level_offsets_len == 8 * 4
    assert h.doc_id_mapping_len == 16 * 6
    # section alignment (hnsw/writer.rs:223-265): edges @4, edge_offsets @8, doc ids @16
    assert index[49:52] == b"\0\0\0"
    off_eo = 52 + h.edges_len + h.points_len
    off_eo += (8 - off_eo % 8) % 8
    lo = np.frombuffer(index, "<u8", 4, off_eo + h.edge_offsets_len)
    assert lo.tolist() == [0, 1, 4, 11]


def test_hnsw_single_layer_entry_point(oracle):
    # graph_storage.rs:527-546: single layer => first point with >= 1 edge
    index = F.write_hnsw_index([{0: [], 1: [2], 2: [1]}], [10, 11, 12], 4)
    h = oracle.BlockBasedHnsw(index, F.write_vector_file(np.zeros((3, 4), np.float32)), 4)
    assert h.entry_point == 1 and h.num_layers == 1


# ----------------------------------------------------------------------------- K8: SPANN end to end
def _line_vectors(n=1000):
    return np.repeat(np.arange(n, dtype=np.float32)[:, None], 4, 1)


def test_k8_spann_search(oracle):
    # rs/index/src/spann/index.rs:293-366 test_spann_search, :369-445 with invalidation
    v = _line_vectors()
    files, _, _ = H.build_spann_files(oracle, v, list(range(1000)), 10)
    sp = oracle.Spann(files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"])
    res = sp.search([2.4, 3.4, 4.4, 5.4], oracle.SearchParams(2, 2))
    assert res.counts[0] == 2 and res.doc_ids(0) == [4, 3]
    assert sp.invalidate(4) and sp.is_invalidated(4) and not sp.invalidate(4)
    res = sp.search([2.4, 3.4, 4.4, 5.4], oracle.SearchParams(2, 2))
    assert res.doc_ids(0) == [3, 5]


def test_k8_spann_search_pq(oracle):
    # spann/index.rs:448-527 test_spann_search_with_pq: subdim 2, 2 bits => all top-5 scores 0.0
    v = _line_vectors()
    cb = H.train_pq_codebook(v, 2, 2)
    pq = oracle.ProductQuantizer(4, 2, 2, cb)
    files, _, _ = H.build_spann_files(oracle, v, list(range(1000)), 10, quantize=pq.quantize)
    quant = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 2, 2, cb)
    sp = oracle.Spann(files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"], quant)
    res = sp.search([2.4, 3.4, 4.4, 5.4], oracle.SearchParams(5, 2))
    assert res.counts[0] == 5 and res.scores[0].tolist() == [0.0] * 5
    # equal scores are ordered by doc id (IdWithScore)
    assert res.doc_ids(0) == sorted(res.doc_ids(0))


# ----------------------------------------------------------------------------- K14: k-means (the reference's own tests)
_KM = [[0, 0], [40, 40], [90, 90], [1, 1], [41, 41], [91, 91], [2, 2], [42, 42], [92, 92]]


def test_k14_kmeans_lloyd(oracle):
    # rs/utils/src/kmeans_builder/kmeans_builder.rs:373-412 test_kmeans_lloyd: init points 0,1,2, tolerance 1e-4
    cent, a, err, it = oracle.kmeans_fit(np.array(_KM, np.float32), 3, 100, 1e-4, [0, 1, 2])
    assert cent.shape == (3, 2)
    assert a[0] == a[3] == a[6] and a[1] == a[4] == a[7] and a[2] == a[5] == a[8]
    assert cent.tolist() == [[1.0, 1.0], [41.0, 41.0], [91.0, 91.0]]


def test_k14_kmeans_no_distance_penalty(oracle):
    # :414-449 test_kmeans_no_distance_penalty: point 7 = (5, 5) joins the cluster of points 0, 3, 6 when tolerance = 0
    data = [r[:] for r in _KM]
    data[7] = [5, 5]
    cent, a, err, it = oracle.kmeans_fit(np.array(data, np.float32), 3, 100, 0.0, [0, 1, 2])
    assert a[0] == a[3] == a[6] == a[7] and a[1] == a[4] and a[2] == a[5] == a[8]


def test_k14_kmeans_with_empty_cluster(oracle):
    # :451-486 test_kmeans_with_empty_cluster: 10 clusters asked of 9 points -> 9 centroids, every cluster non-empty
    # (the reference's init is random there because 3 init values != 9 clusters; any init must give the same property)
    data = [r[:] for r in _KM]
    data[7] = [5, 5]
    for init in ([0, 1, 2, 3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3, 2, 1, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0]):
        cent, a, err, it = oracle.kmeans_fit(np.array(data, np.float32), 10, 100, 0.0, init)
        assert cent.shape == (9, 2) and set(a.tolist()) == set(range(9))


# ----------------------------------------------------------------------------- K11: HNSW builder reindex
def test_k11_hnsw_builder_reindex():
    # rs/index/src/hnsw/builder.rs:460-575 test_hnsw_builder_reindex: 3 points, one layer, entry points [0, 1]
    from muopdb_amd import hnsw_build as HB
    layer = {0: [(2, 1.0)], 1: [(2, 2.0)], 2: [(1, 2.0), (0, 1.0)]}
    codes = np.array([[0] * 5, [1] * 5, [2] * 5], np.uint8)
    layers, entry, docs, vec, assigned = HB.reindex([layer], [0, 1], [100, 101, 102], codes)
    assert assigned.tolist() == [0, 2, 1]                       # expected_mapping
    assert entry == [0, 2]
    assert all(100 <= docs[m] <= 102 for m in (0, 2, 1)) and docs == [100, 102, 101]
    assert layers[0][0] == [(1, 1.0)]
    assert layers[0][1] == [(0, 1.0), (2, 2.0)]                 # the nearest-first sort happens in place during the BFS
    assert layers[0][2] == [(1, 2.0)]
    assert vec.tolist() == [[0] * 5, [2] * 5, [1] * 5]          # vectors follow their points


def test_k11_layer_reindex():
    # builder.rs:577-620 test_layer_reindex: identity mapping changes nothing; the reversed mapping mirrors every id
    from muopdb_amd import hnsw_build as HB
    og = {i: [((i + 1) % 10, 1.0), ((i + 5) % 10, 2.0)] for i in range(10)}
    assert HB.layer_reindex(og, list(range(10))) == og
    rev = HB.layer_reindex(og, list(range(9, -1, -1)))
    for i in range(10):
        assert rev[i] == [((i - 1 + 10) % 10, 1.0), ((i - 5 + 10) % 10, 2.0)]


# ----------------------------------------------------------------------------- K9/K10: multi-user
def test_k9_multi_user(oracle):
    # rs/index/src/multi_spann/index.rs:358-412: user 0 = 1000 x [i,i,i,i] + doc 1000 = [1.2,2.2,3.2,4.2]
    v = np.concatenate([_line_vectors(), np.array([[1.2, 2.2, 3.2, 4.2]], np.float32)])
    f0, _, _ = H.build_spann_files(oracle, v, list(range(1001)), 10)
    v1 = _line_vectors(50) + 0.5
    f1, _, _ = H.build_spann_files(oracle, v1, list(range(5000, 5050)), 3)
    cat = F.concat_multi_spann({0: f0, (1 << 70) + 1: f1})
    ms = oracle.MultiSpannIndex(cat["user_table"], 4, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"],
                                cat["ivf_vectors"])
    # SearchParams::new(k = 3, num_probes = 2, false): ef_construction 2, as the reference's test (index.rs:398-400)
    res = ms.search_for_user([0], [[1.4, 2.4, 3.4, 4.4]], oracle.SearchParams(3, 2))
    assert res.found[0] == 1 and res.doc_ids(0) == [1000, 3, 2]
    assert ms.search_for_user([0], [[1.4, 2.4, 3.4, 4.4]], oracle.SearchParams(3, 100)).doc_ids(0) == [1000, 3, 2]
    res = ms.search_for_user([(1 << 70) + 1, 12345], [[1.4, 2.4, 3.4, 4.4]] * 2, oracle.SearchParams(2, 100))
    assert res.doc_ids(0) == [5002, 5003] and res.found[1] == 0 and res.counts[1] == 0
    # the concatenation pads index blobs to 16 and vector blobs to 8 (multi_spann/writer.rs:171-229)
    recs = [F.unpack_user_index_info(cat["user_table"][i * 112:(i + 1) * 112]) for i in range(2)]
    assert recs[0]["user_id"] == 0 and recs[1]["user_id"] == (1 << 70) + 1
    assert recs[1]["centroid_index_offset"] % 16 == 0 and recs[1]["ivf_index_offset"] % 16 == 0
    assert recs[1]["centroid_vector_offset"] % 8 == 0 and recs[1]["ivf_vectors_offset"] % 8 == 0


def test_k10_ratio_filter(oracle):
    # rs/index/src/multi_spann/reader.rs:80-117: the centroid ratio filter leaves ONE list for user 0
    u0 = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    f0, _, _ = H.build_spann_files(oracle, u0, [1, 2], 2, centroids=u0.copy())
    u1 = np.array([[9, 10, 11, 12]], np.float32)
    f1, _, _ = H.build_spann_files(oracle, u1, [3], 1, centroids=u1.copy())
    cat = F.concat_multi_spann({0: f0, 1: f1})
    ms = oracle.MultiSpannIndex(cat["user_table"], 4, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"],
                                cat["ivf_vectors"])
    p = oracle.SearchParams(3, 100)
    res = ms.search_for_user([0, 1], [[1, 2, 3, 4]] * 2, p)
    assert res.doc_ids(0) == [1] and res.doc_ids(1) == [3]
    allr = ms.search_for_users([0, 1], [1, 2, 3, 4], p)       # snapshot.rs:39-66
    assert allr.doc_ids(0) == [1, 3]
    # PQ variant (reader.rs:119-190): lossy codes, still one list per user
    cb = H.train_pq_codebook(np.concatenate([u0, u1]), 2, 1)
    pq = oracle.ProductQuantizer(4, 2, 1, cb)
    g0, _, _ = H.build_spann_files(oracle, u0, [1, 2], 2, centroids=u0.copy(), quantize=pq.quantize)
    g1, _, _ = H.build_spann_files(oracle, u1, [3], 1, centroids=u1.copy(), quantize=pq.quantize)
    cat = F.concat_multi_spann({0: g0, 1: g1})
    quant = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 2, 1, cb)
    ms = oracle.MultiSpannIndex(cat["user_table"], 4, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"],
                                cat["ivf_vectors"], quant)
    res = ms.search_for_user([0, 1], [[1, 2, 3, 4]] * 2, p)
    assert res.doc_ids(0) == [1] and res.doc_ids(1) == [3]


# ----------------------------------------------------------------------------- K16-K18: the persisted tombstone log
def test_k16_invalidated_ids_storage_files(tmp_path):
    """rs/index/src/ivf/files/invalidated_ids.rs tests: test_invalidate :259-299 (1024-byte files, one record: backing id 0,
    offset 32, the 32 LE bytes), test_invalidate_multiple_files :301-371 (64-byte files = 2 records each, 10 records ->
    files 0..4), test_read_multiple_files :413-463 (31 records: read() recovers backing id / offset / size, iter yields them
    in order, an append lands in the last file), test_invalidate_batch :465-545 (2 + 2048 records through 1024-byte files;
    a re-read ends at offset 64 again).  Writer = the product's formats.InvalidatedIdsStorage, reader = that AND the oracle."""
    import os
    from oracle.oracle import invalidated_ids_iter
    user_id, doc_id = 123456789012345678901234567890123456, 987654321
    d = str(tmp_path / "a"); os.makedirs(d)
    st = F.InvalidatedIdsStorage(d, 1024)
    st.invalidate(user_id, doc_id)
    assert (st.current_backing_id, st.current_offset, st.num_entries()) == (0, 32, 1)
    raw = open(os.path.join(d, "invalidated_ids.bin.0"), "rb").read()
    assert raw == user_id.to_bytes(16, "little") + doc_id.to_bytes(16, "little")
    rd = F.InvalidatedIdsStorage.read(d)                              # test_read_single_file :373-411
    assert (rd.current_backing_id, rd.current_offset, rd.backing_file_size) == (0, 32, 8192)
    assert next(iter(rd)) == (user_id, doc_id) == next(invalidated_ids_iter(d))
    rd.invalidate(user_id, doc_id + 1)
    assert rd.current_offset == 64
    d = str(tmp_path / "b"); os.makedirs(d)
    st = F.InvalidatedIdsStorage(d, 64)
    for i in range(10):
        st.invalidate(i, i)
    assert st.current_backing_id == 4 and st.num_entries() == 10
    for fid in range(5):
        raw = open(os.path.join(d, "invalidated_ids.bin.%d" % fid), "rb").read()
        assert raw == b"".join(F.u128_bytes(i) * 2 for i in range(2 * fid, 2 * fid + 2))
    d = str(tmp_path / "c"); os.makedirs(d)
    st = F.InvalidatedIdsStorage(d, 64)
    for i in range(31):
        st.invalidate(i, i)
    rd = F.InvalidatedIdsStorage.read(d)
    assert (rd.current_backing_id, rd.current_offset, rd.backing_file_size) == (st.current_backing_id, st.current_offset, st.backing_file_size) == (15, 32, 64)
    assert list(rd) == [(i, i) for i in range(31)] == list(invalidated_ids_iter(d))
    rd.invalidate(31, 31)
    assert rd.current_offset == 64 and list(rd)[-1] == (31, 31) and len(list(invalidated_ids_iter(d))) == 32
    d = str(tmp_path / "d"); os.makedirs(d)
    st = F.InvalidatedIdsStorage(d, 1024)
    user2, doc2 = 223456789012345678901234567890123456, 987654322
    st.invalidate_batch([(user_id, doc_id), (user2, doc2)])
    rd = F.InvalidatedIdsStorage.read(d)
    assert (rd.current_backing_id, rd.current_offset) == (0, 64) and list(rd) == [(user_id, doc_id), (user2, doc2)]
    large = [(user_id + i, doc_id + i) for i in range(2048)]
    st.invalidate_batch(large)
    rd = F.InvalidatedIdsStorage.read(d)
    assert rd.current_offset == 64
    assert list(rd) == [(user_id, doc_id), (user2, doc2)] + large == list(invalidated_ids_iter(d))


def test_k16_multi_spann_create_with_invalidation(oracle, tmp_path):
    """multi_spann/index.rs:525-599: the K9 collection opened over a log that already holds (user 0, doc 1000):
    query [1.4, 2.4, 3.4, 4.4], k = 3, ef 2 -> docs 3, 2, 4 (1000 is dead from the first search on)."""
    import os
    v = np.concatenate([_line_vectors(), np.array([[1.2, 2.2, 3.2, 4.2]], np.float32)])
    f0, _, _ = H.build_spann_files(oracle, v, list(range(1001)), 10)
    cat = F.concat_multi_spann({0: f0})
    seg = str(tmp_path / "seg")
    os.makedirs(os.path.join(seg, "invalidated_ids_storage"))
    F.InvalidatedIdsStorage(os.path.join(seg, "invalidated_ids_storage"), 1024).invalidate(0, 1000)
    F.write_segment(seg, cat, 4)
    ms = oracle.MultiSpannIndex(cat["user_table"], 4, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    pending = ms.apply_pending_invalidations(os.path.join(seg, "invalidated_ids_storage"))
    assert pending == {0: {1000}}
    assert ms.invalidate(0, 1000) is False                            # is_invalidated: already a tombstone
    assert ms.search_for_user([0], [[1.4, 2.4, 3.4, 4.4]], oracle.SearchParams(3, 2)).doc_ids(0) == [3, 2, 4]


# ----------------------------------------------------------------------------- IVF / HNSW property pins
def test_ivf_search_properties(oracle):
    # rs/index/src/ivf/block_based/index.rs:505-572: count and ascending scores; plus exactness vs f64
    rng = np.random.default_rng(7)
    v = rng.random((2000, 16), dtype=np.float32)
    c = H.kmeans(v, 20)
    index, vec, pls = H.build_ivf_files(v, list(range(100, 2100)), c)
    ivf = oracle.BlockBasedIvf(index, vec)
    q = rng.random((5, 16), dtype=np.float32)
    res = ivf.search(q, 10, num_probes=20)   # probing every list == exact
    d64 = np.sqrt(((q[:, None, :].astype(np.float64) - v[None]) ** 2).sum(-1))
    for qi in range(5):
        assert res.counts[qi] == 10
        s = res.scores[qi]
        assert np.all(s[:-1] <= s[1:])
        assert [x - 100 for x in res.doc_ids(qi)] == np.argsort(d64[qi], kind="stable")[:10].tolist()
    probes = ivf.find_nearest_centroids(q, 3)
    dc = np.sqrt(((q[:, None, :].astype(np.float64) - c[None]) ** 2).sum(-1))
    assert probes.tolist() == np.argsort(dc, axis=1, kind="stable")[:, :3].tolist()
    with pytest.raises(ValueError):
        ivf.find_nearest_centroids(q, 0)
    with pytest.raises(ValueError):
        ivf.find_nearest_centroids(q, 21)
    # duplicates are kept when a point sits in two probed lists (index.rs:250-286 has no dedup)
    index2, vec2, _ = H.build_ivf_files(v[:50], list(range(50)), c[:4], clusters_per_vector=2)
    ivf2 = oracle.BlockBasedIvf(index2, vec2)
    r2 = ivf2.search(v[:1], 4, num_probes=4)
    assert r2.doc_ids(0)[:2] == [0, 0] and r2.scores[0][0] == 0.0


def test_hnsw_search_properties(oracle):
    # rs/index/src/hnsw/block_based/index.rs:369-462: k results, ascending; recall vs exact on easy data
    rng = np.random.default_rng(9)
    v = rng.random((1500, 8), dtype=np.float32)
    hidx, hvec = H.build_hnsw_files(oracle, v, list(range(1500)), max_neighbors=12, max_layers=4, ef_construction=60)
    h = oracle.BlockBasedHnsw(hidx, hvec, 8)
    q = rng.random((20, 8), dtype=np.float32)
    res = h.ann_search(q, 10, 100)
    d64 = np.sqrt(((q[:, None, :].astype(np.float64) - v[None]) ** 2).sum(-1))
    hits = 0
    for qi in range(20):
        assert res.counts[qi] == 10
        s = res.scores[qi]
        assert np.all(s[:-1] <= s[1:])
        hits += len(set(res.doc_ids(qi)) & set(np.argsort(d64[qi])[:10].tolist()))
    assert hits >= 0.9 * 200
    evals, expanded = h.stats()
    assert evals > expanded > 0


def test_ivf_assign_rule(oracle):
    # ivf/builder.rs:305-321: |d - nearest| <= nearest * threshold on SQUARED distances, among the mc nearest
    cent = np.array([[0, 0], [10, 0], [0, 11], [100, 100]], np.float32)
    v = np.array([[5, 0], [1, 0], [5.2, 0], [0, 0]], np.float32)
    ids, cnt = oracle.ivf_assign(cent, v, 2, 0.1)
    assert cnt.tolist() == [2, 1, 1, 1]          # 25 vs 25 -> both; 1 vs 81 -> one; 23.04 vs 27.04: 4 > 2.304 -> one; 0 vs 100: 100 > 0 -> one
    assert ids[0].tolist() == [0, 1] and ids[1, 0] == 0 and ids[2, 0] == 1
    ids3, cnt3 = oracle.ivf_assign(cent, v, 3, 10.0)
    assert cnt3.tolist() == [3, 1, 3, 1]          # 1 vs 81: 80 > 10; nearest == 0: only exact zeros pass (nearest * thr == 0)
    with pytest.raises(IndexError):
        oracle.ivf_assign(cent, v, 5, 0.1)


def test_c1_golden_fixture(oracle):
    # tests/golden/c1_flat.npz (scripts/make_c1_fixture.py): BASELINE config C1 on the reference's own test dataset
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "c1_flat.npz"))
    base = H.test_hdf5_like()
    assert np.array_equal(base[:256], g["base_head"])          # the regenerated base is the stored array
    ids, dist = oracle.flat_topk(0, base, g["queries"], 10)
    assert np.array_equal(ids, g["ids"]) and np.array_equal(dist.view(np.uint32), g["dist"].view(np.uint32))


def test_golden_index_fixtures(oracle):
    """tests/golden/{hnsw_small,ivfpq_small,mspann_small}.npz (scripts/make_index_fixtures.py): index files in the reference's
    formats + seeded queries + the answers the oracle gave when they were committed — a regression pin of the restatement
    (doc ids, score BITS, HNSW traversal counters)."""
    import os
    gold = os.path.join(os.path.dirname(__file__), "golden")
    g = np.load(os.path.join(gold, "hnsw_small.npz"))
    o = oracle.BlockBasedHnsw(g["index"].tobytes(), g["vectors"].tobytes(), int(g["dimension"]))
    for ef in (40, 600):
        o.stats()
        r = o.ann_search(g["queries"], int(g["k"]), ef)
        assert H.result_rows(r, len(g["queries"])) == H.golden_rows(g, "ef%d_" % ef)
        assert list(o.stats()) == [int(x) for x in g["ef%d_counters" % ef]]
    g = np.load(os.path.join(gold, "ivfpq_small.npz"))
    o = oracle.BlockBasedIvf(g["index"].tobytes(), g["vectors"].tobytes(), oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 8, 5, g["codebook"]))
    q, k, P = g["queries"], int(g["k"]), int(g["nprobe"])
    assert np.array_equal(o.find_nearest_centroids(q, P), g["probes"])
    assert H.result_rows(o.search(q, k, num_probes=P), len(q)) == H.golden_rows(g, "a_")
    for lo, hi in zip(g["dead_lo"], g["dead_hi"]):
        assert o.invalidate((int(hi) << 64) | int(lo))
    assert H.result_rows(o.search(q, k, num_probes=P), len(q)) == H.golden_rows(g, "b_")
    g = np.load(os.path.join(gold, "mspann_small.npz"))
    o = oracle.MultiSpannIndex(g["user_table"].tobytes(), 8, g["hnsw_index"].tobytes(), g["hnsw_vectors"].tobytes(),
                               g["ivf_index"].tobytes(), g["ivf_vectors"].tobytes())
    p = oracle.SearchParams(5, 50, num_explored_centroids=4, centroid_distance_ratio=0.3)
    r = o.search_for_user([int(u) for u in g["user_ids"]], g["queries"], p)
    assert [bool(f) for f in r.found] == [bool(f) for f in g["found"]]
    docs, bits = H.golden_rows(g)
    for i, f in enumerate(g["found"]):
        if f:
            assert r.doc_ids(i) == docs[i]
            assert [int(x) for x in np.asarray(r.scores[i, :len(docs[i])], np.float32).view(np.uint32)] == bits[i]


# ----------------------------------------------------------------------------------- K15: IvfBuilder::reindex
# the reference's own known answers: rs/index/src/ivf/builder.rs:1037-1108 (ids_0), 1110-1181 (ids_1), 1183-1266 (ids_2),
# 1268-1343 (ids_3), 1345-1406 (reindex: vectors [i] and doc ids i + 100 in their new places)
K15_CASES = [
    (22, [[11, 12, 13], [0, 2, 4, 6, 8, 20], [9, 18, 20], [14, 15, 16, 18], [1, 3, 5, 7, 18, 20], [10, 15, 21], [10, 15, 17, 19]],
     {10: 0, 14: 1, 15: 2, 1: 3, 3: 4, 5: 5, 7: 6, 9: 7, 16: 8, 18: 9, 0: 10, 2: 11, 4: 12, 6: 13, 8: 14, 20: 15, 11: 16, 12: 17,
      13: 18, 21: 19, 17: 20, 19: 21}),
    (22, [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19], [0, 4, 8, 12, 16], [1, 5, 9, 13, 17],
          [2, 6, 10, 14, 18], [3, 7, 11, 15, 19]], {i: i for i in range(20)}),
    (30, [[0, 5, 10, 15, 20, 25], [1, 6, 11, 16, 21, 26], [0, 7, 12, 17, 22, 27], [2, 8, 13, 18, 23, 28], [3, 9, 14, 19, 24, 29],
          [4, 20, 21, 22, 23, 24], [1, 25, 26, 27, 28, 29]],
     {0: 0, 1: 1, 4: 2, 5: 3, 10: 4, 15: 5, 20: 6, 6: 7, 11: 8, 16: 9, 21: 10, 7: 11, 12: 12, 17: 13, 22: 14, 2: 15, 8: 16, 13: 17,
      18: 18, 23: 19, 3: 20, 9: 21, 14: 22, 19: 23, 24: 24, 25: 25, 26: 26, 27: 27, 28: 28, 29: 29}),
    (30, [[0, 4, 8, 12, 16, 20], [1, 5, 9, 13, 17, 21], [2, 6, 10, 14, 18, 22], [3, 7, 11, 15, 19, 23], [0, 6, 12, 18], [1, 7, 13, 19]],
     {0: 0, 1: 1, 2: 2, 6: 3, 3: 4, 7: 5, 4: 6, 8: 7, 12: 8, 5: 9, 9: 10, 13: 11, 10: 12, 14: 13, 18: 14, 11: 15, 15: 16, 19: 17,
      16: 18, 20: 19, 17: 20, 21: 21, 22: 22, 23: 23}),
]


@pytest.mark.parametrize("n,lists,want", K15_CASES)
def test_k15_reassigned_ids(oracle, n, lists, want):
    from muopdb_amd import build as B
    got = oracle.reassigned_ids(lists, n)
    for old, new in want.items():
        assert got[old] == new, (old, new, got[old])
    prod = B.reassigned_ids(lists, n)                                   # the product's host logic, same answers
    assert [int(x) for x in prod] == list(got)


def test_k15_reindex_moves_vectors_and_doc_ids(oracle):
    from muopdb_amd import build as B
    n, lists, _ = K15_CASES[0]
    vec = np.arange(n, dtype=np.float32)[:, None]
    docs = np.asarray([i + 100 for i in range(n)], dtype=object)
    want_vec = [10, 14, 15, 1, 3, 5, 7, 9, 16, 18, 0, 2, 4, 6, 8, 20, 11, 12, 13, 21, 17, 19]
    for impl in (oracle.reindex, B.reindex):
        new_lists, ndocs, nvec, mapping = impl(lists, docs, vec)
        assert [float(v[0]) for v in nvec] == [float(x) for x in want_vec]
        assert [int(d) for d in ndocs] == [x + 100 for x in want_vec]
        for old_l, new_l in zip(lists, new_lists):                      # a list keeps its members (under their new names), in order
            assert [int(mapping[o]) for o in old_l] == [int(x) for x in new_l]


def test_reassigned_ids_product_equals_oracle_on_random_lists(oracle):
    """max_clusters_per_vector in {1, 2, 3}, vectors in no list, empty lists: the product's (vectorised) host logic == the restatement."""
    from muopdb_amd import build as B
    rng = np.random.default_rng(15)
    for trial in range(60):
        n = int(rng.integers(1, 120))
        nl = int(rng.integers(1, 12))
        mc = int(rng.integers(1, 4))
        lists = [[] for _ in range(nl)]
        for v in range(n):                                              # vectors are added in id order: lists are ascending (:563-575)
            if rng.random() < 0.1:
                continue
            for l in rng.choice(nl, size=min(mc, nl) if rng.random() < 0.4 else 1, replace=False):
                lists[int(l)].append(v)
        want = oracle.reassigned_ids(lists, n)
        assert [int(x) for x in B.reassigned_ids(lists, n)] == want
        valid = sorted(x for x in want if x >= 0)
        assert valid == list(range(len(valid)))                          # a permutation of 0 .. n' - 1


# ----------------------------------------------------------------------------- caller-given probe tables
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("kind", ["f32", "pq"])
def test_probe_tables_are_the_concatenation_of_their_columns(oracle, kind, metric):
    """rs/index/src/ivf/block_based/index.rs:250-286 restated without the heap: search_with_centroids over any table of list ids is
    the k smallest of the per-column results laid end to end — a list named m times contributes its points m times, in any column
    order.  With monotone doc ids (100 + 3 i) the (distance, point id) and (score, doc id) orders coincide, so ties at rank k are
    decided identically.  The worlds and tables are those of tests/test_gpu_probe_tables.py."""
    from tests.test_gpu_probe_tables import B, NLISTS, build_world
    w = build_world(oracle, kind, lambda n: [100 + 3 * i for i in range(n)])
    o, q, sizes = w["o_" + metric], w["q"], w["sizes"]
    per = []                                                             # every list on its own: (doc ids, scores) per query
    for c in range(NLISTS):
        r = o.search(q, max(sizes[c], 1), probes=np.full((B, 1), c, np.uint32))
        assert np.all(r.counts == sizes[c]) and not r.hi[:, :sizes[c]].any()
        per.append((r.lo[:, :sizes[c]].copy(), r.scores[:, :sizes[c]].copy()))
    for name, table in w["tables"].items():
        got = {k: o.search(q, k, probes=table, threads=8) for k in (1, 10, 2000)}
        for i in range(B):
            # the concatenation's order by (score, doc id): the lists' entries, each repeated once per column that names its list
            times = np.bincount(table[i], minlength=NLISTS)
            docs, sc = np.concatenate([p[0][i] for p in per]), np.concatenate([p[1][i] for p in per])
            reps = np.repeat(times, sizes)
            order = np.lexsort((docs, sc))
            docs, sc = np.repeat(docs[order], reps[order]), np.repeat(sc[order], reps[order])
            assert len(docs) == sum(sizes[c] for c in table[i])
            for k, r in got.items():
                n = min(k, len(docs))
                assert int(r.counts[i]) == n, (name, k, i)
                assert np.array_equal(r.lo[i, :n], docs[:n]) and not r.hi[i, :n].any(), (name, k, i)
                assert np.array_equal(r.scores[i, :n].view(np.uint32), sc[:n].view(np.uint32)), (name, k, i)
    with pytest.raises(ValueError):                                      # storage.rs:280-286: Err("Index out of bound")
        o.search(q, 10, probes=np.full((B, 1), NLISTS, np.uint32))

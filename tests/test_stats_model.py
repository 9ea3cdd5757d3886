"""tests/stats_model.py against the oracle's OWN counts (no GPU): the model that judges mdb_get_stats must not be validated only by the
kernels it judges.

* posting-list scans: the oracle returns every candidate it scanned when k is at least their number, so the sum of its row counts
  IS the number of scored (query, entry) pairs — with repeated lists, tombstones, shared and per-query allow bitmaps;
* SPANN: the same brute count behind the model's ratio filter over the centroid graph's rows;
* graphs: the oracle's counters are additive over a batch, which is how the model uses them; the byte formulas on hand values.
"""
import numpy as np

from tests import helpers as H
from tests import stats_model as M

ALL = 4096    # a k no probe row of these worlds reaches


def _bitmap(points, n):
    bm = np.zeros((n + 31) // 32, np.uint32)
    for p in points:
        bm[p >> 5] |= np.uint32(1 << (p & 31))
    return bm


def _ivf_world(oracle, pq):
    rng = np.random.default_rng(3)
    n, d = 600, 16
    v = H.sift_like(n, d, n_clusters=7, seed=2)
    cent = H.kmeans(v, 7, iters=3, seed=1)
    docs = [10 + 3 * i for i in range(n)]
    if pq:
        cb = H.train_pq_codebook(v, 4, 4, iters=2)
        quant = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 4, 4, cb)
        index, vec, pls = H.build_ivf_files(v, docs, cent, quantize=oracle.ProductQuantizer(d, 4, 4, cb).quantize)
    else:
        quant = oracle.Quant()
        index, vec, pls = H.build_ivf_files(v, docs, cent)
    q = (v[rng.integers(0, n, 6)] + rng.normal(0, 2, (6, d))).astype(np.float32)
    return dict(n=n, docs=docs, pls=pls, q=q, o=oracle.BlockBasedIvf(index, vec, quant), rng=rng)


def test_ivf_scored_is_the_oracles_candidate_count(oracle):
    for pq in (False, True):
        w = _ivf_world(oracle, pq)
        o, q, n, pls = w["o"], w["q"], w["n"], w["pls"]
        nearest = o.find_nearest_centroids(q, 3)
        longest = int(np.argmax([len(p) for p in pls]))
        thrice = np.concatenate([nearest, np.full((len(q), 3), longest, np.uint32)], 1)[:, [0, 3, 1, 4, 5, 2]]
        shared = _bitmap(range(0, n, 2), n)
        per_query = np.stack([_bitmap(sorted(w["rng"].choice(n, n // 2, replace=False)), n) for _ in q])
        wide = np.concatenate([per_query, np.zeros((len(q), 5), np.uint32)], 1)          # words_per_bitmap larger than needed

        def brute(probes, allow=None):
            if allow is None:
                return int(o.search(q, ALL, probes=probes).counts.sum())
            with oracle.planner_filter(allow):
                return int(o.search(q, ALL, probes=probes).counts.sum())

        def check(dead):
            for probes in (nearest, thrice):
                for allow in (None, shared, per_query, wide):
                    want = brute(probes, allow)
                    assert want < ALL * len(q)
                    assert M.ivf_scored(pls, probes, dead, allow) == want, (pq, len(dead), probes.shape, None if allow is None else allow.shape)
        check(())
        assert M.ivf_scored(pls, thrice) == sum(len(pls[int(c)]) for row in thrice for c in row) > M.ivf_scored(pls, nearest)
        # the nearest point of the longest list, per query
        one = np.full((len(q), 1), longest, np.uint32)
        res = o.search(q, 1, probes=one)
        dead_docs = sorted({res.doc_ids(i)[0] for i in range(len(q))})
        for doc in dead_docs:
            assert o.invalidate(doc)
        check([w["docs"].index(doc) for doc in dead_docs])


def test_shards_partition_the_scored_count(oracle):
    w = _ivf_world(oracle, False)
    probes = w["o"].find_nearest_centroids(w["q"], 4)
    whole = M.ivf_scored(w["pls"], probes)
    sizes = [len(p) for p in w["pls"]]
    for world in (1, 2, 3):
        for owner in (M.modulo_owner(len(sizes), world), M.balanced_owner(sizes, world)):
            parts = [M.ivf_scored(w["pls"], probes, owned={c for c, r_ in enumerate(owner) if r_ == r}) for r in range(world)]
            assert sum(parts) == whole and set(owner) == set(range(world))
    # longest first to the least loaded rank: 9 -> rank 0, 7 -> rank 1, 7 -> rank 1 (loads 9, 7), 2 -> rank 0 (loads 9, 14)
    assert M.balanced_owner([7, 9, 2, 7], 2) == [1, 0, 0, 1]


def test_spann_scored_is_the_oracles_candidate_count(oracle):
    rng = np.random.default_rng(8)
    d, nexp, ef = 16, 4, 40
    v = H.sift_like(500, d, n_clusters=12, seed=5)
    files, cent, pls = H.build_spann_files(oracle, v, [7 + 2 * i for i in range(len(v))], 10, seed=1, max_neighbors=8, max_layers=3,
                                           ef_construction=40)
    o = oracle.Spann(files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"])
    graph = oracle.BlockBasedHnsw(files["hnsw_index"], files["hnsw_vectors"], d)
    q = (v[rng.integers(0, len(v), 9)] + rng.normal(0, 3, (9, d))).astype(np.float32)
    trimmed = 0
    for ratio in (0.1, 0.5):
        rows = graph.ann_search(q, nexp, ef)
        kept = [M.ratio_filter(rows.doc_ids(i), rows.scores[i, :int(rows.counts[i])], ratio) for i in range(len(q))]
        trimmed += sum(int(rows.counts[i]) - len(kept[i]) for i in range(len(q)))
        res = o.search(q, oracle.SearchParams(ALL, ef, num_explored_centroids=nexp, centroid_distance_ratio=ratio))
        assert M.ivf_scored(pls, kept) == int(res.counts.sum()) < ALL
        for i in range(len(q)):
            assert M.ivf_scored(pls, [kept[i]]) == int(res.counts[i]), (ratio, i)
    assert trimmed > 0, "the ratio filter dropped no list: the case no longer shows it"


def test_graph_counters_are_additive_over_the_batch(oracle):
    rng = np.random.default_rng(4)
    v = H.sift_like(800, 16, n_clusters=10, seed=6)
    index, vec = H.build_hnsw_files(oracle, v, list(range(len(v))), max_neighbors=8, max_layers=3, ef_construction=40)
    o = oracle.BlockBasedHnsw(index, vec, 16)
    q = (v[rng.integers(0, len(v), 5)] + rng.normal(0, 2, (5, 16))).astype(np.float32)
    o.stats()
    o.ann_search(q, 10, 48)
    whole = o.stats()
    single = []
    for i in range(len(q)):
        o.ann_search(q[i:i + 1], 10, 48)
        single.append(o.stats())
    assert whole == (sum(e for e, _ in single), sum(x for _, x in single)) and whole[0] > whole[1] > 0
    assert o.stats() == (0, 0)                      # reading resets


def test_byte_formulas():
    assert M.flat(777, 30, 5, 3) == dict(scored_vectors=3885, distance_evals=0, expanded_nodes=0, algorithmic_bytes=777 * 120 + 5 * 120 + 5 * 3 * 8)
    assert M.flat(4100, 96, 1, 0)["algorithmic_bytes"] == 4100 * 384 + 384
    assert M.hnsw(1000, 70, d=128) == dict(scored_vectors=0, distance_evals=1000, expanded_nodes=70, algorithmic_bytes=1000 * 516 + 70 * 16)
    assert M.hnsw(1000, 70, m=8)["algorithmic_bytes"] == 1000 * 12 + 70 * 16
    pls = [np.array([0, 1, 2]), np.array([3]), np.array([], np.uint64)]
    assert M.ivf(pls, [[0, 1], [2, 0]], d=32) == dict(scored_vectors=7, distance_evals=0, expanded_nodes=0, algorithmic_bytes=7 * 132)
    assert M.ivf(pls, [[0, 0, 0]], m=16, dead=[1])["algorithmic_bytes"] == 6 * 20
    assert M.spann(50, 9, 200, 32) == dict(scored_vectors=200, distance_evals=50, expanded_nodes=9, algorithmic_bytes=50 * 132 + 9 * 16 + 200 * 132)
    assert M.spann(50, 9, 200, 32, m=8)["algorithmic_bytes"] == 50 * 132 + 9 * 16 + 200 * 12
    assert M.ratio_filter([4, 2, 9], [2.0, 2.1, 2.3], 0.1) == [4, 2] and M.ratio_filter([], [], 0.1) == []

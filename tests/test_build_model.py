"""CPU tests of tests/build_model.py, the plain restatements that tests/test_gpu_build_exact.py holds muopdb_amd.build against:
the models build well-formed graphs, every configuration really meets the situation it exists for (so the GPU comparison
cannot pass vacuously), and each model run stays quick."""
import time

import numpy as np
import pytest

from tests import build_model as BM


@pytest.mark.parametrize("name", list(BM.HNSW_CASES))
def test_hnsw_model_graph_is_well_formed_and_meets_its_case(oracle, name):
    t0 = time.perf_counter()
    x, kw, (layers, levels, stats) = BM.hnsw_model_of(oracle, name)
    took = time.perf_counter() - t0
    print(name, stats, "layers", len(layers), "%.2f s" % took)
    n, d, M, max_layers, efc, batch_frac, exact_below, seed, exists_for = BM.HNSW_CASES[name]
    assert x.shape == (n, d) and len(levels) == n and len(layers[0][0]) == n
    BM.check_graph_invariants(layers, levels, M)
    for key in exists_for:
        assert stats[key] > 0, (key, stats)
    assert stats["tied_pools"] > 0, stats                 # the copies of row 3 reach the heuristic at bit-equal distance
    assert took < 5.0
    if name == "exact":
        assert len(layers) == 5
    if name == "graph":
        assert stats["graph_batches"] >= 10
    if name == "seq":
        assert stats["batches"] == n - 1 and levels[0] > 0
    if name == "bigbatch":
        assert stats["batches"] < 12                      # the batches double


def test_hnsw_model_is_deterministic_and_the_lists_survive_the_file_format(oracle):
    """a second run gives the same graph; written and read back through the oracle's reader the lists are unchanged"""
    from muopdb_amd import formats as F
    x, kw, (layers, levels, stats) = BM.hnsw_model_of(oracle, "exact")
    assert any(not lst for _, lists in layers[1:] for lst in lists)       # an empty list: the reader reports it as absent
    again, levels2, stats2 = BM.insert_hnsw_model(oracle, x, **kw)
    assert BM.first_difference(again, layers) is None and np.array_equal(levels, levels2) and stats == stats2
    assert BM.layers_as_lists(BM.lists_as_csr(layers)) == layers
    o = oracle.BlockBasedHnsw(F.write_hnsw_index(BM.lists_as_csr(layers), np.arange(len(x), dtype=np.uint64), x.shape[1]),
                              F.write_vector_file(x), x.shape[1])
    assert o.entry_point == layers[-1][0][0] and o.num_layers == len(layers)
    for l, (pts, lists) in enumerate(layers):
        for p, lst in zip(pts, lists):
            assert BM.edges_read_back(o, p, l) == lst


def test_first_difference_names_the_lowest_layer_and_point():
    a = [([0, 1, 2], [[1], [0, 2], [1]]), ([2, 0], [[0], [2]])]
    b = [([0, 1, 2], [[1], [2, 0], [1]]), ([0, 2], [[2], [0]])]
    assert BM.first_difference(a, a) is None
    assert BM.first_difference(a, b) == (0, 1, [0, 2], [2, 0])
    assert BM.first_difference(a, [a[0], b[1]]) == (1, None, [2, 0], [0, 2])
    assert BM.first_difference(a, a[:1])[0] == 1
    assert BM.batch_of(400, 0.125, 1) == (0, 1, 1) and BM.batch_of(400, 1.0, 5) == (2, 4, 7)
    assert BM.batch_of(400, 1.0, 399) == (8, 256, 399)


def test_ivf_model_splits_lists_and_splits_a_split_list_again(oracle):
    x, kw = BM.ivf_case()
    cent, lists, stats = BM.ivf_build_centroids_model(oracle, x, **kw)
    print(stats, [len(p) for p in lists])
    assert stats["splits"] >= 2 and stats["resplits"] >= 1, stats
    assert cent.shape == (len(lists), x.shape[1])
    assert 0 < min(len(p) for p in lists) and max(len(p) for p in lists) <= kw["max_posting_list_size"]
    assert sorted(p for pl in lists for p in pl) == list(range(len(x)))


def test_pq_model_pads_a_short_codebook_and_follows_the_sample(oracle):
    x = BM.H.sift_like(600, 24, n_clusters=5, seed=4)
    cb = BM.train_pq_codebook_model(oracle, x[:10], 8, 4, iters=4, seed=1).reshape(3, 16, 8)
    assert np.array_equal(cb[:, 10:], np.repeat(cb[:, 9:10], 6, 1))          # 10 points, 16 codes: the last row six more times
    assert len({r.tobytes() for r in cb[0, :10]}) == 10
    full = BM.train_pq_codebook_model(oracle, x, 8, 4, iters=4, seed=1, sample=None)
    part = BM.train_pq_codebook_model(oracle, x, 8, 4, iters=4, seed=1, sample=200)
    rows = np.sort(np.random.default_rng(1 + 104729).choice(600, size=200, replace=False))
    assert not np.array_equal(full, part)
    assert np.array_equal(part, BM.train_pq_codebook_model(oracle, x[rows], 8, 4, iters=4, seed=1, sample=None))

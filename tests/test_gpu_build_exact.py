"""GPU tests (-m gpu) that pin the build side EXACTLY: muopdb_amd.build's batched HNSW insertion, PQ codebook
training, IvfBuilder::build_centroids' list splitting and the sampled k-means against the plain CPU models of
tests/build_model.py.  Every distance in these builders is one the oracle reproduces bit for bit, and every random draw
comes from a seeded numpy generator, so the products must give the models' edge lists in the models' order and the models'
centroid bits.  tests/test_build_model.py shows on the CPU that each configuration meets the situation it exists for
(trims with and without room, more than 2M newcomers, graph-search batches, a new top layer of several points, ties)."""
import numpy as np
import pytest

from tests import build_model as BM
from tests import helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _as_input(x, device):
    if device == "numpy":
        return x
    import torch
    return torch.from_numpy(x).cuda()


def _assert_graph_equals_model(name, got_layers, got_levels, model):
    layers, levels, _ = model
    n, batch_frac = BM.HNSW_CASES[name][0], BM.HNSW_CASES[name][5]
    assert np.array_equal(np.asarray(got_levels, np.int64), levels), "%s: levels differ" % name
    diff = BM.first_difference(BM.layers_as_lists(got_layers), layers)
    if diff is None:
        return
    layer, point, got, want = diff
    if point is None:
        pytest.fail("%s: layer %d: built %s, the model has %s" % (name, layer, got, want))
    newest = max(got + want + [point])
    pytest.fail("%s: layer %d, point %d (batch %d = points %d..%d): built %s, the model has %s; the newest point in either list "
                "came with batch %d = points %d..%d" % ((name, layer, point) + BM.batch_of(n, batch_frac, point) + (got, want)
                                                       + BM.batch_of(n, batch_frac, newest)))


# ------------------------------------------------------------------------------------------ HNSW
@pytest.mark.parametrize("name", list(BM.HNSW_CASES))
def test_insert_hnsw_builds_the_models_edge_lists(ctx, oracle, name):
    """the same levels, the same number of layers, per layer the same points in the same order and per point the same
    neighbours as a SEQUENCE"""
    from muopdb_amd import build as B
    x, kw, model = BM.hnsw_model_of(oracle, name)
    layers, levels = B.insert_hnsw(ctx, x, **kw)
    _assert_graph_equals_model(name, layers, levels, model)


def test_insert_hnsw_from_a_device_tensor_builds_the_same_graph(ctx, oracle):
    """x as a torch CUDA tensor: the selection kernel then reads device rows; the graph is that of the numpy input, which
    test_insert_hnsw_builds_the_models_edge_lists[graph] holds against the same model"""
    import torch
    from muopdb_amd import build as B
    x, kw, model = BM.hnsw_model_of(oracle, "graph")
    layers, levels = B.insert_hnsw(ctx, torch.from_numpy(x).cuda(), **kw)
    _assert_graph_equals_model("graph", layers, levels, model)


def test_hnsw_file_by_insertion_read_back_by_the_oracle(ctx, oracle):
    """hnsw_files_by_insertion with permuted doc ids: the oracle's reader finds the model's edge list under every point of
    every layer and the model's entry point; the GPU traversal of the file equals the oracle's; the doc ids are the
    permutation of the point ids that a search of the model's own graph returns"""
    from muopdb_amd import build as B
    from muopdb_amd import formats as F
    from muopdb_amd.index import BlockBasedHnsw
    x, kw, (layers, levels, _) = BM.hnsw_model_of(oracle, "exact")
    n, d = x.shape
    perm = (np.random.default_rng(11).permutation(n) + 1000).astype(np.uint64)
    idx, vec = B.hnsw_files_by_insertion(ctx, x, doc_ids=perm, **kw)
    o = oracle.BlockBasedHnsw(idx, vec, d)
    assert o.num_layers == len(layers) and o.entry_point == layers[-1][0][0]
    for l, (pts, lists) in enumerate(layers):
        for p, lst in zip(pts, lists):
            assert BM.edges_read_back(o, p, l) == lst, (l, p)
    rng = np.random.default_rng(12)
    q = (x[rng.integers(0, n, 32)] + rng.normal(0, 4, (32, d))).astype(np.float32)
    g = BlockBasedHnsw(ctx, idx, vec, d)
    res, ores = g.ann_search(q, 10, 20), o.ann_search(q, 10, 20)
    g.close()
    plain = oracle.BlockBasedHnsw(F.write_hnsw_index(BM.lists_as_csr(layers), np.arange(n, dtype=np.uint64), d),
                                  F.write_vector_file(x), d).ann_search(q, 10, 20)
    for i in range(32):
        c = int(ores.counts[i])
        assert c == 10 and res.doc_ids(i) == ores.doc_ids(i), i
        assert np.array_equal(_bits(res.scores[i, :c]), _bits(ores.scores[i, :c]))
        assert res.doc_ids(i) == [int(perm[p]) for p in plain.doc_ids(i)], i


# ------------------------------------------------------------------------------------------ PQ codebook
@pytest.mark.parametrize("device", ["numpy", "cuda"])
@pytest.mark.parametrize("n,d,subdim,sample", [
    (600, 24, 8, None),
    (600, 12, 3, None),      # subvectors of 3: the scalar tail of the distance cascade
    (10, 24, 8, None),       # fewer points than codes: padded rows
    (600, 24, 8, 200),       # a sample of the rows
])
def test_train_pq_codebook_bit_parity(ctx, oracle, n, d, subdim, sample, device):
    """the codebook bits of the model; from a device tensor the subvector slices are non-contiguous views"""
    from muopdb_amd import build as B
    x = H.sift_like(600, d, n_clusters=5, seed=4)[:n]
    want = BM.train_pq_codebook_model(oracle, x, subdim, 4, iters=6, seed=3, sample=sample)
    got = B.train_pq_codebook(ctx, _as_input(x, device), subdim, 4, iters=6, seed=3, sample=sample)
    assert got.shape == want.shape == ((d // subdim) * 16 * subdim,)
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------ IVF list splitting
@pytest.mark.parametrize("device", ["numpy", "cuda"])
def test_ivf_build_centroids_equals_the_model(ctx, oracle, device):
    """the model's centroid bits and the model's lists, list for list (test_build_model.py: this input splits several
    lists, one of them the product of an earlier split)"""
    from muopdb_amd import build as B
    x, kw = BM.ivf_case()
    want_cent, want_lists, _ = BM.ivf_build_centroids_model(oracle, x, **kw)
    cent, lists = B.ivf_build_centroids(ctx, _as_input(x, device), **kw)
    assert len(lists) == len(want_lists) == cent.shape[0]
    for i, (got, want) in enumerate(zip(lists, want_lists)):
        assert got.dtype == np.uint64 and got.tolist() == want, "list %d" % i
    assert np.array_equal(_bits(cent), _bits(want_cent))


# ------------------------------------------------------------------------------------------ sampled k-means
@pytest.mark.parametrize("device", ["numpy", "cuda"])
def test_sampled_kmeans_bit_parity(ctx, oracle, device):
    """kmeans(..., sample=): oracle.kmeans_fit on the same sampled rows from the same initial points"""
    from muopdb_amd import build as B
    x = H.sift_like(1000, 16, n_clusters=7, seed=6)
    want = BM.kmeans_sample_model(oracle, x, 12, iters=6, seed=5, sample=300, tolerance=1e-4)
    got = B.kmeans(ctx, _as_input(x, device), 12, iters=6, seed=5, sample=300, tolerance=1e-4)
    got = got.cpu().numpy() if device == "cuda" else got
    assert got.shape == (12, 16) and np.array_equal(_bits(got), _bits(want))
    whole = BM.kmeans_sample_model(oracle, x, 12, iters=6, seed=5, sample=None, tolerance=1e-4)
    assert not np.array_equal(_bits(want), _bits(whole))     # the sample matters

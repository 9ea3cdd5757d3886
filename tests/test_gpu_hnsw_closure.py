"""The upper layers of the HNSW table path frontier by frontier (muopdb_amd/csrc/mdb_hnsw_closure.hip.h, MDB_HNSW_CLOSURE) against
the oracle (-m gpu): rows, score bits, counts, distance_evals and expanded_nodes, and against the sequential kernels
(MDB_HNSW_CLOSURE=0) on every case.

One graph serves the module: 20 000 x 32 Gaussian rows, synth.bulk_hnsw with max_neighbors = 8 on the CPU (the same graph on every
machine) — layer 1 ~2 500 points, layer 2 ~300 (the split path's TOP set), a tiny top layer.  The tie-heavy and the non-finite cases
keep its topology and overwrite the vector file, as tests/test_gpu_nonfinite.py does.

  * float rows: no query may take the fallback (mdb_hnsw_closure_fallbacks == 0; tests/closure_model.py says so for this seed);
  * integer rows in 0..3: the fallback must run (> 0), and rows and counters are still the oracle's;
  * ef 1, 2, 63, 64, 200, 256, 300, 448 and the three values that put the TOP set at ef + 1, ef and ef - 1 points (theta finite /
    +inf: the boundary with the closure of a whole small layer); batches 1, 31, 32, 64 (both sides of the split path); L2 and dot.
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

N, D, SEED = 20000, 32, 5
ERR_NAN = 5
EFS = [1, 2, 63, 64, 200, 256, 300, 448]


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def graph():
    import torch
    from muopdb_amd import synth
    rng = np.random.default_rng(SEED)
    x = rng.standard_normal((N, D)).astype(np.float32)
    layers, levels = synth.bulk_hnsw(torch.from_numpy(x), max_neighbors=8, max_layers=8, kcand=64, seed=SEED)
    assert len(layers) >= 4 and 2000 <= len(layers[1][0]) <= 3000 and 200 <= len(layers[2][0]) <= 447
    q = rng.standard_normal((64, D)).astype(np.float32)
    return dict(x=x, layers=layers, levels=levels, q=q, index=F.write_hnsw_index(layers, np.arange(N, dtype=np.uint64), D))


def _pair(ctx, oracle, index, vectors, metric):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    vf = F.write_vector_file(vectors)
    return (BlockBasedHnsw(ctx, index, vf, D, NoQuantizer(D, metric)),
            oracle.BlockBasedHnsw(index, vf, D, oracle.Quant(oracle.QUANT_NONE, metric)))


def _rows(res, b):
    return ([int(c) for c in res.counts[:b]],) + H.result_rows(res, b)


def _check(ctx, g, o, q, k, ef):
    """both switch positions against the oracle; -> queries the frontier form handed to the sequential kernels"""
    b = len(q)
    o.stats()
    want = o.ann_search(q, k, ef)
    evals, expanded = o.stats()
    out = {}
    for closure in (1, 0):
        with ctx.option("MDB_HNSW_CLOSURE", closure):
            got = g.ann_search(q, k, ef)
            st = ctx.stats()
            fb = ctx.closure_fallbacks()
        assert _rows(got, b) == _rows(want, b), (closure, ef, b)
        assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (closure, ef, b)
        out[closure] = fb
    assert out[0] == 0
    assert out[1] <= b
    return out[1]


def _efs(graph):
    n2 = len(graph["layers"][2][0])
    return EFS + [n2 - 1, n2, n2 + 1]


@pytest.mark.parametrize("b", [1, 31, 32, 64])
@pytest.mark.parametrize("metric", [0, 1])
def test_float_rows_take_no_fallback(ctx, oracle, graph, metric, b):
    g, o = _pair(ctx, oracle, graph["index"], graph["x"], metric)
    for ef in _efs(graph):
        fb = _check(ctx, g, o, graph["q"][:b], 10, ef)
        assert fb == 0, "ef %d, batch %d: %d queries took the fallback on rows without exact ties" % (ef, b, fb)


@pytest.mark.parametrize("b", [1, 31, 32, 64])
@pytest.mark.parametrize("metric", [0, 1])
def test_integer_rows_take_the_fallback_and_stay_exact(ctx, oracle, graph, metric, b):
    rng = np.random.default_rng(SEED + 1)
    x = rng.integers(0, 4, (N, D)).astype(np.float32)
    q = rng.integers(0, 4, (64, D)).astype(np.float32)
    g, o = _pair(ctx, oracle, graph["index"], x, metric)
    total = 0
    for ef in _efs(graph):
        fb = _check(ctx, g, o, q[:b], 10, ef)
        print("metric %d batch %d ef %d: %d of %d queries fell back" % (metric, b, ef, fb, b))
        total += fb
    assert total > 0, "no query took the fallback on tie-heavy rows: the case no longer shows both paths"


def _upper_points(graph, level):
    return np.flatnonzero(graph["levels"] == level)


@pytest.mark.parametrize("b", [31, 64])
@pytest.mark.parametrize("metric", [0, 1])
def test_inf_and_exact_zero_distances_in_upper_layer_points(ctx, oracle, graph, metric, b):
    """+inf orders behind every number and in front of nothing; exact zeros tie with each other (copies of the queries: L2 distance
    +0.0; an all-zero point: dot score -0.0) — rows, score bits and counters on both switch positions"""
    x = graph["x"].copy()
    q = graph["q"][:b]
    up1, up2 = _upper_points(graph, 1), _upper_points(graph, 2)
    x[up2[3], 5] = np.inf
    x[up1[10], 0] = np.inf
    x[up1[20:26]] = q[0]
    x[up2[7:10]] = q[1]
    x[up1[40:44]] = 0.0
    x[up2[12]] = 0.0
    g, o = _pair(ctx, oracle, graph["index"], x, metric)
    for ef in (16, 64, 200):
        _check(ctx, g, o, q, 10, ef)


@pytest.mark.parametrize("metric", [0, 1])
def test_nan_in_an_upper_layer_point(ctx, oracle, graph, metric):
    """a NaN distance is the sequential kernels' to report (MDB_ERR_NAN where the reference panics, and only there): a batch with a
    query that evaluates the point fails, a batch of queries that never reach it returns the oracle's rows"""
    from muopdb_amd import lib as L
    x = graph["x"].copy()
    p = int(_upper_points(graph, 1)[17])
    x[p, 2] = np.nan
    g, o = _pair(ctx, oracle, graph["index"], x, metric)
    q, ef = graph["q"], 16
    hit = np.zeros(len(q), bool)
    for i in range(len(q)):
        try:
            o.ann_search(q[i:i + 1], 10, ef)
        except ValueError:
            hit[i] = True
    assert hit.any() and not hit.all(), "the planted point must be reached by some queries only (%d of %d)" % (hit.sum(), len(q))
    for closure in (1, 0):
        with ctx.option("MDB_HNSW_CLOSURE", closure):
            for qs in (q[hit], q[:40]):
                with pytest.raises(L.MuopdbError) as e:
                    g.ann_search(qs, 10, ef)
                assert e.value.status == ERR_NAN
    _check(ctx, g, o, q[~hit], 10, ef)
    _check(ctx, g, o, np.repeat(q[~hit], 4, axis=0)[:40], 10, ef)   # the split path's batch size


@pytest.mark.parametrize("b", [31, 64])
def test_upper_rows_with_duplicate_edges(ctx, oracle, graph, b):
    """an upper-layer row that names a point twice: two lanes of one frontier round hit the same visited bit and exactly one is new"""
    rng = np.random.default_rng(SEED + 2)
    layers = list(graph["layers"])
    dup = 0
    for li in (1, 2):
        ids, indptr, edges = layers[li]
        rows = [list(edges[int(indptr[i]):int(indptr[i + 1])]) for i in range(len(ids))]
        for r in rows:
            if len(r) >= 3 and rng.random() < 0.3:
                for _ in range(int(rng.integers(1, 3))):
                    r.insert(int(rng.integers(0, len(r) + 1)), r[int(rng.integers(0, len(r)))])
                dup += 1
        lens = np.array([len(r) for r in rows])
        layers[li] = (ids, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), np.concatenate(rows).astype(np.uint32))
    assert dup > 300
    index = F.write_hnsw_index(layers, np.arange(N, dtype=np.uint64), D)
    g, o = _pair(ctx, oracle, index, graph["x"], 0)
    for ef in (2, 64, 200):
        assert _check(ctx, g, o, graph["q"][:b], 10, ef) == 0

"""mdb_hnsw_describe_search against the handle it describes: the route it prints is the route hnsw_route (csrc/mdb_hnsw_route.h) gives for
the handle's shape — computed here by tests/host/hnsw_route_main.cpp, the header alone — and the searches it describes return the
oracle's rows and traversal counters, over the batch sizes, ef values and options at which the route changes form."""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H
from tests.test_gpu_dispatch import options
from tests.test_gpu_instantiations import _ring_layer
from tests.test_gpu_parity import assert_result_rows

pytestmark = pytest.mark.gpu

BATCHES, EFS = (1, 31, 32), (200, 209, 300, 449)
OPTION_SETS = (dict(), dict(MDB_HNSW_RANK=0), dict(MDB_HNSW_RANK=3), dict(MDB_HNSW_NO_SPLIT=1), dict(MDB_HNSW_CLOSURE=0))


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def route_program(tmp_path_factory):
    return H.build_route_program(tmp_path_factory.mktemp("hnsw_route") / "route")


def _ring_graph(n, d, upper, seed):
    """layer 0: a ring with four random long links over n points; layer i >= 1 over the first upper[i - 1] points"""
    rng = np.random.default_rng(seed)
    v = rng.random((n, d), dtype=np.float32)
    ar = np.arange(n)
    nb = np.stack([(ar + 1) % n, (ar - 1) % n] + [rng.integers(0, n, n) for _ in range(4)], 1)
    layers = [(None, np.arange(n + 1, dtype=np.uint64) * 6, nb.reshape(-1).astype(np.uint32))] + [_ring_layer(rng, np.arange(m)) for m in upper]
    q = (v[rng.integers(0, n, 32)] + rng.normal(0, 0.02, (32, d))).astype(np.float32)
    return v, layers, q


def _f32_graph(oracle, ctx, n, d, upper, seed):
    from muopdb_amd.index import BlockBasedHnsw
    v, layers, q = _ring_graph(n, d, upper, seed)
    index, vf = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d), F.write_vector_file(v)
    return BlockBasedHnsw(ctx, index, vf, d), oracle.BlockBasedHnsw(index, vf, d), q


def _pq_graph(oracle, ctx, n, d, upper, seed):
    from muopdb_amd.index import BlockBasedHnsw, ProductQuantizer
    v, layers, q = _ring_graph(n, d, upper, seed)
    cb = H.train_pq_codebook(v[:1000], 8, 8, iters=2)
    codes = oracle.ProductQuantizer(d, 8, 8, cb, 0).quantize(v)
    index, vf = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d // 8), F.write_vector_file(codes)
    return (BlockBasedHnsw(ctx, index, vf, d, ProductQuantizer(d, 8, 8, cb, 0)),
            oracle.BlockBasedHnsw(index, vf, d, oracle.Quant(oracle.QUANT_PQ, 0, 8, 8, cb)), q)


# name -> (builder, n, d, points of layers 1.., what the shape line must say of the handle)
GRAPHS = {
    "three-layers": (_f32_graph, 2000, 128, (300, 40), dict(kind=0, dimension=128, max_n=2000, nu=300, nu2=40, layers=2, rows_nat=1, map21=1)),
    "two-layers": (_f32_graph, 2000, 128, (300,), dict(kind=0, dimension=128, max_n=2000, nu=300, nu2=0, layers=1, rows_nat=1)),
    "pq": (_pq_graph, 1200, 64, (200, 30), dict(kind=1, dimension=64, max_n=1200, pq_m=8, pq_K=256, pq_subdim=8, nu=0)),
    "no-larger-than-ef": (_f32_graph, 150, 128, (20,), dict(kind=0, dimension=128, max_n=150)),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_described_route_is_the_headers_and_the_search_is_the_oracles(ctx, oracle, route_program, name):
    build, n, d, upper, shape_says = GRAPHS[name]
    g, o, q = build(oracle, ctx, n, d, upper, seed=len(name))
    want = {}
    for b in BATCHES:
        for ef in EFS:
            o.stats()
            rows = o.ann_search(q[:b], 10, ef)
            want[b, ef] = (rows, o.stats())
    cases, described = [], []
    for opts in OPTION_SETS:
        with options(ctx, **opts):
            for (b, ef), (rows, counters) in want.items():
                shape, launches = g.describe_search(b, 10, ef)
                words = dict(w.split("=") for w in shape.split())
                assert {k: int(words[k]) for k in shape_says} == shape_says
                cases.append("%s b=%d k=10 ef=%d qstride=%d %s" % (shape, b, ef, (d + 3) // 4 * 4 + 16,
                                                                  " ".join("%s=%d" % (k[4:].lower(), v) for k, v in opts.items())))
                described.append(launches)
                ctx.stats()
                got = g.ann_search(q[:b], 10, ef)
                st = ctx.stats()
                assert_result_rows(got, rows, b)
                assert (st["distance_evals"], st["expanded_nodes"]) == tuple(counters), (b, ef, opts)
    g.close()
    from muopdb_amd.index import parse_route_line
    routes = H.run_route_program(route_program, cases)[0]
    for case, launches, (lines, _) in zip(cases, described, routes):
        assert launches == [parse_route_line(ln) for ln in lines], case
    # the forms these calls are chosen to reach
    roles = {tuple(role for role, *_ in launches) for launches in described}
    expect = {"three-layers": {("top", "layer1", "fallback", "layer0"), ("table", "layer1", "fallback", "layer0"), ("top", "layer1", "layer0"),
                               ("table", "layer1", "layer0"), ("table", "table", "layer1", "fallback", "layer0"), ("table", "table", "layer1", "layer0"),
                               ("layer0",)},
              "two-layers": {("table", "layer1", "fallback", "layer0"), ("table", "layer1", "layer0"), ("table", "table", "layer1", "fallback", "layer0"),
                             ("table", "table", "layer1", "layer0"), ("layer0",)},
              "pq": {("pq_quantize", "pq_rows", "layer0")},
              "no-larger-than-ef": {("closure",)}}[name]
    assert roles == expect, roles

"""The frontier form with theta as a bound and the counted stop test (muopdb_amd/csrc/mdb_hnsw_closure.hip.h) against the oracle
and against MDB_HNSW_CLOSURE=0 (-m gpu): rows, score bits, counts, distance_evals, expanded_nodes, and mdb_hnsw_closure_fallbacks
against the number of flagged queries tests/closure_bound_model.py gives.

The model runs on the oracle's distances as canonical images, with the bound the kernels take (closure_bound_model.theta_bound: the
select's two histogram passes restated) and their pop-list capacity, per phase as tests/test_gpu_hnsw_closure_local.py does: the
layers >= 2 on theta over the TOP set, layer 1 on theta over every upper point, each phase started from the sequential form's state.

Graphs (synth.bulk_hnsw, d = 128): 17 000 points at max_neighbors 8 (~2.1 k upper points, ~270 TOP points, >= 4 layers: theta is
finite at ef 16, 64 and 200 in both phases) and 36 000 points at max_neighbors 4 (> 8 x 1024 upper points: every thread of the
1024-thread layer-1 block holds several keys of the select and the last trip is not full; > 2048 TOP points: the top blocks leave their
flags to the follow-up launch).  A hand-built path graph forces more single pops on layer 1 than the pop list holds, and rows of
tie groups under a 30-bit key range put whole groups between the select's bound and theta.
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import closure_bound_model as BM
from tests import closure_model as CM
from tests import helpers as H

pytestmark = pytest.mark.gpu

D = 128
ERR_NAN = 5
POP_CAP = 256   # CL_POP_CAP


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


def _describe(x, layers, levels, q):
    levels = np.asarray(levels)
    nl = len(layers)
    small = nl   # the library's small_layer: the lowest of the top layers that hold <= 64 points each
    for layer in range(nl - 1, 0, -1):
        if int((levels >= layer).sum()) > 64:
            break
        small = layer
    return dict(x=x, layers=layers, q=q, index=F.write_hnsw_index(layers, np.arange(len(x), dtype=np.uint64), D),
                rows={l: CM.csr_rows(*layers[l]) for l in range(1, nl)}, small=small, entry=int(layers[nl - 1][0][0]),
                top=np.flatnonzero(levels >= 2), only1=np.flatnonzero(levels == 1), upper=np.flatnonzero(levels >= 1))


def _bulk(n, max_neighbors, seed):
    import torch
    from muopdb_amd import synth
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)).astype(np.float32)
    layers, levels = synth.bulk_hnsw(torch.from_numpy(x).cuda(), max_neighbors=max_neighbors, max_layers=8, kcand=64, seed=seed)
    return _describe(x, layers, levels, rng.standard_normal((64, D)).astype(np.float32))


@pytest.fixture(scope="module")
def graph():
    g = _bulk(17000, 8, 5)
    assert len(g["layers"]) >= 4 and 1900 <= len(g["upper"]) <= 2400 and 201 <= len(g["top"]) <= 447, (len(g["upper"]), len(g["top"]))
    return g


@pytest.fixture(scope="module")
def big_graph():
    g = _bulk(36000, 4, 6)
    assert len(g["layers"]) >= 4 and 8 * 1024 < len(g["upper"]) < 9 * 1024 and len(g["top"]) > 2048, (len(g["upper"]), len(g["top"]))
    return g


def _classify(oracle, graph, x, q, ef, metric=0):
    """per query: (flagged by a tie, flagged by the full pop list), in either phase; a NaN among the upper distances is not handled here"""
    out = []
    nl = len(graph["layers"])
    xu = np.ascontiguousarray(x[graph["upper"]])
    for qi in range(len(q)):
        keys = BM.images(np.asarray(oracle.distance_many(metric, q[qi], xu), dtype=np.float32))
        assert BM.NAN_KEY not in keys
        dist = dict(zip(graph["upper"].tolist(), keys))
        tb_top = BM.theta_bound([dist[int(p)] for p in graph["top"]], ef)
        tb_all = BM.theta_bound(keys, ef)
        ep, vis, tie, cap = graph["entry"], set(), False, False
        for layer in range(nl - 1, 0, -1):
            tb = None if (layer >= graph["small"] and ef >= 64) else tb_top if layer >= 2 else tb_all
            got, info = BM.closure_bound_layer(graph["rows"][layer], dist, ep, ef, vis, tb, POP_CAP)
            cap = cap or info.cap_hit
            tie = tie or (got.hazard and not info.cap_hit)
            ref = CM.search_layer(graph["rows"][layer], dist, ep, ef, vis)
            if not got.hazard:
                assert CM.same(ref, got)
            ep, vis = ref.nearest, ref.visited
        out.append((bool(tie), bool(cap)))
    return out


def _pair(ctx, oracle, index, vectors, metric=0):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    vf = F.write_vector_file(vectors)
    return (BlockBasedHnsw(ctx, index, vf, D, NoQuantizer(D, metric)),
            oracle.BlockBasedHnsw(index, vf, D, oracle.Quant(oracle.QUANT_NONE, metric)))


def _rows(res, b):
    return ([int(c) for c in res.counts[:b]],) + H.result_rows(res, b)


def _check(ctx, g, o, q, k, ef):
    """both switch positions against the oracle; -> queries the frontier form handed to the sequential form"""
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
    return out[1]


def _tie_rows(graph, seed):
    """integer rows in 0..3 on every upper point (the level >= 2 points and the level-1-only points drawn apart)"""
    rng = np.random.default_rng(seed)
    x = graph["x"].copy()
    x[graph["top"]] = rng.integers(0, 4, (len(graph["top"]), D)).astype(np.float32)
    x[graph["only1"]] = rng.integers(0, 4, (len(graph["only1"]), D)).astype(np.float32)
    # 64 queries, every 32 of them binary, in 0..3 and Gaussian ones: ties in either phase, both, none
    q1 = rng.integers(0, 2, (28, D)).astype(np.float32)
    q3 = rng.integers(0, 4, (28, D)).astype(np.float32)
    qf = graph["q"][:8]
    return x, np.concatenate([q1[14:], q3[:14], qf[:4], q1[:14], q3[14:], qf[4:]])


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_float_rows_flag_nobody(ctx, oracle, graph, ef):
    cls = _classify(oracle, graph, graph["x"], graph["q"], ef)
    assert not any(t or c for t, c in cls)
    g, o = _pair(ctx, oracle, graph["index"], graph["x"])
    for b in (64, 32, 31):
        assert _check(ctx, g, o, graph["q"][:b], 10, ef) == 0, (ef, b)


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_integer_rows_flag_many(ctx, oracle, graph, ef):
    x, q = _tie_rows(graph, 105)
    cls = _classify(oracle, graph, x, q, ef)
    assert not any(c for _, c in cls)
    g, o = _pair(ctx, oracle, graph["index"], x)
    for b in (64, 32, 31):
        want = sum(1 for t, _ in cls[:b] if t)
        print("ef %d batch %d: %d flagged" % (ef, b, want))
        assert 0 < want < b, "ef %d batch %d: the batch must hold flagged and clean queries (%d flagged)" % (ef, b, want)
        assert _check(ctx, g, o, q[:b], 10, ef) == want, (ef, b)


@pytest.mark.parametrize("rows", ["float", "integer"])
def test_more_upper_points_than_eight_per_thread(ctx, oracle, big_graph, rows):
    ef = 64
    x, q = (big_graph["x"], big_graph["q"]) if rows == "float" else _tie_rows(big_graph, 106)
    cls = _classify(oracle, big_graph, x, q, ef)
    want = [sum(1 for t, c in cls[:b] if t or c) for b in (64, 31)]
    assert (want[0] == 0) if rows == "float" else (0 < want[0] < 64), want
    g, o = _pair(ctx, oracle, big_graph["index"], x)
    for b, w in zip((64, 31), want):
        assert _check(ctx, g, o, q[:b], 10, ef) == w, (rows, b)


def test_keys_that_span_fewer_than_eight_bits(ctx, oracle, graph):
    """every upper point at (1000, e, 0, ...) with e in quarters, the queries at (-j, 0, ...): the upper row of a query is
    (1000 + j)^2 + e^2, five values inside 16 ulps — the select resolves it in one pass and the layers are all ties"""
    rng = np.random.default_rng(31)
    x = graph["x"].copy()
    x[graph["upper"]] = 0.0
    x[graph["upper"], 0] = 1000.0
    x[graph["upper"], 1] = rng.integers(0, 5, len(graph["upper"])).astype(np.float32) / 4
    q = np.zeros((64, D), np.float32)
    q[:, 0] = -(np.arange(64) % 24).astype(np.float32)
    xu = np.ascontiguousarray(x[graph["upper"]])
    for qi in (0, 23, 63):
        keys = BM.images(np.asarray(oracle.distance_many(0, q[qi], xu), dtype=np.float32))
        assert 0 < (max(keys) - min(keys)).bit_length() < 8
    g, o = _pair(ctx, oracle, graph["index"], x)
    for ef in (16, 200):
        cls = _classify(oracle, graph, x, q, ef)
        for b in (64, 31):
            want = sum(1 for t, c in cls[:b] if t or c)
            assert want > 0, "ef %d batch %d: rows of five values must flag" % (ef, b)
            assert _check(ctx, g, o, q[:b], 10, ef) == want, (ef, b)


def test_tie_groups_between_the_bound_and_theta(ctx, oracle, graph):
    """integer patterns on 32 coordinates of every upper point, all of them 300 away from the queries on another, and one point of
    either phase 1e18 away: the row is 90 000 + a small integer with long tie groups, its key range 30 bits, so the select leaves 8 bits
    open — a bin holds two neighbouring distances, and where theta is the upper one the whole tie group below it is demoted from the
    frontiers to single pops.  Every other query carries a little noise and has no exact ties."""
    rng = np.random.default_rng(41)
    x, up = graph["x"].copy(), graph["upper"]
    xu = np.zeros((len(up), D), np.float32)
    xu[:, 0] = 300.0
    xu[:, 1:33] = rng.integers(0, 4, (len(up), 32))
    x[up] = xu
    for p in (int(graph["top"][5]), int(graph["only1"][3])):
        x[p] = 0.0
        x[p, 1] = 1e18
    q = np.zeros((64, D), np.float32)
    q[:, 1:33] = rng.integers(0, 4, (64, 32))
    q[1::2, 1:33] += rng.standard_normal((32, 32)).astype(np.float32) * 0.05
    g, o = _pair(ctx, oracle, graph["index"], x)
    for ef in (16, 64):
        gap = []   # per query: points in [bound, theta) over every upper point, over the TOP set
        for qi in range(len(q)):
            n = []
            for pts in (up, graph["top"]):
                keys = BM.images(np.asarray(oracle.distance_many(0, q[qi], np.ascontiguousarray(x[pts])), dtype=np.float32))
                tb, th = BM.theta_bound(keys, ef), CM.theta_of(keys, ef)
                assert tb <= th and (max(keys) - min(keys)).bit_length() > 22
                n.append(sum(1 for v in keys if tb <= v < th))
            gap.append(tuple(n))
        cls = _classify(oracle, graph, x, q, ef)
        assert not any(c for _, c in cls)
        for b in (64, 32, 31):
            flagged = [t for t, _ in cls[:b]]
            # the class the case exists for: queries with points between the bound and theta, in either phase, flagged ones and clean ones
            assert any(a for a, _ in gap[:b]) and any(t for _, t in gap[:b]), (ef, b)
            assert any(f and (a or t) for f, (a, t) in zip(flagged, gap[:b])) and any(not f and (a or t) for f, (a, t) in zip(flagged, gap[:b])), (ef, b)
            assert _check(ctx, g, o, q[:b], 10, ef) == sum(flagged), (ef, b)


def test_keys_that_span_all_32_bits(ctx, oracle, graph):
    """dot-product distances of either sign: the images of a row span more than 2^31, the select's two passes leave 10 bits open"""
    xu = np.ascontiguousarray(graph["x"][graph["upper"]])
    keys = BM.images(np.asarray(oracle.distance_many(1, graph["q"][0], xu), dtype=np.float32))
    assert (max(keys) - min(keys)).bit_length() == 32
    g, o = _pair(ctx, oracle, graph["index"], graph["x"], metric=1)
    for ef in (16, 200):
        cls = _classify(oracle, graph, graph["x"], graph["q"], ef, metric=1)
        assert not any(t or c for t, c in cls)
        for b in (64, 31):
            assert _check(ctx, g, o, graph["q"][:b], 10, ef) == 0, (ef, b)


def test_ef_one_below_the_size_of_the_top_set(ctx, oracle, graph):
    """n = ef + 1: theta is the second largest image of the TOP set, all but two of its points are certain"""
    ef = len(graph["top"]) - 1
    for rows, (x, q) in (("float", (graph["x"], graph["q"])), ("integer", _tie_rows(graph, 107))):
        cls = _classify(oracle, graph, x, q, ef)
        g, o = _pair(ctx, oracle, graph["index"], x)
        for b in (64, 31):
            want = sum(1 for t, c in cls[:b] if t or c)
            assert (want == 0) if rows == "float" else (0 < want < b), (rows, b, want)   # clean on float rows, both classes on integer rows
            assert _check(ctx, g, o, q[:b], 10, ef) == want, (ef, b)


@pytest.mark.parametrize("where", ["top", "only1"])
def test_nan_in_an_upper_point(ctx, oracle, graph, where):
    """the NaN's key sorts last in the select (and widens the key range to 32 bits); a query that evaluates the point fails with
    MDB_ERR_NAN on both switch positions, the others return the oracle's rows"""
    from muopdb_amd import lib as L
    x = graph["x"].copy()
    x[int(graph[where][17]), 2] = np.nan
    g, o = _pair(ctx, oracle, graph["index"], x)
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
            with pytest.raises(L.MuopdbError) as e:
                g.ann_search(np.concatenate([np.resize(q[~hit], (39, D)), q[hit][:1]]), 10, ef)
            assert e.value.status == ERR_NAN
    for b in (40, 31):
        assert _check(ctx, g, o, np.resize(q[~hit], (b, D)), 10, ef) == 0


def _path_graph(n, n2, n3):
    """points 0 .. n-1 on a line, every one of them on layer 1, the first n2 on layer 2, the first n3 on layer 3; edges to the two neighbours"""
    def layer(count, points):
        indptr, edges = [0], []
        for i in range(count):
            edges += [j for j in (i - 1, i + 1) if 0 <= j < count]
            indptr.append(len(edges))
        return (np.arange(count, dtype=np.uint32) if points else None, np.asarray(indptr, np.uint64), np.asarray(edges, np.uint32))
    x = np.zeros((n, D), np.float32)
    x[:, 0] = np.arange(n)
    levels = np.zeros(n, np.int64) + 1
    levels[:n2] = 2
    levels[:n3] = 3
    return x, [layer(n, False), layer(n, True), layer(n2, True), layer(n3, True)], levels


def test_more_single_pops_than_the_list_holds(ctx, oracle):
    """a walk along a path towards the query: every point it meets is nearer than all before it and, outside the ef nearest, uncertain —
    one single pop per step.  Queries far down the path fill the list and come back through the sequential form, counted once each;
    queries near the entry point stay in the frontier form"""
    ef = 16
    x, layers, levels = _path_graph(700, 8, 2)
    at = np.asarray([20, 60, 120, 200, 330, 450, 560, 690] * 8, np.float32)
    q = np.zeros((64, D), np.float32)
    q[:, 0] = at + 0.25                                   # (no two points equally far)
    graph = _describe(x, layers, levels, q)
    cls = _classify(oracle, graph, x, q, ef)
    assert not any(t for t, _ in cls), "the path holds no ties"
    assert [c for _, c in cls[:8]] == [False, False, False, False, True, True, True, True], cls[:8]
    g, o = _pair(ctx, oracle, graph["index"], x)
    for b in (64, 32, 31):
        assert _check(ctx, g, o, q[:b], 10, ef) == sum(1 for _, c in cls[:b] if c), b

"""The fallback protocol of the frontier form (muopdb_amd/csrc/mdb_hnsw_closure.hip.h) phase by phase (-m gpu): a query flagged in the
top launch is re-run by the block that flagged it, a query flagged on layer 1 by a follow-up launch over layer 1 alone, and
mdb_hnsw_closure_fallbacks counts a query once wherever it was flagged.

The graph is the recipe of tests/test_gpu_hnsw_closure.py (20 000 x 32, synth.bulk_hnsw, max_neighbors 8: layer 1 ~2 500 points,
layer 2 ~300 = the TOP set of the split path); the cases keep its topology and overwrite the vector file.  Every search is compared
with the oracle (rows, score bits, counts, distance_evals, expanded_nodes) on both positions of MDB_HNSW_CLOSURE, and the fallback
count with tests/closure_model.py, which classifies every query per phase over the oracle's distances: theta over the TOP set for
the layers >= 2, over every upper point for layer 1, +inf for the tiny top layers at ef >= 64 — what the launches do.

A layer evaluates the points it discovers that no layer above has visited, and a flag needs ef + 1 evaluated points, so on this graph
(layer 2: 334 points, 332 with an in-edge, 37 of them on layer 3) the top phase cannot flag at ef >= ~297: at ef 300 the test asserts
exactly that from the model and asks for the other two classes only.
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import closure_model as CM
from tests import helpers as H

pytestmark = pytest.mark.gpu

N, D, SEED = 20000, 32, 5
ERR_NAN = 5


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
    levels = np.asarray(levels)
    nl = len(layers)
    # the library's small_layer: the lowest of the top layers that hold <= 64 points each (their edges stay inside them)
    small = nl
    for layer in range(nl - 1, 0, -1):
        if int((levels >= layer).sum()) > 64:
            break
        small = layer
    return dict(x=x, layers=layers, levels=levels, q=q, index=F.write_hnsw_index(layers, np.arange(N, dtype=np.uint64), D),
                rows={l: CM.csr_rows(*layers[l]) for l in range(1, nl)}, small=small, entry=int(layers[nl - 1][0][0]),
                top=np.flatnonzero(levels >= 2), only1=np.flatnonzero(levels == 1), upper=np.flatnonzero(levels >= 1))


def _classify(oracle, graph, x, q, ef, metric=0):
    """per query: (flagged on a layer >= 2, flagged on layer 1), each phase started from the sequential form's state above it"""
    out = []
    nl = len(graph["layers"])
    xu = np.ascontiguousarray(x[graph["upper"]])
    for qi in range(len(q)):
        dist = dict(zip(graph["upper"].tolist(), (float(v) for v in oracle.distance_many(metric, q[qi], xu))))
        assert not any(v != v for v in dist.values())
        th_top = CM.theta_of([dist[int(p)] for p in graph["top"]], ef)
        th_all = CM.theta_of(list(dist.values()), ef)
        ep, vis, top = graph["entry"], set(), False
        for layer in range(nl - 1, 1, -1):
            th = None if (layer >= graph["small"] and ef >= 64) else th_top
            top = top or CM.closure_layer(graph["rows"][layer], dist, ep, ef, vis, th).hazard
            ref = CM.search_layer(graph["rows"][layer], dist, ep, ef, vis)
            ep, vis = ref.nearest, ref.visited
        th = None if (1 >= graph["small"] and ef >= 64) else th_all
        out.append((bool(top), bool(CM.closure_layer(graph["rows"][1], dist, ep, ef, vis, th).hazard)))
    return out


def _pair(ctx, oracle, index, vectors, metric=0):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    vf = F.write_vector_file(vectors)
    return (BlockBasedHnsw(ctx, index, vf, D, NoQuantizer(D, metric)),
            oracle.BlockBasedHnsw(index, vf, D, oracle.Quant(oracle.QUANT_NONE, metric)))


def _rows(res, b):
    return ([int(c) for c in res.counts[:b]],) + H.result_rows(res, b)


def _check(ctx, g, o, q, k, ef, rank=None):
    """both switch positions against the oracle; -> queries the frontier form handed to the sequential form"""
    b = len(q)
    o.stats()
    want = o.ann_search(q, k, ef)
    evals, expanded = o.stats()
    out = {}
    for closure in (1, 0):
        with ctx.option("MDB_HNSW_CLOSURE", closure):
            if rank is None:
                got = g.ann_search(q, k, ef)
            else:
                with ctx.option("MDB_HNSW_RANK", rank):
                    got = g.ann_search(q, k, ef)
            st = ctx.stats()
            fb = ctx.closure_fallbacks()
        assert _rows(got, b) == _rows(want, b), (closure, rank, ef, b)
        assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (closure, rank, ef, b)
        out[closure] = fb
    assert out[0] == 0
    return out[1]


def _tie_rows(graph, seed=SEED + 100):
    """integer rows in 0..3 on every upper point (the level >= 2 points and the level-1-only points drawn apart)"""
    rng = np.random.default_rng(seed)
    x = graph["x"].copy()
    x[graph["top"]] = rng.integers(0, 4, (len(graph["top"]), D)).astype(np.float32)
    x[graph["only1"]] = rng.integers(0, 4, (len(graph["only1"]), D)).astype(np.float32)
    return x, rng


def _mixed_queries(graph):
    """64 queries, every 32 of them 14 binary, 14 in 0..3 and 4 Gaussian ones: ties with the integer rows in either phase, both, none"""
    x, rng = _tie_rows(graph)
    q1 = rng.integers(0, 2, (28, D)).astype(np.float32)
    q3 = rng.integers(0, 4, (28, D)).astype(np.float32)
    qf = graph["q"][:8]
    return x, np.concatenate([q1[14:], q3[:14], qf[:4], q1[:14], q3[14:], qf[4:]])   # (the two top-only queries at ef 200: in the first 32)


def _top_evaluable(graph, ef):
    """the most points layer 2 can evaluate, whatever the query: its entry point and the targets of its edges that the layers above
    have not visited.  At ef >= 64 the tiny layers above are closed whole (small_layer), so layer 3 visits everything its entry point
    reaches: the bound takes the layer-3 entry point that leaves most"""
    lay2, lay3 = graph["rows"][2], graph["rows"].get(3, {})
    targets = set(e for r in lay2.values() for e in r)
    if not (ef >= 64 and graph["small"] <= 3 and lay3):
        return len(targets) + 1
    most = 0
    for ep in lay3:
        reach, todo = {ep}, [ep]
        while todo:
            for e in lay3.get(todo.pop(), ()):
                if e not in reach:
                    reach.add(e)
                    todo.append(e)
        most = max(most, len(targets - reach) + 1)
    return most


@pytest.mark.parametrize("ef", [16, 64, 200, 300])
def test_flag_in_either_phase_both_or_none(ctx, oracle, graph, ef):
    x, q = _mixed_queries(graph)
    cls = _classify(oracle, graph, x, q, ef)
    top_can_flag = _top_evaluable(graph, ef) > ef
    assert top_can_flag == (ef < 300)
    for b in (32, 64):
        have = set(cls[:b])
        print("ef %d batch %d: top only %d, layer 1 only %d, both %d, neither %d" % (
            ef, b, cls[:b].count((True, False)), cls[:b].count((False, True)), cls[:b].count((True, True)), cls[:b].count((False, False))))
        if top_can_flag:
            assert have == {(True, False), (False, True), (True, True), (False, False)}, (ef, b, have)
        else:
            assert have == {(False, True), (False, False)}, (ef, b, have)
    g, o = _pair(ctx, oracle, graph["index"], x)
    # the default (flags resolved where they are raised), the from-the-top protocol (MDB_HNSW_RANK 0: no sorted-position top block;
    # batch 31: one launch over every upper layer) and the sorted-position follow-up launch (MDB_HNSW_RANK 3)
    for b, rank in ((32, None), (64, None), (32, 0), (64, 0), (32, 3), (64, 3), (31, None)):
        want = sum(1 for t, l in cls[:b] if t or l)
        assert _check(ctx, g, o, q[:b], 10, ef, rank) == want, (ef, b, rank)


def test_no_word_of_a_flagged_batch_survives_into_the_next(ctx, oracle, graph):
    ef = 64
    x, rng = _tie_rows(graph)
    pool = rng.integers(0, 4, (96, D)).astype(np.float32)
    cls = _classify(oracle, graph, x, pool, ef)
    flagged = pool[[i for i, c in enumerate(cls) if c[0] or c[1]]][:64]
    assert len(flagged) == 64 and sum(1 for c in cls if c[0]) >= 16
    clean = graph["q"]
    assert not any(t or l for t, l in _classify(oracle, graph, x, clean, ef))
    g, o = _pair(ctx, oracle, graph["index"], x)
    for fb_b, clean_b in ((64, 64), (64, 32), (31, 64), (32, 31)):
        assert _check(ctx, g, o, clean[:clean_b], 10, ef) == 0
        assert _check(ctx, g, o, flagged[:fb_b], 10, ef) == fb_b
        assert _check(ctx, g, o, clean[:clean_b], 10, ef) == 0
        assert _check(ctx, g, o, flagged[:fb_b], 10, ef) == fb_b


@pytest.mark.parametrize("where", ["top", "only1"])
def test_nan_in_either_phase(ctx, oracle, graph, where):
    """a batch of 40 with a query that evaluates the planted point fails with MDB_ERR_NAN on both switch positions (the top block's own
    re-run hands the NaN word down; the follow-up launch over layer 1 raises the flag); queries that never reach it return the oracle's rows"""
    from muopdb_amd import lib as L
    x = graph["x"].copy()
    p = int(graph[where][17])
    x[p, 2] = np.nan
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
            for qs in (np.resize(q[hit], (40, D)), np.concatenate([np.resize(q[~hit], (39, D)), q[hit][:1]])):
                with pytest.raises(L.MuopdbError) as e:
                    g.ann_search(qs, 10, ef)
                assert e.value.status == ERR_NAN
    assert _check(ctx, g, o, np.resize(q[~hit], (40, D)), 10, ef) == 0


@pytest.mark.parametrize("ef", [8, 9])
def test_a_tie_group_as_long_as_ef(ctx, oracle, graph, ef):
    """eight copies of a query among the level >= 2 points and eight among the level-1-only points (its nearest ones, so that the
    traversal meets them): exact zeros tied with each other, a group that ends at the stop test of the top phase and straddles layer 1's"""
    x = graph["x"].copy()
    q = graph["q"].copy()
    for qi in (0, 1, 40):
        for where in ("top", "only1"):
            pts = graph[where]
            near = pts[np.argsort(((graph["x"][pts] - q[qi]) ** 2).sum(1), kind="stable")[:8]]
            x[near] = q[qi]
    cls = _classify(oracle, graph, x, q, ef)
    print("ef %d: flagged (top, layer 1) of the planted queries: %s" % (ef, [cls[i] for i in (0, 1, 40)]))
    g, o = _pair(ctx, oracle, graph["index"], x)
    for b in (31, 32, 64):
        assert _check(ctx, g, o, q[:b], 10, ef) == sum(1 for t, l in cls[:b] if t or l), (ef, b)

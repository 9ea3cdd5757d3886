"""The frontier form's theta over the points not yet visited, selected late and reused downwards (muopdb_amd/csrc/mdb_hnsw_closure.hip.h)
against the oracle and against MDB_HNSW_CLOSURE=0 (-m gpu): rows, score bits, counts, distance_evals, expanded_nodes, and
mdb_hnsw_closure_fallbacks against the number of flagged queries tests/closure_visited_model.py gives.

The model chains the upper layers of every query the way the launches do — the layers >= 2 select over the TOP set, layer 1 over every
upper point, each select behind the entry of the first layer that uses it and skipping what the layers above visited; the tiny top
layers are certain as a whole at ef >= 64 — on canonical images with cl_theta's two histogram passes, is held against
closure_model.search_layer layer by layer, and says which classes a case contains; every case asserts that the ones it exists for occur:
  below_row_theta   points visited on entry that lie below the theta of the whole set (each of them cost the old select a rank)
  fewer_pops        fewer single pops than under the theta of the whole set
  reused            a layer that ran under a select taken at a layer above
  inf_by_pool       a set of more than ef points whose unvisited rest is <= ef - 1: theta = +inf by the first pass's grand total
Shapes: ~2.1 k upper / ~270 TOP points (synth.bulk_hnsw, the recipe of tests/test_gpu_hnsw_closure_bound.py), d = 128, at ef 16 / 64 /
200 and batches 64, 32 and 31 (31: one launch over every upper layer, the TOP set through its map); five layers of exact sizes with
two TOP layers larger than ef under one select; a TOP set of ef + 1 points of which two are visited on entry; a NaN in an upper point.
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import closure_bound_model as BM
from tests import closure_model as CM
from tests import closure_visited_model as VM
from tests import helpers as H

pytestmark = pytest.mark.gpu

POP_CAP = 256   # CL_POP_CAP
ERR_NAN = 5
D = 128


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
    layers, levels = synth.bulk_hnsw(torch.from_numpy(x), max_neighbors=max_neighbors, max_layers=8, kcand=64, seed=seed)
    return _describe(x, layers, levels, rng.standard_normal((64, D)).astype(np.float32))


def _leveled(n, sizes, max_neighbors, seed, nq=64):
    """a graph whose layers 1, 2, ... hold exactly sizes[0] > sizes[1] > ... points (drawn at random among the n), synth's layer graphs"""
    import torch
    from muopdb_amd import synth
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, D)).astype(np.float32)
    order = rng.permutation(n)
    levels = np.zeros(n, np.int64)
    for layer, size in enumerate(sizes, 1):
        levels[order[:size]] = layer
    xt, lv = torch.from_numpy(x), torch.from_numpy(levels)
    layers = []
    for layer in range(len(sizes) + 1):
        ids = torch.nonzero(lv >= layer, as_tuple=False).reshape(-1)
        indptr, edges = synth._layer_graph(xt, ids, max_neighbors, min(64, len(ids) - 1))
        layers.append((None if layer == 0 else ids.cpu().numpy().astype(np.uint32), indptr, edges))
    return _describe(x, layers, levels, rng.standard_normal((nq, D)).astype(np.float32))


def _classify(oracle, graph, x, q, ef):
    """per query: flagged on any upper layer (a tie or the full pop list); and the classes seen over all of them"""
    seen = dict(below_row_theta=0, pops=0, pops_row_theta=0, reused=0, inf_by_pool=0, selects=0)
    nl = len(graph["layers"])
    layers = [(l, graph["rows"][l]) for l in range(nl - 1, 0, -1)]
    members = {"top": [int(p) for p in graph["top"]], "all": [int(p) for p in graph["upper"]]}
    set_of = {l: ("all" if l == 1 else "top") for l in range(1, nl)}
    all_certain = {l for l in range(1, nl) if l >= graph["small"] and ef >= 64}
    xu = np.ascontiguousarray(x[graph["upper"]])
    out = []
    for qi in range(len(q)):
        keys = BM.images(np.asarray(oracle.distance_many(0, q[qi], xu), dtype=np.float32))
        assert BM.NAN_KEY not in keys
        dist = dict(zip(members["all"], keys))
        runs = VM.chain(layers, dist, graph["entry"], ef, set_of, members, all_certain, select=VM.select_rest_hist, pop_cap=POP_CAP)
        flagged = False
        for r, (layer, rows) in zip(runs, layers):
            ref = CM.search_layer(rows, dist, r.ep, ef, r.visited_in)
            if not r.state.hazard:
                assert CM.same(ref, r.state), (qi, layer)
            flagged = flagged or r.state.hazard
            seen["pops"] += r.state.pops
            seen["selects"] += r.selected
            if layer in all_certain:
                continue
            seen["reused"] += not r.selected
            row_tb = BM.theta_bound([dist[p] for p in members[set_of[layer]]], ef)
            old, oinfo = BM.closure_bound_layer(rows, dist, r.ep, ef, r.visited_in, row_tb, POP_CAP)
            assert old.hazard == r.state.hazard or r.info.cap_hit or oinfo.cap_hit, (qi, layer)
            seen["pops_row_theta"] += old.pops
            if row_tb is not None:
                seen["below_row_theta"] += sum(1 for p in r.visited_in if p != r.ep and dist[p] < row_tb)
            seen["inf_by_pool"] += r.selected and r.theta is None and len(members[set_of[layer]]) > ef
        out.append(bool(flagged))
    return out, seen


def _pair(ctx, oracle, graph, vectors):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    vf = F.write_vector_file(vectors)
    return (BlockBasedHnsw(ctx, graph["index"], vf, D, NoQuantizer(D, 0)),
            oracle.BlockBasedHnsw(graph["index"], vf, D, oracle.Quant(oracle.QUANT_NONE, 0)))


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


def _tie_rows(graph, seed, hi=4):
    """integer rows in 0..hi-1 on every upper point (the level >= 2 points and the level-1-only points drawn apart); 64 queries, every
    32 of them binary, in 0..3 and Gaussian ones: ties in either phase, both, none"""
    rng = np.random.default_rng(seed)
    x = graph["x"].copy()
    x[graph["top"]] = rng.integers(0, hi, (len(graph["top"]), D)).astype(np.float32)
    x[graph["only1"]] = rng.integers(0, hi, (len(graph["only1"]), D)).astype(np.float32)
    q1 = rng.integers(0, 2, (28, D)).astype(np.float32)
    q3 = rng.integers(0, 4, (28, D)).astype(np.float32)
    qf = graph["q"][:8]
    return x, np.concatenate([q1[14:], q3[:14], qf[:4], q1[:14], q3[14:], qf[4:]])


@pytest.fixture(scope="module")
def graph():
    g = _bulk(17000, 8, 5)
    assert len(g["layers"]) >= 4 and 1900 <= len(g["upper"]) <= 2400 and 201 <= len(g["top"]) <= 447, (len(g["upper"]), len(g["top"]))
    return g


@pytest.fixture(scope="module")
def classified(oracle, graph):
    """the model's verdicts, computed once per (rows, ef) and shared by the batch sizes"""
    cache = {}

    def get(rows, ef):
        if (rows, ef) not in cache:
            x, q = (graph["x"], graph["q"]) if rows == "float" else _tie_rows(graph, 105)
            cache[rows, ef] = (x, q) + _classify(oracle, graph, x, q, ef)
        return cache[rows, ef]
    return get


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_float_rows(ctx, oracle, graph, classified, ef):
    x, q, cls, seen = classified("float", ef)
    print("ef %d: %s" % (ef, seen))
    assert not any(cls)
    assert seen["below_row_theta"] > 0, (ef, seen)
    if ef >= 64:   # (at ef 16 the layers above leave a point or two below theta, and the entry point left out costs as much)
        assert seen["pops"] < seen["pops_row_theta"], (ef, seen)
    g, o = _pair(ctx, oracle, graph, x)
    for b in (64, 32, 31):
        assert _check(ctx, g, o, q[:b], 10, ef) == 0, (ef, b)


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_integer_rows(ctx, oracle, graph, classified, ef):
    x, q, cls, seen = classified("integer", ef)
    print("ef %d: %d flagged, %s" % (ef, sum(cls), seen))
    assert seen["below_row_theta"] > 0, (ef, seen)
    g, o = _pair(ctx, oracle, graph, x)
    for b in (64, 32, 31):
        want = sum(cls[:b])
        assert 0 < want < b, (ef, b, want)
        assert _check(ctx, g, o, q[:b], 10, ef) == want, (ef, b)


@pytest.mark.parametrize("ef", [16, 64])
def test_one_select_serves_two_top_layers(ctx, oracle, ef):
    """layers of 2 200 / 700 / 260 / 40 points: at ef 64 the top layer is certain as a whole and the select runs at layer 3, behind
    its visits, for layers 3 and 2; at ef 16 it runs at layer 4 for all three"""
    g5 = _leveled(5000, (2200, 700, 260, 40), 8, 11)
    assert len(g5["layers"]) == 5 and g5["small"] == 4
    for rows in ("float", "integer"):
        x, q = (g5["x"], g5["q"]) if rows == "float" else _tie_rows(g5, 111, hi=3)
        cls, seen = _classify(oracle, g5, x, q, ef)
        print("ef %d, %s rows: %d flagged, %s" % (ef, rows, sum(cls), seen))
        assert seen["selects"] == 2 * len(q) and seen["reused"] == (1 if ef >= 64 else 2) * len(q), seen
        assert seen["below_row_theta"] > 0, seen
        g, o = _pair(ctx, oracle, g5, x)
        for b in (64, 31):
            assert _check(ctx, g, o, q[:b], 10, ef) == sum(cls[:b]), (rows, b)


def test_a_top_set_of_ef_plus_one_points_with_two_visited_on_entry(ctx, oracle):
    """layer 3 holds two points linked to each other and is closed whole (ef >= 64): both are visited when layer 2 — ef + 1 points, the
    TOP set — is entered.  ef - 1 unvisited points are a pool of ef: theta = +inf, by the first pass's grand total"""
    ef = 64
    g4 = _leveled(5000, (2200, ef + 1, 2), 8, 13)
    assert len(g4["layers"]) == 4 and g4["small"] == 3 and len(g4["top"]) == ef + 1
    assert all(len(r) == 1 for r in g4["rows"][3].values())
    for rows in ("float", "integer"):
        x, q = (g4["x"], g4["q"]) if rows == "float" else _tie_rows(g4, 113)
        cls, seen = _classify(oracle, g4, x, q, ef)
        print("%s rows: %d flagged, %s" % (rows, sum(cls), seen))
        assert seen["inf_by_pool"] == len(q), seen
        g, o = _pair(ctx, oracle, g4, x)
        for b in (64, 31):
            assert _check(ctx, g, o, q[:b], 10, ef) == sum(cls[:b]), (rows, b)


@pytest.mark.parametrize("where", ["top", "only1"])
def test_nan_in_an_upper_point(ctx, oracle, graph, where):
    """a batch with a query that evaluates the planted point fails with MDB_ERR_NAN on both switch positions (the selects skip no NaN
    of an unvisited point: it sorts last); queries that never reach it return the oracle's rows"""
    from muopdb_amd import lib as L
    x = graph["x"].copy()
    x[int(graph[where][17]), 2] = np.nan
    g, o = _pair(ctx, oracle, graph, x)
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
            for qs in (np.resize(q[hit], (40, D)), np.concatenate([np.resize(q[~hit], (30, D)), q[hit][:1]])):
                with pytest.raises(L.MuopdbError) as e:
                    g.ann_search(qs, 10, ef)
                assert e.value.status == ERR_NAN
    assert _check(ctx, g, o, np.resize(q[~hit], (40, D)), 10, ef) == 0

"""The single pop's incremental pass of the frontier form (muopdb_amd/csrc/mdb_hnsw_closure.hip.h) against the oracle and against
MDB_HNSW_CLOSURE=0 (-m gpu): rows, score bits, counts, distance_evals, expanded_nodes, and mdb_hnsw_closure_fallbacks against the number
of flagged queries the models give.

tests/closure_incremental_model.py runs every phase of every query the way the launches do — the layers >= 2 by 256 threads over the TOP
set in its own numbering (the points in id order), layer 1 by 1024 threads over every upper point; a batch below 32 is one launch of
1024 threads over every upper layer — from the sequential form's state above it, is held against tests/closure_bound_model.py, and
says which classes of the bookkeeping a case contains; every case asserts that the classes it exists for occur:
  one_slice        two consecutive single pops in one thread's slice of the bitmap (the owner forgot the slice and walked it again)
  ties_in_slice    pending ties of u inside u's slice;  ties_elsewhere: in other threads' slices
  nearer           the pop's expansion evaluated the next u (the new minimum comes from new bits only)
  nothing_new      a pop that evaluated nothing;  only_certain: a pop after which only certain points were found
  found_in_round   an uncertain point first evaluated in a round (by a lane of whichever thread expands its discoverer), not by the pop
  left_pending     a layer that ends by lt >= ef with pending points left;  stale_differs: the layer below returns something else when
                   the threads' values of that layer are left in place (the model's `threads` hook)
Shapes: ~2.1 k upper / ~270 TOP points (synth.bulk_hnsw, the recipe of tests/test_gpu_hnsw_closure_bound.py) at ef 16 / 64 / 200 and
batches 64, 32 and 31; five layers with exact sizes for the top phase of three layers; and the bitmap sizes at which ownership changes
— words << ltpw just below the block size, equal to it and just above it (every thread walks several slices: the full walk) — for the
256-thread top block (TOP sets of 8 000 / 8 100 / 8 200 points: 252 / 256 / 260 words) and the 1024-thread block (32 600 / 32 700 /
32 800 upper points: 1020 / 1024 / 1028 words).
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import closure_bound_model as BM
from tests import closure_incremental_model as IM
from tests import closure_model as CM
from tests import helpers as H

pytestmark = pytest.mark.gpu

POP_CAP = 256   # CL_POP_CAP
CLASSES = ("one_slice", "ties_in_slice", "ties_elsewhere", "nearer", "nothing_new", "only_certain", "found_in_round", "left_pending",
           "stale_differs")


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
    d = x.shape[1]
    return dict(x=x, d=d, layers=layers, q=q, index=F.write_hnsw_index(layers, np.arange(len(x), dtype=np.uint64), d),
                rows={l: CM.csr_rows(*layers[l]) for l in range(1, nl)}, small=small, entry=int(layers[nl - 1][0][0]),
                top=np.flatnonzero(levels >= 2), only1=np.flatnonzero(levels == 1), upper=np.flatnonzero(levels >= 1))


def _bulk(n, d, max_neighbors, seed):
    import torch
    from muopdb_amd import synth
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    # (built on the host: the classes the cases assert were counted on this very graph)
    layers, levels = synth.bulk_hnsw(torch.from_numpy(x), max_neighbors=max_neighbors, max_layers=8, kcand=64, seed=seed)
    return _describe(x, layers, levels, rng.standard_normal((64, d)).astype(np.float32))


def _leveled(n, d, sizes, max_neighbors, seed, nq=64, device="cpu"):
    """a graph whose layers 1, 2, ... hold exactly sizes[0] > sizes[1] > ... points (drawn at random among the n), synth's layer graphs"""
    import torch
    from muopdb_amd import synth
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    order = rng.permutation(n)
    levels = np.zeros(n, np.int64)
    for layer, size in enumerate(sizes, 1):
        levels[order[:size]] = layer
    xt, lv = torch.from_numpy(x).to(device), torch.from_numpy(levels).to(device)
    layers = []
    for layer in range(len(sizes) + 1):
        ids = torch.nonzero(lv >= layer, as_tuple=False).reshape(-1)
        indptr, edges = synth._layer_graph(xt, ids, max_neighbors, 64)
        layers.append((None if layer == 0 else ids.cpu().numpy().astype(np.uint32), indptr, edges))
    return _describe(x, layers, levels, rng.standard_normal((nq, d)).astype(np.float32))


def _local(rows, pts):
    """a layer's rows in the numbering of the launch that runs it: position in `pts` (ascending ids)"""
    pos = {int(p): i for i, p in enumerate(pts)}
    return {pos[p]: [pos[e] for e in r] for p, r in rows.items()}, pos


def _words(n):
    return (n // 32 + 4) & ~3   # the library's bitmap over n points


def _layer_classes(seen, trace, rows, dist, tb, nt, n):
    _, ltpw, _, own_one = IM.slices(n, nt, _words(n))
    if not own_one:
        return
    slice_of = lambda p: (p >> 5 << ltpw) + ((p & 31) >> (5 - ltpw))
    for prev, pop in zip(trace, trace[1:]):
        u, pu = pop["u"], prev["u"]
        pend = pop["evaluated"] - pop["expanded"]
        ties = [p for p in pend if p != u and dist[p] == dist[u]]
        new = pop["evaluated"] - prev["evaluated"]
        seen["one_slice"] += slice_of(pu) == slice_of(u)
        seen["ties_in_slice"] += any(slice_of(p) == slice_of(u) for p in ties)
        seen["ties_elsewhere"] += any(slice_of(p) != slice_of(u) for p in ties)
        seen["nearer"] += u in new
        seen["nothing_new"] += not new
        seen["only_certain"] += bool(new) and all(tb is None or dist[p] < tb for p in new)
        seen["found_in_round"] += any(not (tb is None or dist[p] < tb) for p in new - set(rows.get(pu, ())))
    if trace and trace[-1]["lt"] >= trace[-1]["ef"] and trace[-1]["evaluated"] - trace[-1]["expanded"]:
        seen["left_pending"] += 1


def _classify(oracle, graph, x, q, ef, single, classes=True, stale=False):
    """per query: flagged by a tie, flagged by the full pop list (in either phase); and the classes seen over all of them.
    single: one launch of 1024 threads over every upper layer (a batch below 32), else the split path's two launches"""
    out, seen = [], dict.fromkeys(CLASSES, 0)
    nl = len(graph["layers"])
    xu = np.ascontiguousarray(x[graph["upper"]])
    loc = {}
    for layer in range(1, nl):
        pts = graph["upper"] if (single or layer == 1) else graph["top"]
        loc[layer] = _local(graph["rows"][layer], pts) + (pts, 1024 if (single or layer == 1) else 256)
    for qi in range(len(q)):
        keys = BM.images(np.asarray(oracle.distance_many(0, q[qi], xu), dtype=np.float32))
        assert BM.NAN_KEY not in keys
        dist = dict(zip(graph["upper"].tolist(), keys))
        tb_top = BM.theta_bound([dist[int(p)] for p in graph["top"]], ef)
        tb_all = BM.theta_bound(keys, ef)
        ep, vis, tie, cap, kept = graph["entry"], set(), False, False, {}
        for layer in range(nl - 1, 0, -1):
            tb = None if (layer >= graph["small"] and ef >= 64) else tb_top if layer >= 2 else tb_all
            want, winfo = BM.closure_bound_layer(graph["rows"][layer], dist, ep, ef, vis, tb, POP_CAP)
            if classes:
                rows, pos, pts, nt = loc[layer]
                ldist = [dist[int(p)] for p in pts]
                lvis = set(pos[p] for p in vis if p in pos)
                trace = []
                got, ginfo = IM.closure_incremental_layer(rows, ldist, pos[ep], ef, lvis, tb, nt, POP_CAP, trace, None, _words(len(pts)))
                assert (got.hazard, got.evals, got.expanded, got.pops, ginfo) == (want.hazard, want.evals, want.expanded, want.pops, winfo)
                assert set(int(pts[p]) for p in got.visited - lvis) == want.visited - vis and int(pts[got.nearest]) == want.nearest
                for t in trace:
                    t["ef"] = ef
                _layer_classes(seen, trace, rows, ldist, tb, nt, len(pts))
            if classes and stale:
                # the same launch's threads, had their values survived the layer above
                th = kept.setdefault(nt, IM.new_threads(nt))
                old, _ = IM.closure_incremental_layer(rows, ldist, pos[ep], ef, lvis, tb, nt, POP_CAP, None, th, _words(len(pts)))
                seen["stale_differs"] += (old.hazard, old.evals, old.expanded, old.nearest) != (got.hazard, got.evals, got.expanded, got.nearest)
            cap = cap or winfo.cap_hit
            tie = tie or (want.hazard and not winfo.cap_hit)
            ref = CM.search_layer(graph["rows"][layer], dist, ep, ef, vis)
            if not want.hazard:
                assert CM.same(ref, want)
            ep, vis = ref.nearest, ref.visited
        out.append(bool(tie or cap))
    return out, seen


def _pair(ctx, oracle, graph, vectors):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    vf = F.write_vector_file(vectors)
    d = graph["d"]
    return (BlockBasedHnsw(ctx, graph["index"], vf, d, NoQuantizer(d, 0)),
            oracle.BlockBasedHnsw(graph["index"], vf, d, oracle.Quant(oracle.QUANT_NONE, 0)))


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
    x, d = graph["x"].copy(), graph["d"]
    x[graph["top"]] = rng.integers(0, hi, (len(graph["top"]), d)).astype(np.float32)
    x[graph["only1"]] = rng.integers(0, hi, (len(graph["only1"]), d)).astype(np.float32)
    q1 = rng.integers(0, 2, (28, d)).astype(np.float32)
    q3 = rng.integers(0, 4, (28, d)).astype(np.float32)
    qf = graph["q"][:8]
    return x, np.concatenate([q1[14:], q3[:14], qf[:4], q1[:14], q3[14:], qf[4:]])


@pytest.fixture(scope="module")
def graph():
    g = _bulk(17000, 128, 8, 5)
    assert len(g["layers"]) >= 4 and 1900 <= len(g["upper"]) <= 2400 and 201 <= len(g["top"]) <= 447, (len(g["upper"]), len(g["top"]))
    return g


@pytest.fixture(scope="module")
def classified(oracle, graph):
    """the models' verdicts, computed once per (rows, ef, launch form) and shared"""
    cache = {}

    def get(rows, ef, single):
        key = (rows, ef, single)
        if key not in cache:
            x, q = (graph["x"], graph["q"]) if rows == "float" else _tie_rows(graph, 105)
            cache[key] = (x, q) + _classify(oracle, graph, x, q, ef, single)
        return cache[key]
    return get


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_float_rows(ctx, oracle, graph, classified, ef):
    """no ties: nobody is flagged; the pops of a layer fall into one slice, find nearer points, nothing, or certain points only"""
    g, o = _pair(ctx, oracle, graph, graph["x"])
    for b, single in ((64, False), (32, False), (31, True)):
        x, q, cls, seen = classified("float", ef, single)
        print("ef %d batch %d: %s" % (ef, b, seen))
        assert not any(cls)
        if ef < 200:   # (at ef 200 the TOP set of ~270 is nearly all certain and layer 1 pops a handful of points)
            assert min(seen[c] for c in ("one_slice", "nearer", "only_certain", "found_in_round", "left_pending")) > 0, (ef, b, seen)
        assert _check(ctx, g, o, q[:b], 10, ef) == 0, (ef, b)


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_integer_rows(ctx, oracle, graph, classified, ef):
    """ties everywhere: ties of u in its own slice, in other threads' slices, pops that evaluate nothing; flagged and clean queries"""
    for b, single in ((64, False), (32, False), (31, True)):
        x, q, cls, seen = classified("integer", ef, single)
        g, o = _pair(ctx, oracle, graph, x)
        want = sum(cls[:b])
        print("ef %d batch %d: %d flagged, %s" % (ef, b, want, seen))
        assert 0 < want < b, (ef, b, want)
        assert min(seen[c] for c in ("ties_in_slice", "ties_elsewhere", "nothing_new", "one_slice")) > 0, (ef, b, seen)
        assert _check(ctx, g, o, q[:b], 10, ef) == want, (ef, b)


def test_flagged_and_clean_alternate_then_the_reverse_batch(ctx, oracle, graph, classified):
    ef = 64
    x, q, cls, _ = classified("integer", ef, False)
    flagged, clean = [i for i, c in enumerate(cls) if c], [i for i, c in enumerate(cls) if not c]
    n = min(len(flagged), len(clean), 32)
    assert n >= 8
    order = [i for pair in zip(flagged[:n], clean[:n]) for i in pair]
    g, o = _pair(ctx, oracle, graph, x)
    for batch in (order, order[::-1], order):
        assert _check(ctx, g, o, q[batch], 10, ef) == n


def test_a_top_phase_of_three_layers_and_nothing_survives_a_layer(ctx, oracle):
    """layers of 2 200 / 700 / 260 / 90 points at ef 16: the top launch runs three layers, each with a finite theta; layers end by
    lt >= ef with pending points left, and the model says the layer below would return something else had the values survived"""
    ef = 16
    g5 = _leveled(5000, 32, (2200, 700, 260, 90), 8, 11)
    assert len(g5["layers"]) == 5 and g5["small"] == 5
    for rows in ("float", "integer"):
        x, q = (g5["x"], g5["q"]) if rows == "float" else _tie_rows(g5, 111, hi=3)
        g, o = _pair(ctx, oracle, g5, x)
        for b, single in ((64, False), (31, True)):
            cls, seen = _classify(oracle, g5, x, q[:b], ef, single, stale=True)
            print("%s rows, batch %d: %d flagged, %s" % (rows, b, sum(cls), seen))
            assert seen["left_pending"] > 0 and seen["stale_differs"] > 0, (rows, b, seen)
            assert _check(ctx, g, o, q[:b], 10, ef) == sum(cls), (rows, b)


@pytest.mark.parametrize("nu,nu2", [(32600, 8000), (32700, 8100), (32800, 8200)])
def test_ownership_at_its_edges(ctx, oracle, nu, nu2):
    """bitmaps of (1020, 252), (1024, 256) and (1028, 260) words under blocks of (1024, 256) threads: one slice per thread with threads
    to spare, exactly one per thread, and more slices than threads (the full walk); batch 32 runs both launches, batch 8 the 1024-thread
    launch over every layer"""
    ef = 24
    g3 = _leveled(36000, 32, (nu, nu2, 40), 6, nu, nq=32, device="cuda")
    words, words2 = _words(nu), _words(nu2)
    assert (words, words2) in ((1020, 252), (1024, 256), (1028, 260))
    x, q = g3["x"], g3["q"]
    g, o = _pair(ctx, oracle, g3, x)
    cls, _ = _classify(oracle, g3, x, q, ef, False, classes=False)
    for b in (32, 8):
        assert _check(ctx, g, o, q[:b], 10, ef) == sum(cls[:b]), (nu, nu2, b)

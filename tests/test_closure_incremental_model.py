"""The single pop's incremental pass (tests/closure_incremental_model.py: the per-thread bookkeeping mdb_hnsw_closure.hip.h keeps —
seen, mu, mties, me, the owner's reset, the per-layer reset) against the scan of tests/closure_bound_model.py.  Runs without a GPU.

Random small graphs with integer rows, so that ties are common, and float rows; for every theta' up to the exact one — the exact value,
a coarse bin edge below it, 0 and the row's minimum (every point uncertain: the layer is popped one point at a time) — and for blocks
with a thread per word, several threads per word, one thread too few (every thread walks all its slices: the form before) and the
sizes in between:
  * at every pop, u, lt and le are what a scan over the pending set gives (closure_bound_layer's three lines, restated on the
    model's own sets), and the nearest evaluated point is the scan's;
  * what the layer returns — visited set, evaluations, expansions, handed-down point, the flag, the pops, the full pop list — is
    closure_bound_layer's;
  * two layers in a row: the second layer's trace is the same whether or not a first layer ran before it (nothing survives a layer).
"""
import numpy as np
import pytest
import torch

from muopdb_amd import synth
from tests import closure_bound_model as BM
from tests import closure_incremental_model as IM
from tests import closure_model as CM

NQ = 8


def _rows(x, max_neighbors, dup_seed=None):
    ids = np.arange(len(x), dtype=np.int64)
    indptr, edges = synth._layer_graph(torch.from_numpy(x), torch.from_numpy(ids), max_neighbors, min(64, len(ids) - 1))
    rows = CM.csr_rows(ids, indptr, edges)
    if dup_seed is not None:   # duplicate edges: every third row repeats two of its edges
        rng = np.random.default_rng(dup_seed)
        for p in range(0, len(x), 3):
            if len(rows[p]) >= 2:
                rows[p] = rows[p] + [rows[p][int(rng.integers(0, len(rows[p])))], rows[p][0]]
    return rows


def _bounds(pool, ef):
    th = CM.theta_of(pool, ef)
    if th is None:
        return {"exact": None}
    lo = min(pool)
    w = (th - lo) / 4.0
    edge = lo + float(np.floor((th - lo) / w - 0.5)) * w if w > 0 else lo
    return {"exact": th, "bin edge": min(max(edge, lo), th), "zero": 0.0, "row minimum": lo}


def _block_sizes(n):
    """threads per block, by what they make of a bitmap of `words` words: more than one slice per thread (the full walk), exactly as
    many threads as words, one more and one fewer, two threads per word less one and exact, 32 threads per word and more"""
    words = (n + 31) // 32
    return sorted({max(1, words // 3), words - 1, words, words + 1, 2 * words - 1, 2 * words, 8 * words, 32 * words, 32 * words + 7})


def _scan(pop, dist, ncert_of, popped):
    """closure_bound_layer's pass over the pending set, on the sets the model stood on at this pop"""
    pending = pop["evaluated"] - pop["expanded"]
    u = min(pending, key=lambda p: (dist[p], -p))
    lt = ncert_of(pop["evaluated"]) + sum(1 for d in popped if d < dist[u])
    le = lt + sum(1 for p in pending if dist[p] == dist[u]) + sum(1 for d in popped if d == dist[u])
    return u, lt, le, min(pop["evaluated"], key=lambda p: (dist[p], p))


def _check(oracle, x, q, rows, ef, seed, pop_cap=None):
    rng = np.random.default_rng(seed)
    n = len(x)
    seen = dict(runs=0, pops=0, flagged=0, cap_hit=0, tied_pop=0, pops_in_one_slice=0, ties_in_slice=0, ties_elsewhere=0,
                empty_pop=0, nearer_pop=0, full_walk=0, ended_with_pending=0)
    for qi in range(len(q)):
        dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
        pre = set(int(p) for p in rng.choice(n, n // 10, replace=False))
        ep = int(rng.integers(0, n))
        starts = [(0, set()), (ep, pre - {ep}), (int(np.argmax(dist)), set())]
        for ep, visited in starts:
            for name, tb in _bounds(dist, ef).items():
                want, winfo = BM.closure_bound_layer(rows, dist, ep, ef, visited, tb, pop_cap)
                for nt in _block_sizes(n):
                    words, ltpw, wbits, own_one = IM.slices(n, nt)
                    trace = []
                    got, ginfo = IM.closure_incremental_layer(rows, dist, ep, ef, visited, tb, nt, pop_cap, trace)
                    assert got.hazard == want.hazard and CM.same(want, got), (name, qi, ep, nt)
                    assert (got.pops, got.rounds) == (want.pops, want.rounds) and ginfo == winfo, (name, qi, ep, nt)
                    popped, prev = [], None

                    def ncert_of(evaluated):
                        return sum(1 for p in evaluated if tb is None or dist[p] < tb)

                    for i, pop in enumerate(trace):
                        u, lt, le, nearest = _scan(pop, dist, ncert_of, popped)
                        assert (pop["u"], pop["lt"], pop["le"], pop["nearest"]) == (u, lt, le, nearest), (name, qi, ep, nt, i)
                        if own_one and prev is not None:
                            slice_of = lambda p: (p >> 5 << ltpw) + ((p & 31) >> (5 - ltpw))
                            pend = pop["evaluated"] - pop["expanded"]
                            ties = [p for p in pend if p != u and dist[p] == dist[u]]
                            seen["pops_in_one_slice"] += slice_of(prev["u"]) == slice_of(u)
                            seen["ties_in_slice"] += any(slice_of(p) == slice_of(u) for p in ties)
                            seen["ties_elsewhere"] += any(slice_of(p) != slice_of(u) for p in ties)
                            new = pop["evaluated"] - prev["evaluated"]
                            seen["empty_pop"] += not new
                            seen["nearer_pop"] += u in new
                        popped.append(dist[pop["u"]])
                        prev = pop
                    seen["runs"] += 1
                    seen["pops"] += got.pops
                    seen["flagged"] += got.hazard
                    seen["cap_hit"] += ginfo.cap_hit
                    seen["tied_pop"] += ginfo.tied_with_earlier_pop
                    seen["full_walk"] += not own_one
                    seen["ended_with_pending"] += bool(trace) and trace[-1]["lt"] >= ef
    return seen


@pytest.mark.parametrize("n,d,hi,ef", [(300, 6, 2, 16), (500, 8, 3, 50), (260, 4, 1, 8), (330, 16, 1, 100)])
def test_integer_rows_every_pop_is_the_scans(oracle, n, d, hi, ef):
    rng = np.random.default_rng(n + d + ef)
    x = rng.integers(0, hi + 1, (n, d)).astype(np.float32)
    q = rng.integers(0, hi + 1, (NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 10, dup_seed=4), ef, 19)
    print(seen)
    assert seen["flagged"] > 0 and seen["tied_pop"] > 0 and seen["full_walk"] > 0, seen
    # the classes the bookkeeping can go wrong on all occur: consecutive pops in one thread's slice, ties of u inside that slice and
    # in other threads', a pop that evaluates nothing, a pop whose new minimum is a newly evaluated point
    assert min(seen[k] for k in ("pops_in_one_slice", "ties_in_slice", "ties_elsewhere", "empty_pop", "nearer_pop")) > 0, seen


@pytest.mark.parametrize("ef", [16, 64])
def test_float_rows_every_pop_is_the_scans(oracle, ef):
    rng = np.random.default_rng(5)
    n, d = 700, 12
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 10, dup_seed=3), ef, 17)
    assert seen["flagged"] == 0 and seen["pops"] > 0 and seen["pops_in_one_slice"] > 0 and seen["nearer_pop"] > 0, seen
    assert seen["ended_with_pending"] > 0 and seen["full_walk"] > 0, seen   # (layers that end by lt >= ef: pending points are left behind)


def test_a_full_pop_list_flags_alike(oracle):
    rng = np.random.default_rng(9)
    n, d, ef = 400, 8, 24
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 10), ef, 23, pop_cap=4)
    assert 0 < seen["cap_hit"] < seen["runs"], seen


def test_nothing_survives_a_layer(oracle):
    """a layer that ends by lt >= ef leaves pending points behind; the layer below, run after it from fresh values, returns what the
    scan returns — and with the values of the layer above still in the threads it does not (the test can fail)"""
    rng = np.random.default_rng(31)
    n, d, ef = 600, 8, 12
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    upper, lower = _rows(x, 6), _rows(x, 12)
    left_behind = told = 0
    for qi in range(NQ):
        dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
        tb = _bounds(dist, ef)["bin edge"]
        for nt in (19, 40, 160):
            assert IM.slices(n, nt)[3]
            t1, kept = [], IM.new_threads(nt)
            first, _ = IM.closure_incremental_layer(upper, dist, 0, ef, set(), tb, nt, None, t1, kept)
            want1, _ = BM.closure_bound_layer(upper, dist, 0, ef, set(), tb)
            assert not first.hazard and CM.same(want1, first)
            left_behind += bool(t1) and t1[-1]["lt"] >= ef and bool(t1[-1]["evaluated"] - t1[-1]["expanded"])
            want, _ = BM.closure_bound_layer(lower, dist, first.nearest, ef, first.visited, tb)
            fresh, _ = IM.closure_incremental_layer(lower, dist, first.nearest, ef, first.visited, tb, nt)
            assert fresh.hazard == want.hazard and CM.same(want, fresh) and fresh.pops == want.pops
            stale, _ = IM.closure_incremental_layer(lower, dist, first.nearest, ef, first.visited, tb, nt, None, None, kept)
            told += not (CM.same(want, stale) and stale.pops == want.pops)
    assert left_behind > 0 and told > 0, (left_behind, told)

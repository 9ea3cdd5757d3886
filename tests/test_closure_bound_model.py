"""theta as a bound and the counted stop test (tests/closure_bound_model.py: what mdb_hnsw_closure.hip.h runs) against the frontier
form with the exact theta and the scanned stop test (tests/closure_model.py, unchanged).  Runs without a GPU.

For every theta' <= theta — the exact value, a coarse bin edge below it, 0 and the row's minimum (every point uncertain: the layer is
popped one point at a time) — visited set, evaluations, expansions, handed-down point AND the flag are those of the existing model,
on float rows (no ties) and on integer rows (mostly ties).  A theta' ABOVE theta is not valid, and the test shows that it can be told:
it changes what a layer returns.
"""
import numpy as np
import pytest
import torch

from muopdb_amd import synth
from tests import closure_bound_model as BM
from tests import closure_model as CM

NQ = 12


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
    """the theta' <= theta the test runs, by name.  "bin edge": bins a quarter of [row minimum, theta] wide, and the lower edge of the
    one that holds theta less half a bin: row minimum + 3/4 of the way — strictly between the row minimum and theta wherever the two
    differ, so that some points stay certain and those in [edge, theta) are demoted to single pops"""
    th = CM.theta_of(pool, ef)
    if th is None:
        return {"exact": None}
    lo = min(pool)
    w = (th - lo) / 4.0
    edge = lo + float(np.floor((th - lo) / w - 0.5)) * w if w > 0 else lo
    return {"exact": th, "bin edge": min(max(edge, lo), th), "zero": 0.0, "row minimum": lo}


def _starts(rng, n, dist):
    pre = set(int(p) for p in rng.choice(n, n // 10, replace=False))
    ep = int(rng.integers(0, n))
    return [(0, set()), (ep, pre - {ep}), (int(np.argmax(dist)), set())]   # (the farthest point: an uncertain entry point)


def _check(oracle, x, q, rows, ef, seed, pop_cap=None):
    rng = np.random.default_rng(seed)
    seen = dict(runs=0, flagged=0, entry_uncertain=0, tied_pop=0, pops=0, cap_hit=0, edge_below=0, in_gap=0, demoted=0, demoted_flagged=0)
    for qi in range(len(q)):
        dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
        bounds = _bounds(dist, ef)
        th = bounds["exact"]
        if th is not None:
            # the select's own restatement keeps its promise on this row
            keys = BM.images(np.asarray(dist, dtype=np.float32))
            assert BM.theta_bound(keys, ef) <= CM.theta_of(keys, ef)
            assert all(b <= th for b in bounds.values())
            seen["edge_below"] += bounds["row minimum"] < bounds["bin edge"] < th
            seen["in_gap"] += sum(1 for v in dist if bounds["bin edge"] <= v < th)
        for ep, visited in _starts(rng, len(x), dist):
            want = CM.closure_layer(rows, dist, ep, ef, visited, th)
            if not want.hazard:
                assert CM.same(CM.search_layer(rows, dist, ep, ef, visited), want)
            for name, tb in bounds.items():
                got, info = BM.closure_bound_layer(rows, dist, ep, ef, visited, tb, pop_cap)
                if name == "bin edge" and not info.cap_hit:
                    # points of [edge, theta) this layer evaluated and expanded: popped alone here, frontier members under the exact theta
                    n = sum(1 for p in got.visited - set(visited) if tb <= dist[p] < th)
                    seen["demoted"] += n
                    seen["demoted_flagged"] += bool(n and got.hazard)
                seen["runs"] += 1
                seen["pops"] += got.pops
                seen["cap_hit"] += info.cap_hit
                if info.cap_hit:
                    continue                       # flagged for the list alone: the sequential form decides
                assert got.hazard == want.hazard, (name, qi, ep)
                assert CM.same(want, got), (name, qi, ep)
                seen["flagged"] += got.hazard
                seen["entry_uncertain"] += info.entry_uncertain
                seen["tied_pop"] += info.tied_with_earlier_pop
    return seen


@pytest.mark.parametrize("ef", [16, 64, 200])
def test_float_rows_any_bound_below_theta(oracle, ef):
    rng = np.random.default_rng(5)
    n, d = 1500, 24
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 12, dup_seed=3), ef, 17)
    assert seen["flagged"] == 0 and seen["entry_uncertain"] > 0, seen
    # the intermediate bound is a real one on every row: below theta, above the minimum, points in between, some of them reached
    assert seen["edge_below"] == NQ and seen["in_gap"] > 0 and seen["demoted"] > 0, seen


@pytest.mark.parametrize("n,d,hi,ef,long_groups,between", [(600, 8, 3, 50, False, True), (600, 8, 3, 200, False, True),
                                                           (1200, 6, 2, 64, True, True), (300, 16, 1, 100, False, True),
                                                           (400, 4, 1, 8, True, False)])
def test_tie_heavy_rows_any_bound_below_theta(oracle, n, d, hi, ef, long_groups, between):
    """integer rows: tie groups as long as ef and longer, u tied with an earlier pop, most queries flagged — by the same test whatever the bound"""
    rng = np.random.default_rng(n + d + ef)
    x = rng.integers(0, hi + 1, (n, d)).astype(np.float32)
    q = rng.integers(0, hi + 1, (NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 12, dup_seed=4), ef, 19)
    assert seen["flagged"] > 0 and seen["tied_pop"] > 0 and seen["entry_uncertain"] > 0, seen
    # ... also under the intermediate bound: on most rows it lies strictly between the minimum and theta with whole tie groups in
    # [edge, theta), the traversals reach them, and queries that demoted points are among the flagged ones (by the tie test further out)
    # (the last shape has five distinct distances and more than ef points at the nearest: theta IS the row minimum there)
    if between:
        assert seen["edge_below"] > NQ // 2 and seen["in_gap"] > 0 and seen["demoted"] > 0 and seen["demoted_flagged"] > 0, seen
    else:
        assert seen["edge_below"] == 0
    groups = max(np.unique(oracle.distance_many(0, q[0], x), return_counts=True)[1])
    assert groups >= ef or not long_groups, "longest tie group %d < ef %d: the shape no longer holds a tie group as long as ef" % (groups, ef)


def test_layer_of_at_most_64_points_has_no_bound_to_lower(oracle):
    """theta = +inf: a plain closure, nothing popped, nothing flagged; a finite bound over such a layer pops but returns the same"""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, (60, 6)).astype(np.float32)
    q = rng.integers(0, 3, (8, 6)).astype(np.float32)
    rows = _rows(x, 8)
    for ef in (64, 200):
        for qi in range(len(q)):
            dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
            assert CM.theta_of(dist, ef) is None
            want = CM.closure_layer(rows, dist, 5, ef, {1, 2}, None)
            got, _ = BM.closure_bound_layer(rows, dist, 5, ef, {1, 2}, None)
            assert not got.hazard and got.pops == 0 and CM.same(want, got), (ef, qi)
            low, _ = BM.closure_bound_layer(rows, dist, 5, ef, {1, 2}, min(dist))
            assert not low.hazard and low.pops >= low.expanded > 0 and CM.same(want, low), (ef, qi)


def test_a_full_pop_list_flags_and_nothing_else_changes(oracle):
    rng = np.random.default_rng(9)
    n, d, ef = 800, 16, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    seen = _check(oracle, x, q, _rows(x, 12), ef, 23, pop_cap=4)
    # (the row minimum as the bound pops every expansion alone: more than four of them)
    assert seen["cap_hit"] > 0 and seen["cap_hit"] < seen["runs"], seen


def test_a_bound_above_theta_can_be_told(oracle):
    """the test can fail: with theta' = +inf on a layer of more than ef points the form expands what the reference never reaches"""
    rng = np.random.default_rng(21)
    n, d, ef = 1500, 24, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    rows = _rows(x, 12)
    differ = 0
    for qi in range(len(q)):
        dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
        want = CM.closure_layer(rows, dist, 0, ef, set(), CM.theta_of(dist, ef))
        for tb in (None, sorted(dist)[4 * ef]):
            got, _ = BM.closure_bound_layer(rows, dist, 0, ef, set(), tb)
            differ += not CM.same(want, got)
    assert differ > 0

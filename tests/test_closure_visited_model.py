"""theta over the points not yet visited, selected late and reused downwards (tests/closure_visited_model.py: what
mdb_hnsw_closure.hip.h runs) against the reference's loop (tests/closure_model.search_layer, unchanged), layer by layer over chains of
three to five layers that share one visited set.  Runs without a GPU.

Every layer of every chain: visited set, evaluations, expansions and handed-down point are search_layer's from the same state, and the
flag is the one closure_model.closure_layer raises under the exact theta of the whole set (a point that becomes certain could not have
flagged).  Each case asserts that the class it exists for occurs.

The negative cases show that the comparison can tell a wrong pool and a wrong rank.  About the rank: the select takes index ef - 2 of
the unvisited rest (the entry point left out).  Index ef - 1 of the rest is never above index ef of the pool, and the form's lemma has
exactly that one rank to spare (a point with ef - 1 others as near is still accepted, never evicted and never behind the break), so it
returns what the reference returns — asserted here, so that the statement is checked and not only made.  Index ef of the rest is one
above every rank the lemma can carry, and that one is told apart.
"""
import numpy as np
import pytest
import torch

from muopdb_amd import synth
from tests import closure_bound_model as BM
from tests import closure_model as CM
from tests import closure_visited_model as VM

NQ = 12


def _rows(x, max_neighbors):
    ids = np.arange(len(x), dtype=np.int64)
    indptr, edges = synth._layer_graph(torch.from_numpy(x), torch.from_numpy(ids), max_neighbors, min(64, len(ids) - 1))
    return CM.csr_rows(ids, indptr, edges)


def _graph(x, sizes, max_neighbors=12):
    """layer l + 1 over the first sizes[l] points (sizes[0] = all of them): ([(layer, rows)] top first, set_of, members)"""
    layers = [(l + 1, _rows(x[:s], max_neighbors)) for l, s in enumerate(sizes)][::-1]
    members = {"all": range(sizes[0]), "top": range(sizes[1])}
    set_of = {l + 1: ("all" if l == 0 else "top") for l in range(len(sizes))}
    return layers, set_of, members


def _data(kind, n, d, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(0, 4, (n, d)).astype(np.float32), rng.integers(0, 4, (nq, d)).astype(np.float32)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)


def _dist(oracle, q, x, as_images):
    d = oracle.distance_many(0, q, x)
    return BM.images(np.asarray(d, dtype=np.float32)) if as_images else [float(v) for v in d]


def _hold(layers, set_of, members, dist, ef, all_certain, runs, seen):
    """every layer of one chain against search_layer and the exact-theta flag; class counts into `seen`"""
    for r, (layer, rows) in zip(runs, layers):
        want = CM.search_layer(rows, dist, r.ep, ef, r.visited_in)
        pool_of = [dist[p] for p in members[set_of[layer]]]
        row_theta = None if layer in all_certain else CM.theta_of(pool_of, ef)
        old = CM.closure_layer(rows, dist, r.ep, ef, r.visited_in, row_theta)
        assert r.state.hazard == old.hazard, (layer, r.ep)
        if not r.state.hazard:
            assert CM.same(want, r.state), (layer, r.ep)
        seen["layers"] += 1
        seen["flagged"] += r.state.hazard
        seen["pops"] += r.state.pops
        seen["pops_row_theta"] += old.pops
        seen["selects"] += r.selected
        seen["reused"] += (layer not in all_certain) and not r.selected
        if layer in all_certain or r.theta is None:
            continue
        rest = sorted(dist[p] for p in members[set_of[layer]] if p not in r.visited_in and p != r.ep)
        if row_theta is not None:
            seen["visited_below_row_theta"] += sum(1 for p in r.visited_in if p != r.ep and dist[p] < row_theta)
        if r.selected:
            assert r.rest == len(rest)
            seen["visited_nearer_than_all_rest"] += bool(r.visited_in) and min(dist[p] for p in r.visited_in) < rest[0]
            seen["tie_at_bound"] += sum(1 for v in rest if v == r.theta) >= 2
            seen["tie_across_bound"] += len(rest) > ef - 1 and rest[ef - 2] == rest[ef - 1]
            seen["ep_nearest"] += dist[r.ep] <= rest[0]
            seen["ep_farthest"] += dist[r.ep] >= rest[-1]


def _seen():
    return dict.fromkeys(("layers flagged pops pops_row_theta selects reused visited_below_row_theta visited_nearer_than_all_rest "
                          "tie_at_bound tie_across_bound ep_nearest ep_farthest").split(), 0)


@pytest.mark.parametrize("kind,n,sizes,d,ef", [("float", 1500, [1500, 200, 30], 24, 64), ("float", 1500, [1500, 200, 30], 24, 16),
                                                 ("float", 1200, [1200, 400, 30], 24, 200), ("int", 800, [800, 200, 30], 8, 50),
                                                 ("int", 800, [800, 200, 30], 8, 64)])
def test_chains_of_three_layers(oracle, kind, n, sizes, d, ef):
    x, q = _data(kind, n, d, NQ, n + d + ef)
    layers, set_of, members = _graph(x, sizes)
    all_certain = {l + 1 for l, s in enumerate(sizes) if s <= 64 and ef >= 64}
    seen = _seen()
    for qi in range(NQ):
        for as_images in (False, True):
            dist = _dist(oracle, q[qi], x, as_images)
            select = VM.select_rest_hist if as_images else VM.select_rest
            runs = VM.chain(layers, dist, 0, ef, set_of, members, all_certain, select=select)
            if as_images:       # the histogram's bin edge never lies above the exact select, nor is +inf where that is finite
                for r in runs:
                    if r.selected:
                        exact, rest = VM.select_rest(dist, members[set_of[r.layer]], r.visited_in | {r.ep}, ef)
                        assert rest == r.rest and (r.theta is None) == (exact is None) and (exact is None or r.theta <= exact)
            _hold(layers, set_of, members, dist, ef, all_certain, runs, seen)
    print(kind, ef, seen)
    # the layers above leave points below the whole set's theta in the visited set, and single pops fall against that theta
    assert seen["visited_below_row_theta"] > 0 and seen["visited_nearer_than_all_rest"] > 0 and seen["ep_nearest"] > 0, seen
    if ef >= 50:
        assert seen["pops"] < seen["pops_row_theta"], seen
    if kind == "int":
        assert seen["flagged"] > 0 and seen["tie_at_bound"] > 0 and seen["tie_across_bound"] > 0, seen
    else:
        assert seen["flagged"] == 0, seen


def test_a_select_reused_two_layers_down(oracle):
    """five layers, the three in the middle larger than ef and over one set: one select at layer 4 serves layers 3 and 2 as well;
    the entry point is the set's farthest point"""
    ef = 24
    sizes = [1200, 400, 300, 200, 20]                      # layers 1 .. 5; set "top" = the first 400 points
    x, q = _data("float", sizes[0], 16, NQ, 77)
    xi, qi_ = _data("int", sizes[0], 8, NQ, 78)
    seen = _seen()
    for xs, qs in ((x, q), (xi, qi_)):
        xs[0] = 50.0                                        # point 0, on every layer: farther from every query than any other point
        layers, set_of, members = _graph(xs, sizes)
        layers = layers[1:]                                 # start at layer 4, from point 0
        for qi in range(NQ):
            dist = _dist(oracle, qs[qi], xs, False)
            assert dist[0] == max(dist)
            runs = VM.chain(layers, dist, 0, ef, set_of, members)
            assert [r.selected for r in runs] == [True, False, False, True]
            assert runs[0].theta == runs[1].theta == runs[2].theta
            _hold(layers, set_of, members, dist, ef, (), runs, seen)
    print(seen)
    assert seen["reused"] == 2 * 2 * NQ and seen["ep_farthest"] > 0 and seen["visited_below_row_theta"] > 0, seen
    assert seen["pops"] < seen["pops_row_theta"], seen


@pytest.mark.parametrize("kind", ["float", "int"])
@pytest.mark.parametrize("extra,finite", [(8, False), (9, False), (10, True)])
def test_a_pool_of_ef_less_one_ef_and_ef_plus_one_points(oracle, kind, extra, finite):
    """layer 2: ten points, each linked to all the others, closed whole — all ten are visited when layer 1 is entered, its entry point
    among them.  Layer 1 over ef + extra points then has an unvisited rest of ef - 2, ef - 1 and ef points: a pool of ef - 1 and of ef
    points takes theta = +inf (nothing is popped alone), a pool of ef + 1 a finite one"""
    ef = 40
    n = ef + extra
    x, q = _data(kind, n, 8, NQ, 5 + extra)
    layers, set_of, members = _graph(x, [n, 10], max_neighbors=9)
    for qi in range(NQ):
        for as_images in (False, True):
            dist = _dist(oracle, q[qi], x, as_images)
            runs = VM.chain(layers, dist, 3, ef, set_of, members, all_certain={2},
                            select=VM.select_rest_hist if as_images else VM.select_rest)
            top, low = runs
            assert len(top.state.visited) == 10 and low.selected and low.rest == n - 10
            assert (low.theta is not None) == finite
            if not finite:
                assert low.state.pops == 0 and not low.state.hazard
            want = CM.search_layer(layers[1][1], dist, low.ep, ef, low.visited_in)
            if not low.state.hazard:
                assert CM.same(want, low.state)


def _mismatches(oracle, select, ef, kind="float", n=1500, d=24, sizes=(1500, 200, 30), seed=3):
    """-> (queries, of NQ, on which some layer's result differs from search_layer's or its flag from closure_layer's under the whole
    set's exact theta; flagged layers; selects whose rest holds a tie group across indices ef - 2 .. ef)"""
    x, q = _data(kind, n, d, NQ, seed)
    layers, set_of, members = _graph(x, list(sizes))
    all_certain = {l + 1 for l, s in enumerate(sizes) if s <= 64 and ef >= 64}
    bad = flagged = ties = 0
    for qi in range(NQ):
        dist = _dist(oracle, q[qi], x, False)
        runs = VM.chain(layers, dist, 0, ef, set_of, members, all_certain, select=select)
        wrong = False
        for r, (layer, rows) in zip(runs, layers):
            row_theta = None if layer in all_certain else CM.theta_of([dist[p] for p in members[set_of[layer]]], ef)
            wrong |= r.state.hazard != CM.closure_layer(rows, dist, r.ep, ef, r.visited_in, row_theta).hazard
            wrong |= not r.state.hazard and not CM.same(CM.search_layer(rows, dist, r.ep, ef, r.visited_in), r.state)
            flagged += r.state.hazard
            if r.selected and r.theta is not None:
                rest = sorted(dist[p] for p in members[set_of[layer]] if p not in r.visited_in and p != r.ep)
                ties += len(rest) > ef and rest[ef - 2] == rest[ef - 1] == rest[ef]
        bad += wrong
    return bad, flagged, ties


def test_a_pool_that_also_drops_unvisited_points_can_be_told(oracle):
    ef = 64

    def select(dist, members, visited, ef):
        nearest = sorted((p for p in members if p not in visited), key=lambda p: dist[p])[:ef // 4]
        return VM.select_rest(dist, members, visited, ef, drop=set(nearest))

    assert _mismatches(oracle, VM.select_rest, ef)[0] == 0
    assert _mismatches(oracle, select, ef)[0] > 0


TIE_ROWS = [dict(kind="int", n=800, d=8, sizes=(800, 200, 30), seed=9), dict(kind="int", n=1200, d=6, sizes=(1200, 300, 30), seed=10)]


def test_a_rank_too_high_can_be_told(oracle):
    """(module docstring) index ef - 1 of the rest — one above the rule — is inside the lemma's spare rank: results and flags are
    the reference's, on float rows and on integer rows with tie groups across the rank, flagged layers among them; index ef of the
    rest is one above every rank the lemma can carry, and is told apart"""
    for ef in (50, 64):
        def one_up(*a, ef=ef):
            return VM.select_rest(*a, rank=ef - 1)
        assert _mismatches(oracle, one_up, ef)[0] == 0
        for rows in TIE_ROWS:
            bad, flagged, ties = _mismatches(oracle, one_up, ef, **rows)
            assert bad == 0 and flagged > 0 and ties > 0, (ef, rows, bad, flagged, ties)
    ef = 64
    assert _mismatches(oracle, lambda *a: VM.select_rest(*a, rank=ef), ef)[0] > 0

"""The frontier form of an upper layer (tests/closure_model.py: what mdb_hnsw_closure.hip.h runs) against the reference's sequential
search_layer, both restated on the CPU over the oracle's distances.  Runs without a GPU.

  * whenever the hazard flag is clear, visited set, both counters and the handed-down point are the sequential form's;
  * every divergence carries the flag;
  * float Gaussian rows have no exact ties: the flag never fires there, and the frontier form needs a handful of rounds;
  * integer rows are mostly ties: the flag fires on most queries.

Two layers per case (a random eighth of the points above all of them), the visited set carried down, and — as a second start of the
lower layer — a random pre-visited set with a random entry point.
"""
import numpy as np
import pytest
import torch

from muopdb_amd import synth
from tests import closure_model as CM

NQ = 24


def _graph(x, max_neighbors, seed):
    """rows of layer 2 (a random eighth of the points) and layer 1 (all points)"""
    n = len(x)
    rng = np.random.default_rng(seed)
    top = np.sort(rng.choice(n, max(n // 8, 2), replace=False)).astype(np.int64)
    xt = torch.from_numpy(x)
    layers = []
    for ids in (top, np.arange(n, dtype=np.int64)):
        t = torch.from_numpy(ids)
        indptr, edges = synth._layer_graph(xt, t, max_neighbors, min(64, len(ids) - 1))
        layers.append((ids, CM.csr_rows(ids, indptr, edges)))
    return layers


def _run_case(oracle, x, q, layers, ef, seed):
    """-> (query-layers run, flagged, diverged, diverged without the flag, frontier rounds, single pops)"""
    rng = np.random.default_rng(seed)
    n = len(x)
    runs = flagged = diverged = unflagged = rounds = pops = 0
    for qi in range(len(q)):
        dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
        assert not any(v != v for v in dist)
        (top_ids, top_rows), (all_ids, all_rows) = layers
        starts = []
        # the query as ann_search runs it: top layer from its first point, the lower layer from what the top hands down
        ref2 = CM.search_layer(top_rows, dist, int(top_ids[0]), ef, set())
        starts.append((top_rows, [dist[int(p)] for p in top_ids], int(top_ids[0]), set()))
        starts.append((all_rows, dist, ref2.nearest, ref2.visited))
        # ... and the lower layer from a random entry point behind a random pre-visited set
        pre = set(int(p) for p in rng.choice(n, n // 10, replace=False))
        ep = int(rng.integers(0, n))
        starts.append((all_rows, dist, ep, pre - {ep}))
        for rows, pool, ep, visited in starts:
            ref = CM.search_layer(rows, dist, ep, ef, visited)
            got = CM.closure_layer(rows, dist, ep, ef, visited, CM.theta_of(pool, ef))
            runs += 1
            flagged += got.hazard
            rounds += got.rounds
            pops += got.pops
            if not CM.same(ref, got):
                diverged += 1
                unflagged += not got.hazard
    return runs, flagged, diverged, unflagged, rounds, pops


@pytest.mark.parametrize("ef", [64, 200])
def test_float_rows_never_flag_and_equal_the_sequential_form(oracle, ef):
    rng = np.random.default_rng(7)
    n, d = 4000, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    runs, flagged, diverged, unflagged, rounds, pops = _run_case(oracle, x, q, _graph(x, 16, 1), ef, 11)
    assert flagged == 0 and diverged == 0, (runs, flagged, diverged)
    # the point of the form: its dependent steps (block-wide rounds + single pops) are far fewer than the ~ef pops of the
    # sequential form — under half of them even on unclustered data from a random entry point
    print("ef %d: %.1f rounds + %.1f pops per query-layer" % (ef, rounds / runs, pops / runs))
    assert (rounds + pops) / runs < ef / 2, (rounds / runs, pops / runs)


@pytest.mark.parametrize("n,d,hi,ef", [(600, 8, 3, 50), (600, 8, 3, 200), (2000, 6, 2, 64), (300, 16, 1, 100)])
def test_tie_heavy_rows_flag_every_divergence(oracle, n, d, hi, ef):
    rng = np.random.default_rng(n + d + ef)
    x = rng.integers(0, hi + 1, (n, d)).astype(np.float32)
    q = rng.integers(0, hi + 1, (NQ, d)).astype(np.float32)
    runs, flagged, diverged, unflagged, _, _ = _run_case(oracle, x, q, _graph(x, 16, 2), ef, 13)
    assert unflagged == 0, "%d of %d query-layers differ from search_layer without the hazard flag" % (unflagged, runs)
    assert flagged > runs // 2, "the flag fired on %d of %d query-layers: the shape no longer exercises the tie case" % (flagged, runs)


def test_layer_of_at_most_ef_points_is_a_plain_closure(oracle):
    """theta = +inf: every reachable point is expanded, nothing is popped alone, no flag even on exact ties"""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, (120, 6)).astype(np.float32)
    q = rng.integers(0, 3, (8, 6)).astype(np.float32)
    ids = np.arange(120, dtype=np.int64)
    indptr, edges = synth._layer_graph(torch.from_numpy(x), torch.from_numpy(ids), 8, 32)
    rows = CM.csr_rows(ids, indptr, edges)
    for ef in (120, 121, 400):
        for qi in range(len(q)):
            dist = [float(v) for v in oracle.distance_many(0, q[qi], x)]
            ref = CM.search_layer(rows, dist, 5, ef, {1, 2})
            got = CM.closure_layer(rows, dist, 5, ef, {1, 2}, CM.theta_of(dist, ef))
            assert CM.theta_of(dist, ef) is None and not got.hazard and got.pops == 0 and CM.same(ref, got), (ef, qi)

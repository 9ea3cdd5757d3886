"""GPU parity tests (-m gpu) of the register beam's two compaction paths and of the layer-0 distance phase: rows, score
bits and both traversal counters against the CPU oracle.

Compaction.  When the over-full beam B has no free slot left, hnsw_beam_kernel and hnsw_upper_kernel first try to drop what
lies beyond `fbound` (a bound of furthest.distance the accept test maintains anyway) and only run the exact radix select
when that does not free enough slots.  Both leave a superset of the working set, so nothing observable may change.  The
graphs are 20 000 integer-valued rows of 16 dimensions (squared distances are small integers: exact ties everywhere), the
beam widths sit on both sides of every register-count boundary (208 | 209: four | five registers, 256 | 300: five | eight)
and every query of every case expands at least 2 ef nodes, i.e. B certainly filled up several times.

Distance phase.  A hand-written chain of hubs forces the number of unvisited neighbours of successive layer-0 pops to
0, 1, 12, 13, 24, 25, 28, 29 and 64 — every side of the one-vector-per-group / two-vectors-per-group switch — at d = 128
and d = 768.
"""
import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H
from tests.test_gpu_parity import assert_result_rows

pytestmark = pytest.mark.gpu

N, D, M = 20000, 16, 32
EFS = [64, 200, 208, 209, 256, 300, 448]


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


def _int_rows(n, d, seed):
    # SiftLike, narrow clusters: integer coordinates, so distances tie exactly by the hundred
    return H.sift_like(n, d, n_clusters=24, sigma=6.0, seed=seed)


def _int_queries(v, nq, seed):
    rng = np.random.default_rng(seed)
    return np.rint(v[rng.integers(0, len(v), nq)] + rng.normal(0, 3, (nq, v.shape[1]))).astype(np.float32)


def _knn_files(v, seed):
    import torch
    from muopdb_amd import synth as S
    return S.hnsw_files(torch.from_numpy(v).cuda(), max_neighbors=M, max_layers=8, kcand=2 * M, seed=seed)


@pytest.fixture(scope="module")
def graphs(oracle):
    """(index bytes, vector bytes, rows) per build, made once: the insert build is the oracle's HnswBuilder, the k-NN build
    muopdb_amd.synth's."""
    v = _int_rows(N, D, 5)
    ins = H.build_hnsw_files(oracle, v, list(range(N)), max_neighbors=M, max_layers=6, ef_construction=40, seed=2)
    knn = _knn_files(v, 2)
    return {"insert": ins + (v,), "knn": tuple(knn) + (v,)}


def _open(ctx, oracle, hidx, hvec, d, metric):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    return (BlockBasedHnsw(ctx, hidx, hvec, d, NoQuantizer(d, metric)),
            oracle.BlockBasedHnsw(hidx, hvec, d, oracle.Quant(oracle.QUANT_NONE, metric)))


def _check(ctx, g, o, batches, k, ef, min_expanded):
    """Every batch: rows + score bits; counters of the call equal the oracle's; EVERY query of it expands at least
    `min_expanded` nodes (the oracle, one query at a time: the counters are per call) — long enough to compact.  Returns the
    oracle's rows of the last batch."""
    for q in batches:
        o.stats()
        want = o.ann_search(q, k, ef)
        evals, expanded = o.stats()
        got = g.ann_search(q, k, ef)
        st = ctx.stats()
        assert_result_rows(got, want, len(q))
        assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (ef, len(q))
        per_query = [expanded]
        if len(q) > 1:
            per_query = []
            for i in range(len(q)):
                o.ann_search(q[i:i + 1], k, ef)
                per_query.append(o.stats()[1])
            assert sum(per_query) == expanded
        assert min(per_query) >= min_expanded, (ef, per_query)
    return want


@pytest.mark.parametrize("batch", [32, 1])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("build", ["insert", "knn"])
def test_compaction_paths_equal_oracle(ctx, oracle, graphs, build, metric, batch):
    """Batch 32: the table path (split: hnsw_upper_kernel on layer 1, then the layer-0 instance of hnsw_beam_kernel).
    Batch 1: the table path's single upper launch, and — MDB_HNSW_NO_TABLE — the all-layers beam kernel (ef <= 256; the
    general kernel above)."""
    hidx, hvec, v = graphs[build]
    g, o = _open(ctx, oracle, hidx, hvec, D, metric)
    q = _int_queries(v, 32, 11 + metric)
    for ef in EFS:
        if batch == 32:
            _check(ctx, g, o, [q], 10, ef, 2 * ef)
        else:
            _check(ctx, g, o, [q[5:6]], 10, ef, 2 * ef)
            with ctx.option("MDB_HNSW_NO_TABLE", 1):
                _check(ctx, g, o, [q[i:i + 1] for i in (0, 7, 19)], 10, ef, 2 * ef)
    g.close()


def _nearer_than(metric, q, x, t):
    """per query: how many rows of x are strictly nearer than the point t (f64, exact on these integer coordinates; only used
    to choose queries)"""
    q, x, t = q.astype(np.float64), x.astype(np.float64), t.astype(np.float64)
    if metric == 0:   # |q - x|^2 < |q - t|^2  <=>  |x|^2 - 2 q.x < |t|^2 - 2 q.t
        return (((x * x).sum(1)[None, :] - 2.0 * (q @ x.T)) < ((t * t).sum() - 2.0 * (q @ t))[:, None]).sum(1)
    return ((q @ x.T) > (q @ t)[:, None]).sum(1)


def test_compaction_with_long_tie_runs_equals_oracle(ctx, oracle):
    """40 % of the base is three distinct vectors (runs of ~2 700 exact ties).  The graph is built over jittered copies of them
    and searched over the exact copies — the files are independent — so a run is woven into its surroundings instead of being
    an island of copies that link to each other, and every traversal is as long as in the other cases (>= 2 ef expansions).
    The queries sit at graded distances from a run: 0, 30, 70 ... 400 other points are nearer than the run.  Where fewer than ef
    are, furthest.distance IS the run's distance while nearer points keep arriving: `fbound` equals furthest across the run, the
    bound drop frees nothing and the exact select runs; with more than the beam's slack of nearer points the block re-runs
    its query with the general traversal.  Asserted from the oracle's rows (k = ef): for ef >= 200 at least five queries end with
    a run member as furthest AND more than 56 results outside the runs."""
    v = _int_rows(N, D, 6)
    rng = np.random.default_rng(17)
    dup = rng.permutation(N)[:2 * N // 5]
    runs, which = v[dup[:3]].copy(), rng.integers(0, 3, len(dup))
    v[dup] = np.rint(runs[which] + rng.normal(0, 6, (len(dup), D))).astype(np.float32)
    hidx, _ = H.build_hnsw_files(oracle, v, list(range(N)), max_neighbors=M, max_layers=6, ef_construction=40, seed=3)
    v[dup] = runs[which]
    hvec = F.write_vector_file(v)
    in_run = np.zeros(N, bool)
    in_run[dup] = True
    others = v[~in_run]
    for metric in (0, 1):
        qs = []
        for t in runs:
            cand = np.rint(t + rng.normal(0, 1, (600, D)) * rng.uniform(2, 16, (600, 1))).astype(np.float32)
            nearer = _nearer_than(metric, cand, others, t)
            qs += [cand[np.argmin(np.abs(nearer - c))] for c in (0, 30, 70, 110, 150, 190, 240, 300, 400)]
        q = np.stack(qs + [v[dup[0]]])
        g, o = _open(ctx, oracle, hidx, hvec, D, metric)
        for ef in (64, 200, 256, 448):
            want = _check(ctx, g, o, [q], ef, ef, 2 * ef)
            rows = [want.doc_ids(i) for i in range(len(q))]
            straddle = sum(1 for r in rows if len(r) == ef and in_run[int(r[-1])] and sum(1 for x in r if not in_run[int(x)]) > 56)
            assert ef < 200 or straddle >= 5, (metric, ef, straddle)
        g.close()


# ----------------------------------------------------------------------------------- layer-0 distance phase
NEW_PER_POP = [1, 12, 13, 24, 25, 28, 29, 64]   # + 0: the last hub and every leaf


def _hub_chain(d, seed):
    """Two layers.  Layer 1 holds hub 0 alone (the entry point).  On layer 0, hub i's row is hub i + 1 and c_i - 1 fresh leaves,
    the last hub's row is its predecessor, a leaf's row is its hub: c_i unvisited neighbours when hub i is popped, none for the
    rest.  Hub i + 1 is nearer to every query than hub i and than any leaf, so the hubs are popped in order."""
    rng = np.random.default_rng(seed)
    nh = len(NEW_PER_POP) + 1
    rows, vec = {}, []
    for i in range(nh):
        x = np.zeros(d, np.float32)
        x[0] = 2.0 * (nh - i)
        vec.append(x)
    for i, c in enumerate(NEW_PER_POP):
        leaves = list(range(len(vec), len(vec) + c - 1))
        for p in leaves:
            vec.append(np.rint(rng.normal(0, 40, d)).astype(np.float32) + np.float32(100.0))
            rows[p] = [i]
        rows[i] = [i + 1] + leaves
    rows[nh - 1] = [nh - 2]
    vec = np.stack(vec)
    n = len(vec)
    assert max(len(r) for r in rows.values()) == 64 and n == nh + sum(NEW_PER_POP) - len(NEW_PER_POP)
    index = F.write_hnsw_index([rows, {0: []}], list(range(n)), d)
    return index, F.write_vector_file(vec), vec


@pytest.mark.parametrize("ef", [200, 400])
@pytest.mark.parametrize("d", [128, 768])
def test_layer0_distance_phase_on_hub_chain(ctx, oracle, d, ef):
    hidx, hvec, vec = _hub_chain(d, 31 + d)
    g, o = _open(ctx, oracle, hidx, hvec, d, 0)
    rng = np.random.default_rng(d + ef)
    q = rng.normal(0, 0.05, (64, d)).astype(np.float32)
    n, nh = len(vec), len(NEW_PER_POP) + 1
    for batch in (q, q[:33], q[:1]):
        o.stats()
        want = o.ann_search(batch, 150, ef)
        evals, expanded = o.stats()
        got = g.ann_search(batch, 150, ef)
        st = ctx.stats()
        assert_result_rows(got, want, len(batch))
        assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded)
        # the chain was walked to its end: every point evaluated once per layer-0 traversal (+ hub 0 on layer 1), all of them expanded
        assert evals == (n + 1) * len(batch) and expanded == n * len(batch)
        assert [int(x) for x in want.doc_ids(0)[:nh]] == list(range(nh - 1, -1, -1))   # nearest first = last hub first
    g.close()


def test_layer0_distance_phase_on_wide_rows(ctx, oracle):
    """The 20 000-row integer base at d = 128, k-NN build, batch 64: rows of up to 64 edges on the layer-0 instance."""
    v = _int_rows(N, 128, 8)
    hidx, hvec = _knn_files(v, 4)
    q = _int_queries(v, 64, 29)
    for metric in (0, 1):
        g, o = _open(ctx, oracle, hidx, hvec, 128, metric)
        for ef in (200, 400):
            _check(ctx, g, o, [q], 10, ef, 2 * ef)
        g.close()

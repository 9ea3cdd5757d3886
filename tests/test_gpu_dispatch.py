"""Parity of every kernel form the host dispatch and the MDB_* options can select (-m gpu).  Each case forces one form — through
the shape that selects it by default or through the option — and compares ids, counts and f32 score bits with the oracle; where a
batch is larger than the oracle can afford, every row is compared with the exact kernels (MDB_FLAT_NO_MFMA, or the default path of
the same index) and at least 32 rows, the last (partial) query block included, with the oracle.  HNSW cases check the traversal
counters against the oracle's, IVF cases the scored-vector counter against the default path's."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_parity import _ivf_case, assert_result_rows, assert_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, **opts):
    with contextlib.ExitStack() as st:
        for name, val in opts.items():
            st.enter_context(ctx.option(name, val))
        yield


def _same(a, b, what=""):
    ids, dist, counts = a
    eids, edist, ecounts = b
    assert np.array_equal(counts, ecounts), what
    assert np.array_equal(ids, eids), what
    assert np.array_equal(dist.view(np.uint32), edist.view(np.uint32)), what


def _oracle_rows(b):
    """32 rows: the first 16 and the last 16 (the last, partial query block)"""
    return np.unique(np.r_[0:min(16, b), max(0, b - 16):b])


def _check_oracle(oracle, metric, base, q, k, got):
    ids, dist, counts = got
    sel = _oracle_rows(len(q))
    oids, odist = oracle.flat_topk(metric, base, q[sel], k, threads=max(1, min(64, oracle.num_threads())))
    kk = min(k, len(base))
    assert counts[sel].tolist() == [kk] * len(sel)
    assert np.array_equal(ids[sel, :kk], oids[:, :kk])
    assert_scores(dist[sel, :kk], odist[:, :kk])


def _exact(ctx, idx, q, k):
    with ctx.option("MDB_FLAT_NO_MFMA", 1):
        return idx.search(q, k)


# ----------------------------------------------------------------------------------- flat, batched path (mdb_flat_mfma.hip)
@pytest.fixture(scope="module")
def qb_base():
    """262 145 rows of d = 128: the first 262 144 are the last base whose bf16 rows fit 64 MB (block filter QB 1), all of them the first
    on QB 2"""
    rng = np.random.default_rng(262_144)
    base = H.sift_like(262_145, 128, n_clusters=80, seed=7)
    q = (base[rng.integers(0, len(base), 520)] + rng.normal(0, 10, (520, 128))).astype(np.float32)
    return base, q


@pytest.mark.parametrize("n,metric", [(262_144, 0), (262_145, 0), (262_145, 1)])
def test_block_filter_automatic_query_blocks(ctx, oracle, qb_base, n, metric):
    """flat_bf16x1_block_kernel takes one query block per wave while the bf16 rows fit 64 MB (n <= 262 144 at d = 128), two beyond"""
    from muopdb_amd.index import FlatIndex
    base, q = qb_base
    base = base[:n]
    idx = FlatIndex(ctx, base, metric)
    with ctx.option("MDB_BF_X1", 2):   # (dot stores take the three-product filter by default; the block filter is the one-product form)
        got = idx.search(q, 10)
    _same(got, _exact(ctx, idx, q, 10))
    _check_oracle(oracle, metric, base, q, 10, got)


@pytest.fixture(scope="module")
def base100k():
    return H.sift_like(100_000, 128, n_clusters=60, seed=100)


@pytest.mark.parametrize("qb", [1, 2, 4])
def test_block_filter_query_blocks_option(ctx, oracle, base100k, qb):
    """MDB_BF_BLOCK_QB = 1 / 2 / 4 query blocks per wave, at batches that leave a partial query block"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(qb)
    base = base100k
    idx = FlatIndex(ctx, base, 0)
    for b in (512, 513, 777):
        q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 12, (b, 128))).astype(np.float32)
        with ctx.option("MDB_BF_BLOCK_QB", qb):
            got = idx.search(q, 10)
        _same(got, _exact(ctx, idx, q, 10), (qb, b))
        _check_oracle(oracle, 0, base, q, 10, got)


@pytest.mark.parametrize("qb", [1, 2, 8])
def test_filter_query_blocks_option(ctx, oracle, base100k, qb):
    """MDB_BF_QB: query blocks of 32 per block of the per-wave bf16 filter (batches below MDB_BF_BLOCK_MIN_B), L2 (one product) and
    dot (three products), d = 128 and d = 120"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(10 + qb)
    for d, metric in ((128, 0), (120, 0), (128, 1)):
        base = np.ascontiguousarray(base100k[:, :d])
        idx = FlatIndex(ctx, base, metric)
        for b in (300, 97):
            q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 12, (b, d))).astype(np.float32)
            with ctx.option("MDB_BF_QB", qb):
                got = idx.search(q, 20)
            _same(got, _exact(ctx, idx, q, 20), (qb, d, metric, b))
            _check_oracle(oracle, metric, base, q, 20, got)


def _sweep_bases():
    rng = np.random.default_rng(65_536)
    gauss = H.sift_like(65_536, 128, n_clusters=40, seed=3)
    distinct = np.rint(rng.standard_normal((4096, 120)) * 2).astype(np.float32)
    dup = distinct[rng.permutation(np.repeat(np.arange(4096), 16))]    # every row 16 times: ties reach the k-th slot
    return {"sift": gauss, "dup": dup}


@pytest.fixture(scope="module")
def sweep_bases():
    return _sweep_bases()


@pytest.mark.parametrize("kind,metric", [("sift", 0), ("sift", 1), ("dup", 0)])
@pytest.mark.parametrize("b", [8, 100, 600])
def test_flat_k_sweep(ctx, oracle, sweep_bases, kind, metric, b):
    """k across the forms' limits (the bf16 sample bound and the refine by query groups up to 256, the small group blocks up to 128,
    wave slices up to 64, the filter's candidate cap at 1024, MDB_MAX_K) on a 65 536-row base that takes the matrix-core filter:
    the default sample (1/32: k <= 256 filtered) and the whole base as the sample (MDB_MF_SAMPLE_DIV=1 at load: k <= 1024 filtered,
    k > 256 through the exact sample top-k and the refine by slices)"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(b + metric)
    base = sweep_bases[kind]
    d = base.shape[1]
    q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 1 if kind == "dup" else 10, (b, d))).astype(np.float32)
    if kind == "dup":
        q[: b // 4] = base[rng.integers(0, len(base), b // 4)]                 # queries ON stored rows: 16 ties at distance 0
    idx = FlatIndex(ctx, base, metric)
    with ctx.option("MDB_MF_SAMPLE_DIV", 1):
        idx1 = FlatIndex(ctx, base, metric)
    with ctx.option("MDB_MF_COOLDOWN", 0):   # (an overflowing list must not send the next calls to the exact kernels)
        for k in (1, 64, 65, 128, 129, 256, 257, 1024, 2048):
            exact = _exact(ctx, idx, q, k)
            for g in (idx, idx1):
                _same(g.search(q, k), exact, k)
            _check_oracle(oracle, metric, base, q, k, exact)


@pytest.mark.parametrize("opts", [dict(MDB_REFINE_GROUP_BIG=1),
                                  dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=1), dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=3),
                                  dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=8), dict(MDB_REFINE_SLICES=3),
                                  dict(MDB_FLAT_QT=1), dict(MDB_FLAT_QT=2), dict(MDB_FLAT_QT=4)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("d", [128, 120])
def test_flat_refine_and_scan_options(ctx, oracle, sweep_bases, opts, d):
    """the refine's forms (one block per query with the 2048-key blocks behind the whole-base bound; slices of 1 / 3 / 8 with the
    merge launch, 256-thread and one-wave slices) and the exact scan's queries per block (the sample top-k of k > 256, the exact
    kernels) — at batches 8 / 100 / 600 and k on both sides of the forms' limits"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(d)
    base = np.ascontiguousarray(sweep_bases["sift"][:, :d])
    idx = FlatIndex(ctx, base, 0)
    with ctx.option("MDB_MF_SAMPLE_DIV", 1):   # (the whole base as the sample: k = 300 filtered, through the exact sample top-k)
        idx1 = FlatIndex(ctx, base, 0)
    for b in (8, 100, 600):
        q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 10, (b, d))).astype(np.float32)
        for k in (10, 100, 300):
            exact = _exact(ctx, idx, q, k)
            with options(ctx, MDB_MF_COOLDOWN=0, **opts):
                for g in (idx, idx1):
                    _same(g.search(q, k), exact, (b, k))
                if "MDB_FLAT_QT" in opts:
                    with ctx.option("MDB_FLAT_NO_MFMA", 1):
                        _same(idx.search(q, k), exact, (b, k))
            _check_oracle(oracle, 0, base, q, k, exact)


@pytest.mark.parametrize("metric", [0, 1])
def test_flat_f32_matrix_core_filter(ctx, oracle, sweep_bases, metric):
    """MDB_MF_F32 (read at load): the f32-MFMA filter over the centred copy instead of the bf16 filters"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(32 + metric)
    for d in (128, 120):
        base = np.ascontiguousarray(sweep_bases["sift"][:, :d])
        with ctx.option("MDB_MF_F32", 1):
            idx = FlatIndex(ctx, base, metric)
        for b in (8, 100, 600):
            q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 10, (b, d))).astype(np.float32)
            for k in (10, 129):
                with ctx.option("MDB_MF_COOLDOWN", 0):
                    got = idx.search(q, k)
                _same(got, _exact(ctx, idx, q, k), (d, b, k))
                _check_oracle(oracle, metric, base, q, k, got)


# ----------------------------------------------------------------------------------- IVF / PQ posting-list scans (mdb_ivf.hip)
def _batch(v, b, seed, d):
    rng = np.random.default_rng(seed)
    return (v[rng.integers(0, len(v), b)] + rng.normal(0, 2, (b, d))).astype(np.float32)


def _scored(ctx):
    return ctx.stats()["scored_vectors"]


# mw = code words per vector: m = 4 / 8 / 16 / 32 subspaces of 8 bits
PQ_SHAPES = {1: (32, 8), 2: (64, 8), 4: (128, 8), 8: (128, 4)}


@pytest.mark.parametrize("mw", [1, 2, 4, 8])
def test_two_phase_pq_scan_forms(ctx, oracle, mw):
    """ivf_scan_pq3_kernel at its two instantiated block sizes (MDB_PQ3_BLOCK 512 / 1024), with and without the whole-word code path
    (pq_full: 8-bit codes in whole words; MDB_PQ_NO_FULL), its grid (MDB_PQ3_BLOCKS), the selector's warm rounds and eager trim, and
    candidate lists that overflow (MDB_PQ3_CAP=8: the gated one-phase launch redoes the batch)"""
    d, sub = PQ_SHAPES[mw]
    n, L, P, k, b = 3000, 12, 6, 10, 520
    o, g, _, v, _ = _ivf_case(oracle, ctx, n, d, L, seed=700 + mw, quant=(sub, 8))
    q = _batch(v, b, mw, d)
    want = o.search(q, k, num_probes=P)
    got = g.search(q, k, P)
    base_scored = _scored(ctx)
    assert_result_rows(got, want, b)
    assert base_scored > 0
    cases = [dict(MDB_PQ3_BLOCK=1024), dict(MDB_PQ_NO_FULL=1), dict(MDB_PQ3_BLOCK=1024, MDB_PQ_NO_FULL=1),
             dict(MDB_PQ3_BLOCKS=1), dict(MDB_PQ3_BLOCKS=4096), dict(MDB_PQ3_WARM_ROUNDS=0), dict(MDB_PQ3_WARM_ROUNDS=255),
             dict(MDB_PQ_EAGER_TRIM=0), dict(MDB_PQ_EAGER_TRIM=2), dict(MDB_PQ3_BLOCK=1024, MDB_PQ3_CAP=8),
             dict(MDB_PQ3_BLOCK=1024, MDB_PQ_EAGER_TRIM=2, MDB_PQ3_WARM_ROUNDS=0)]
    for opts in cases:
        with options(ctx, **opts):
            assert_result_rows(g.search(q, k, P), want, b)
        assert _scored(ctx) == base_scored, opts


@pytest.mark.parametrize("bits", [6, 8])
def test_two_phase_pq_scan_small_batches(ctx, oracle, bits):
    """MDB_PQ_TWO_PHASE_MIN_B=1 (with one block per query, MDB_PQ_BLOCKS=1): the two-phase scan at batches 1 and 33, also with
    candidate lists of 8 slots (the overflow re-run); codes of 6 bits (no whole-word path) and of 8"""
    n, d, sub, L, P, k = 3000, 64, 8, 10, 5, 10
    o, g, q24, v, _ = _ivf_case(oracle, ctx, n, d, L, seed=900 + bits, quant=(sub, bits))
    q = _batch(v, 33, bits, d)
    for b in (1, 33):
        want = o.search(q[:b], k, num_probes=P)
        with ctx.option("MDB_PQ_NO_FUSED", 1):
            g.search(q[:b], k, P)
            ref_scored = _scored(ctx)
        for cap in (2048, 8):
            with options(ctx, MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1, MDB_PQ3_CAP=cap):
                assert_result_rows(g.search(q[:b], k, P), want, b)
            assert _scored(ctx) == ref_scored, (b, cap)


@pytest.mark.parametrize("d,sub,bits", [(64, 8, 8), (128, 8, 8), (128, 4, 8), (64, 8, 6), (48, 16, 6)])
def test_one_phase_pq_scan_options(ctx, oracle, d, sub, bits):
    """the unfused one-phase step: the generic kernel (MDB_PQ_NO_FAST), ivf_scan_pq2_kernel without the whole-word path
    (MDB_PQ_NO_FULL), one split per query and the largest split count (MDB_PQ_BLOCKS 1 / 100000), the per-subspace quantizer
    (MDB_PQ_NO_QUANTIZE8: the codes must equal too)"""
    from muopdb_amd.index import ProductQuantizer
    n, L, P, k = 3000, 10, 6, 10
    o, g, q, v, _ = _ivf_case(oracle, ctx, n, d, L, seed=d + sub + bits, quant=(sub, bits))
    b = len(q)
    want = o.search(q, k, num_probes=P)
    with ctx.option("MDB_PQ_NO_FUSED", 1):
        assert_result_rows(g.search(q, k, P), want, b)
        ref_scored = _scored(ctx)
        for opts in (dict(MDB_PQ_NO_FAST=1), dict(MDB_PQ_NO_FULL=1), dict(MDB_PQ_BLOCKS=1), dict(MDB_PQ_BLOCKS=100000),
                     dict(MDB_PQ_NO_QUANTIZE8=1), dict(MDB_PQ_NO_FAST=1, MDB_PQ_BLOCKS=1)):
            with options(ctx, **opts):
                assert_result_rows(g.search(q, k, P), want, b)
            assert _scored(ctx) == ref_scored, opts
    cb = H.train_pq_codebook(v[: min(n, 2000)], sub, bits, iters=3)
    pq, opq = ProductQuantizer(d, sub, bits, cb), oracle.ProductQuantizer(d, sub, bits, cb)
    want_codes = opq.quantize(v[:500])
    with ctx.option("MDB_PQ_NO_QUANTIZE8", 1):
        assert np.array_equal(pq.quantize(ctx, v[:500]), want_codes)
    assert np.array_equal(pq.quantize(ctx, v[:500]), want_codes)


@pytest.fixture(scope="module")
def fused_case(oracle, ctx):
    """1 024 centroids of d = 64 (matrix-core coarse search), 8-bit PQ of 8 subspaces: the fused step's shape"""
    from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
    rng = np.random.default_rng(1024)
    L_, d, n = 1024, 64, 4000
    cent = H.sift_like(L_, d, n_clusters=32, seed=11)
    pick = rng.integers(0, L_, n)
    v = (cent[pick] + rng.normal(0, 3.0, (n, d))).astype(np.float32)
    cb = H.train_pq_codebook(v[:1500], 8, 8, iters=2)
    opq = oracle.ProductQuantizer(d, 8, 8, cb)
    index, vec, _ = H.build_ivf_files(v, list(range(10, 10 + n)), cent, quantize=opq.quantize)
    o = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 8, 8, cb))
    g = BlockBasedIvf(ctx, index, vec, ProductQuantizer(d, 8, 8, cb))
    q = (cent[rng.integers(0, L_, 48)] + rng.normal(0, 4.0, (48, d))).astype(np.float32)
    return o, g, q, n


@pytest.mark.parametrize("opts", [dict(MDB_CM_SPLIT=1), dict(MDB_CM_GLOBAL_BOUND=0), dict(MDB_PQF_NO_QUANT_IN_COARSE=1),
                                  dict(MDB_CM_SPLIT=1, MDB_PQF_CAP=8), dict(MDB_IVF_COARSE_MFMA_MIN_B=1)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_fused_step_coarse_options(ctx, oracle, fused_case, opts):
    """ivf_pq_fused_kernel behind the matrix-core coarse search: the candidates ranked in a launch of their own (MDB_CM_SPLIT), without
    the second-level bound (MDB_CM_GLOBAL_BOUND=0), queries quantized by the fused kernel itself, the coarse filter at batches 1..31"""
    o, g, q, n = fused_case
    P, k = 16, 10
    for b in (48, 33, 31, 7, 1):
        want = o.search(q[:b], k, num_probes=P)
        with ctx.option("MDB_PQ_NO_FUSED", 1):
            g.search(q[:b], k, P)
            ref_scored = _scored(ctx)
        with options(ctx, **opts):
            assert np.array_equal(g.find_nearest_centroids(q[:b], P), o.find_nearest_centroids(q[:b], P)), b
            assert_result_rows(g.search(q[:b], k, P), want, b)
            assert _scored(ctx) == ref_scored, b


@pytest.mark.parametrize("div", [1, 64])
def test_large_coarse_quantizer_sample_div(ctx, oracle, div):
    """MDB_IVF_COARSE_SAMPLE_DIV (read at load): the sample of a >= 64K-centroid coarse quantizer as the whole quantizer / 1/64 of it"""
    from muopdb_amd import formats as F
    from muopdb_amd.index import BlockBasedIvf
    rng = np.random.default_rng(div)
    L_, d = 65_536, 24
    cent = (rng.standard_normal((L_, d)) * 30).astype(np.float32)
    cent[100] = cent[7]
    v = (cent + rng.standard_normal((L_, d))).astype(np.float32)
    pls = [np.array([i], np.uint64) for i in range(L_)]
    index, vec = F.write_ivf_index(cent, [3 * i + 1 for i in range(L_)], pls), F.write_vector_file(v)
    with ctx.option("MDB_IVF_COARSE_SAMPLE_DIV", div):
        g = BlockBasedIvf(ctx, index, vec)
    o = oracle.BlockBasedIvf(index, vec)
    q = (cent[rng.integers(0, L_, 70)] + rng.standard_normal((70, d)) * 2).astype(np.float32)
    q[3] = cent[7]
    with ctx.option("MDB_MF_COOLDOWN", 0):
        for P in (8, 16):   # (1/64: 16 sample tiles bound k <= 16 candidates' worth of the filter)
            assert np.array_equal(g.find_nearest_centroids(q, P), o.find_nearest_centroids(q, P)), P
            assert_result_rows(g.search(q, 10, P), o.search(q, 10, num_probes=P), len(q))
    g.close()


def _three_states(ctx, oracle, o, g, q, k, P, n):
    """rows under MDB_SCAN_MASKS_ALWAYS=1 and without it: clean index, a shared planner filter, per-query filters, tombstones"""
    from muopdb_amd.index import allow_bitmap

    def search(planner=None):
        return g.search(q, k, P, planner=planner)
    b = len(q)
    rng = np.random.default_rng(n)
    want = o.search(q, k, num_probes=P)
    for masks in (0, 1):
        with ctx.option("MDB_SCAN_MASKS_ALWAYS", masks):
            assert_result_rows(search(), want, b)
    shared = allow_bitmap(np.sort(rng.choice(n, n // 2, replace=False)), n)
    per_q = np.stack([allow_bitmap(np.sort(rng.choice(n, n // 3, replace=False)), n) for _ in range(b)])
    for bm in (shared, per_q):
        with oracle.planner_filter(bm):
            fw = o.search(q, k, num_probes=P)
        for masks in (0, 1):
            with ctx.option("MDB_SCAN_MASKS_ALWAYS", masks):
                assert_result_rows(search(planner=bm), fw, b)
    dead = sorted({want.doc_ids(i)[0] for i in range(b) if want.counts[i]})[:8]
    for doc in dead:
        assert g.invalidate(doc) and o.invalidate(doc)
    want = o.search(q, k, num_probes=P)
    for masks in (0, 1):
        with ctx.option("MDB_SCAN_MASKS_ALWAYS", masks):
            assert_result_rows(search(), want, b)


@pytest.mark.parametrize("form", ["f32", "two_phase", "fused"])
def test_scan_masks_always(ctx, oracle, form):
    """MDB_SCAN_MASKS_ALWAYS: the posting-list scans read the tombstone / allow words even when nothing was invalidated and no filter
    is given — the f32 scan, the two-phase PQ scan and the fused IVF-PQ step, each without tombstones, with a planner filter and with
    tombstones"""
    n, d, L, P, k = 3000, 64, 12, 6, 10
    if form == "f32":
        o, g, q, v, _ = _ivf_case(oracle, ctx, n, d, L, seed=41)
    else:
        o, g, q, v, _ = _ivf_case(oracle, ctx, n, d, L, seed=42, quant=(8, 8))
    if form == "two_phase":
        q = _batch(v, 520, 3, d)
    _three_states(ctx, oracle, o, g, q, k, P, n)


# ----------------------------------------------------------------------------------- HNSW upper layers (mdb_hnsw_upper.hip)
@pytest.fixture(scope="module", params=[(128, 0), (128, 1)], ids=["l2", "dot"])
def hnsw_case(request, oracle, ctx):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    d, metric = request.param
    rng = np.random.default_rng(31)
    n = 3000
    v = H.sift_like(n, d, n_clusters=24, seed=6)
    if metric == 1:
        v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    hidx, hvec = H.build_hnsw_files(oracle, v, list(range(n)), max_neighbors=12, max_layers=4, ef_construction=60, metric=metric)
    g = BlockBasedHnsw(ctx, hidx, hvec, d, NoQuantizer(d, metric))
    o = oracle.BlockBasedHnsw(hidx, hvec, d, oracle.Quant(oracle.QUANT_NONE, metric))
    q = (v[rng.integers(0, n, 40)] + rng.normal(0, 0.05 if metric == 1 else 4, (40, d))).astype(np.float32)
    return g, o, q


@pytest.mark.parametrize("opts", [dict(MDB_HNSW_TABLE_QT=2), dict(MDB_HNSW_TABLE_QT=8), dict(MDB_HNSW_TABLE64_MIN_B=1),
                                  dict(MDB_HNSW_TABLE64_MIN_B=1 << 30), dict(MDB_HNSW_TABLE_MIN_B=1 << 30), dict(MDB_HNSW_NB4_SLACK=0),
                                  dict(MDB_HNSW_TABLE64_MIN_B=1, MDB_HNSW_TABLE_QT=8)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_hnsw_upper_layer_options(ctx, hnsw_case, opts):
    """the upper-layer table kernel's queries per pass, the lane = query table kernel from batch 1 / never, no table path at all,
    the five-register beam at every ef: rows and (distance_evals, expanded_nodes) equal the oracle's, at batches 9 and 40"""
    g, o, q = hnsw_case
    for b in (9, 40):
        for k, ef in [(10, 100), (10, 200), (5, 8), (20, 256)]:
            want = o.ann_search(q[:b], k, ef)
            evals, expanded = o.stats()
            with options(ctx, **opts):
                got = g.ann_search(q[:b], k, ef)
            st = ctx.stats()
            assert_result_rows(got, want, b)
            assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (b, k, ef)


# ----------------------------------------------------------------------------------- SPANN closure and remap (mdb_hnsw.hip, mdb_ivf.hip)
@pytest.fixture(scope="module")
def spann_case(oracle):
    from muopdb_amd.index import ProductQuantizer
    n, d = 4000, 32
    v = H.sift_like(n, d, n_clusters=30, seed=16)
    cb = H.train_pq_codebook(v[:1500], 8, 6, iters=3)
    opq = oracle.ProductQuantizer(d, 8, 6, cb)
    files, _, _ = H.build_spann_files(oracle, v, list(range(n)), 40, quantize=opq.quantize, max_neighbors=8, max_layers=3,
                                      ef_construction=50)
    q = (v[np.random.default_rng(5).integers(0, n, 300)] + np.random.default_rng(6).normal(0, 3, (300, d))).astype(np.float32)
    return dict(d=d, files=files, q=q, quant=ProductQuantizer(d, 8, 6, cb),
                oquant=oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 8, 6, cb))


@pytest.mark.parametrize("opts", [dict(MDB_CLOSURE_NO_FILTER=1), dict(MDB_CLOSURE_NO_STAGE=1), dict(MDB_CLOSURE_BLOCK=1024),
                                  dict(MDB_CLOSURE_BLOCK=256), dict(MDB_CLOSURE_NO_FILTER=1, MDB_CLOSURE_NO_STAGE=1)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
def test_spann_closure_forms(ctx, oracle, spann_case, opts):
    """hnsw_closure_kernel (centroid graphs no larger than ef): the ratio filter as a launch of its own (spann_filter_kernel), rows
    fetched round by round, the 1024-thread form at batch > 256 and the 256-thread form at batch <= 256"""
    from muopdb_amd.index import SearchParams, Spann
    f, q = spann_case["files"], spann_case["q"]
    sp = Spann(ctx, f["hnsw_index"], f["hnsw_vectors"], f["ivf_index"], f["ivf_vectors"], spann_case["quant"])
    osp = oracle.Spann(f["hnsw_index"], f["hnsw_vectors"], f["ivf_index"], f["ivf_vectors"], spann_case["oquant"])
    for ratio in (None, 0.3):
        p, op = SearchParams(10, 50).with_num_explored_centroids(8), oracle.SearchParams(10, 50, num_explored_centroids=8, **(
            {} if ratio is None else {"centroid_distance_ratio": ratio}))
        if ratio is not None:
            p = p.with_centroid_distance_ratio(ratio)
        for b in (300, 24):
            want = osp.search(q[:b], op)
            with options(ctx, **opts):
                assert_result_rows(sp.search(q[:b], p), want, b)
    sp.close()


def test_spann_device_calls_without_fused_remap(ctx, oracle, spann_case):
    """device-resident multi-user SPANN calls: the scan's merge launch remaps the rows itself, or (MDB_SCAN_NO_FUSED_REMAP) merge and
    remap as two launches — the same rows as the oracle's"""
    torch = pytest.importorskip("torch")
    from muopdb_amd import formats as F, lib as L_
    from muopdb_amd.index import MultiSpannIndex, SearchParams
    f, q = spann_case["files"], spann_case["q"][:40]
    b, k = len(q), 10
    cat = F.concat_multi_spann({5: f, 9: f})
    margs = (cat["user_table"], spann_case["d"], cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    ms = MultiSpannIndex(ctx, *margs, spann_case["quant"])
    oms = oracle.MultiSpannIndex(*margs, spann_case["oquant"])
    users = [5 if i % 2 else 9 for i in range(b)]
    p = SearchParams(k, 50).with_num_explored_centroids(8)
    want = oms.search_for_user(users, q, oracle.SearchParams(k, 50, num_explored_centroids=8))
    dev = torch.device("cuda", torch.cuda.current_device())
    qd = torch.from_numpy(q).to(dev)
    pc = p.to_c()

    def dev_call():
        ids = torch.zeros((b, k, 2), dtype=torch.int64, device=dev)
        sc = torch.zeros((b, k), dtype=torch.float32, device=dev)
        cn = torch.zeros(b, dtype=torch.int32, device=dev)
        fo = torch.zeros(b, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()   # the upload and the fills run on torch's stream, the search on the context's
        ctx.check(ctx.lib.mdb_multi_spann_search(ms.h, L_.u128_array(users), C.c_void_p(qd.data_ptr()), C.c_size_t(b), C.byref(pc),
                                                 C.c_int(L_.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                                 C.c_void_p(cn.data_ptr()), C.c_void_p(fo.data_ptr())))
        ctx.sync()
        hi = ids.cpu().numpy().view(np.uint64)
        cnt = cn.cpu().numpy()
        return ([[(int(hi[i, j, 1]) << 64) | int(hi[i, j, 0]) for j in range(int(cnt[i]))] for i in range(b)],
                sc.cpu().numpy(), cnt, fo.cpu().numpy())

    for remap in (0, 1):
        with ctx.option("MDB_SCAN_NO_FUSED_REMAP", remap):
            rows, sc, cnt, found = dev_call()
        assert np.all(found == 1)
        for i in range(b):
            c = int(want.counts[i])
            assert int(cnt[i]) == c and rows[i] == want.doc_ids(i), (remap, i)
            assert_scores(sc[i, :c], want.scores[i, :c])
    ms.close()

"""Parity of every compiled instantiation of the kernel templates (-m gpu).  tests/test_gpu_dispatch.py forces every kernel FORM;
the forms are templates, and the dispatch picks a compile-time instantiation from the metric, the PQ subvector width, the code
words per vector, the dimension, the beam width and so on.  Each case here derives its shape from the dispatch condition that
selects one instantiation (named in the case id) and compares ids, counts and f32 score bits with the oracle; IVF cases compare the
scored-vector counter with the default path's, HNSW cases the traversal counters with the oracle's.  Which kernels a run of the
suite launched is recorded in tests/kernel_launch_record.json (scripts/kernel_inventory.py; tests/test_kernel_coverage.py)."""
import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_dispatch import _batch, _check_oracle, _exact, _same, _scored, _three_states, options
from tests.test_gpu_parity import _ivf_case, assert_result_rows, assert_scores

pytestmark = pytest.mark.gpu

L2, DOT = 0, 1


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------------- PQ posting-list scans (mdb_ivf.hip)
# The scans are compiled for SUBDIM in {4, 8, 16, 32} x MW (code words of four one-byte codes per vector) in {1, 2, 4, 8}.  A cell's
# natural shape is m = 4 MW subspaces of 8-bit codes, d = SUBDIM * 4 * MW (16 .. 1024).  ivf_scan_pq2_kernel and the two-phase scan
# keep the codebook (d * K * 4 bytes) in LDS, so with 8-bit codes they serve the cells of SUBDIM * MW <= 32 (d <= 128) only; the
# wider cells reach them with fewer bits per code (FULL = false by shape), and reach the generic ivf_scan_pq_kernel with 8.
SUBDIMS, MWS = (4, 8, 16, 32), (1, 2, 4, 8)
GRID = [(sd, mw) for sd in SUBDIMS for mw in MWS]


def _fits_lds(sd, mw):
    return sd * mw <= 32


def _narrow_bits(sd, mw):
    """most bits per code whose codebook (d * 2^bits * 4 bytes) stays at 64 KB: 6 at d = 256, 5 at 512, 4 at 1024"""
    return {256: 6, 512: 5, 1024: 4}[sd * 4 * mw]


class _Cell:
    """one index file of n = 3000 rows in 12 lists (or `L` given centroids), read under both metrics; the last 60 rows repeat the
    first 60, and the first queries sit on them: equal scores under either metric"""

    def __init__(self, oracle, ctx, sd, mw, bits, L=12, n=3000):
        from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
        self.sd, self.mw, self.bits, self.n = sd, mw, bits, n
        self.d = d = sd * 4 * mw
        seed = 1000 * sd + 10 * mw + bits
        rng = np.random.default_rng(seed)
        if L <= 64:
            v = H.sift_like(n, d, n_clusters=6, seed=seed)
            cent = H.kmeans(v, L, iters=2, seed=seed)
        else:   # (a coarse quantizer the matrix-core search serves: rows around given centroids, as test_gpu_dispatch's fused_case)
            cent = H.sift_like(L, d, n_clusters=32, seed=seed)
            v = (cent[rng.integers(0, L, n)] + rng.normal(0, 3.0, (n, d))).astype(np.float32)
        v[n - 60:] = v[:60]
        self.v = v
        doc_ids = [100 + 3 * i + ((i % 7) << 70) for i in range(n)]
        cb = H.train_pq_codebook(v[:1000], sd, bits, iters=1)
        opq = oracle.ProductQuantizer(d, sd, bits, cb)
        index, vec, _ = H.build_ivf_files(v, doc_ids, cent, quantize=opq.quantize)
        self.o = {m: oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_PQ, m, sd, bits, cb)) for m in (L2, DOT)}
        self.g = {m: BlockBasedIvf(ctx, index, vec, ProductQuantizer(d, sd, bits, cb, m)) for m in (L2, DOT)}

    def queries(self, b, seed):
        q = _batch(self.v, b, seed, self.d)
        t = min(6, b)
        q[:t] = self.v[:t]
        return q


_cells = {}


@pytest.fixture(scope="module")
def cell(oracle, ctx):
    """cells by (SUBDIM, MW, bits, lists): one codebook and one index file serve every case of a cell"""
    def get(sd, mw, bits=8, L=12):
        key = (sd, mw, bits, L)
        if key not in _cells:
            _cells[key] = _Cell(oracle, ctx, sd, mw, bits, L)
        return _cells[key]
    yield get
    for c in _cells.values():
        for g in c.g.values():
            g.close()
    _cells.clear()


def _one_phase_cases(metric, full_by_option):
    cases = [dict()]
    if metric == L2:
        cases.append(dict(MDB_PQ_NO_FILTER=1))
    if full_by_option:
        cases.append(dict(MDB_PQ_NO_FULL=1))
        if metric == L2:
            cases.append(dict(MDB_PQ_NO_FULL=1, MDB_PQ_NO_FILTER=1))
    return cases


@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
@pytest.mark.parametrize("sd,mw", GRID, ids=["sd%d-mw%d" % c for c in GRID])
def test_pq_one_phase_scan_grid(ctx, oracle, cell, sd, mw, metric):
    """the unfused one-phase step (MDB_PQ_NO_FUSED) of every (SUBDIM, MW) cell under both metrics.  8-bit codes: cells whose codebook
    fits LDS take ivf_scan_pq2_kernel<METRIC, SUBDIM, MW, FILT, FULL> — FILT: the L2 bound filter, off with MDB_PQ_NO_FILTER and under
    dot; FULL: whole-word codes, off with MDB_PQ_NO_FULL — the wider ones the generic ivf_scan_pq_kernel<METRIC, false> (table in
    HBM).  The wider cells then take ivf_scan_pq2_kernel<.., FULL = false> by shape, with 4- to 6-bit codes.  MDB_PQ_NO_FAST: the
    generic kernel on every cell, its table in LDS where it fits 150 KB.  Batches 24 (several splits per query) and 1100 (one)."""
    k, P = 10, 6
    runs = [(cell(sd, mw), _one_phase_cases(metric, _fits_lds(sd, mw)) + [dict(MDB_PQ_NO_FAST=1)])]
    if not _fits_lds(sd, mw):
        runs.append((cell(sd, mw, _narrow_bits(sd, mw)), _one_phase_cases(metric, False) + [dict(MDB_PQ_NO_FAST=1)]))
    if (sd, mw) == (4, 8):   # 32 subspaces: the bound filter's table fits beside a 7-bit codebook, not beside the 8-bit one (below)
        runs.append((cell(sd, mw, 7), _one_phase_cases(metric, False)))
    for c, cases in runs:
        o, g = c.o[metric], c.g[metric]
        q = c.queries(24, mw)
        want = o.search(q, k, num_probes=P)
        with ctx.option("MDB_PQ_NO_FUSED", 1):
            ref_scored = None
            for opts in cases:
                with options(ctx, **opts):
                    assert_result_rows(g.search(q, k, P), want, len(q))
                ref_scored = _scored(ctx) if ref_scored is None else ref_scored
                assert _scored(ctx) == ref_scored > 0, (c.bits, opts)
            # one split per query (the rows written in place, no merge launch) and no two-phase scan in front of it
            qb = c.queries(1100, sd)
            sel = np.r_[0:16, 1084:1100]
            wb = o.search(qb[sel], k, num_probes=P)
            with ctx.option("MDB_PQ_NO_TWO_PHASE", 1):
                got = g.search(qb, k, P)
            for j, i in enumerate(sel):
                assert got.doc_ids(int(i)) == wb.doc_ids(j), (c.bits, i)
                assert_scores(got.scores[i, :int(got.counts[i])], wb.scores[j, :int(wb.counts[j])])
            if metric == L2:   # every row against the default (two-phase) path
                dflt = g.search(qb, k, P)
                assert H.result_rows(got, len(qb)) == H.result_rows(dflt, len(qb))
            else:              # dot has one path: every row against the same scan at 100 queries a call (splits + merge launch)
                rows = H.result_rows(got, len(qb))
                for s0 in range(0, len(qb), 100):
                    part = H.result_rows(g.search(qb[s0:s0 + 100], k, P), 100)
                    assert (rows[0][s0:s0 + 100], rows[1][s0:s0 + 100]) == part, s0


def test_pq_one_phase_scan_widest_filtered_cell_k0(ctx, oracle, cell):
    """ivf_scan_pq2_kernel<0, 4, 8, true, true>: 128 KB of codebook and 16 KB of bound table leave the selector 11 KB, which it
    needs for k = 0 only (k >= 1: 16 KB, and the cell scans without the filter).  There are no rows to compare: the call returns
    empty rows as the oracle does, with and without the filter, and the next search is unaffected."""
    c = cell(4, 8)
    o, g = c.o[L2], c.g[L2]
    q = c.queries(24, 3)
    with ctx.option("MDB_PQ_NO_FUSED", 1):
        for opts in (dict(), dict(MDB_PQ_NO_FILTER=1)):
            with options(ctx, **opts):
                got = g.search(q, 0, 6)
            assert got.counts.tolist() == [0] * len(q) == o.search(q, 0, num_probes=6).counts.tolist()
        assert_result_rows(g.search(q, 10, 6), o.search(q, 10, num_probes=6), len(q))


@pytest.mark.parametrize("sd,mw", GRID, ids=["sd%d-mw%d" % c for c in GRID])
def test_pq_two_phase_scan_grid(ctx, oracle, cell, sd, mw):
    """ivf_scan_pq3_kernel<MW, BLOCK, FULL> + ivf_pq3_refine_kernel<SUBDIM, MW, FULL> (L2 only) on every cell, at both block sizes:
    from batch 1 on (MDB_PQ_TWO_PHASE_MIN_B=1, 40 queries) and by the default threshold (520 queries).  FULL with 8-bit codes on the
    cells whose codebook fits LDS (and MDB_PQ_NO_FULL there); the wider cells by shape, with 4- to 6-bit codes."""
    k, P = 10, 6
    fits = _fits_lds(sd, mw)
    c = cell(sd, mw) if fits else cell(sd, mw, _narrow_bits(sd, mw))
    o, g = c.o[L2], c.g[L2]
    q = c.queries(40, 7 + mw)
    want = o.search(q, k, num_probes=P)
    with ctx.option("MDB_PQ_NO_FUSED", 1):
        assert_result_rows(g.search(q, k, P), want, len(q))
        ref_scored = _scored(ctx)
    for blk in (512, 1024):
        for full in ((0, 1) if fits else (0,)):
            for cap in (2048, 8):   # (8 slots: every list overflows, the gated one-phase launch redoes the batch)
                with options(ctx, MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1, MDB_PQ3_BLOCK=blk, MDB_PQ_NO_FULL=full, MDB_PQ3_CAP=cap):
                    assert_result_rows(g.search(q, k, P), want, len(q))
                assert _scored(ctx) == ref_scored > 0, (blk, full, cap)
    qb = c.queries(520, 9 + sd)
    sel = np.r_[0:16, 504:520]
    wb = o.search(qb[sel], k, num_probes=P)
    with ctx.option("MDB_PQ_NO_TWO_PHASE", 1):
        one = g.search(qb, k, P)
    for blk in (512, 1024):
        with ctx.option("MDB_PQ3_BLOCK", blk):
            got = g.search(qb, k, P)
        assert H.result_rows(got, len(qb)) == H.result_rows(one, len(qb)), blk
        for j, i in enumerate(sel):
            assert got.doc_ids(int(i)) == wb.doc_ids(j), (blk, i)
            assert_scores(got.scores[i, :int(got.counts[i])], wb.scores[j, :int(wb.counts[j])])


def _cm_dim_ok(d):
    return d in (64, 96, 128, 192, 256)


@pytest.mark.parametrize("sd,mw", GRID, ids=["sd%d-mw%d" % c for c in GRID])
def test_pq_fused_step_grid(ctx, oracle, cell, sd, mw):
    """ivf_pq_fused_kernel<SUBDIM, MW, COARSE> on every cell (8-bit codes, L2): COARSE 0 with the caller's probes, 1 with the
    distances of ivf_prep_kernel (12 centroids), 2 behind the matrix-core coarse search, which serves 1 024 .. 16 384 centroids of
    d = 64 / 96 / 128 / 192 / 256 — ten of the sixteen cells; the dispatch instantiates COARSE = 2 for those only.  Candidate lists
    of 2 048 and of 8 slots (every block overflows into its exact pass); the scored-vector counter equals the unfused step's."""
    k = 10
    shapes = [(cell(sd, mw), 6)]
    if _cm_dim_ok(sd * 4 * mw):
        shapes.append((cell(sd, mw, 8, 1024), 16))
    for c, P in shapes:
        o, g = c.o[L2], c.g[L2]
        q = c.queries(24, 11 + mw)
        want = o.search(q, k, num_probes=P)
        probes = o.find_nearest_centroids(q, P)
        with ctx.option("MDB_PQ_NO_FUSED", 1):
            assert_result_rows(g.search(q, k, P), want, len(q))
            ref_scored = _scored(ctx)
        for cap in (2048, 8):
            with options(ctx, MDB_PQF_CAP=cap, MDB_IVF_COARSE_MFMA_MIN_B=1):
                assert np.array_equal(g.find_nearest_centroids(q, P), probes)
                assert_result_rows(g.search(q, k, P), want, len(q))                       # COARSE 1 (12 lists) / 2 (1 024 lists)
                assert _scored(ctx) == ref_scored > 0, cap
                assert_result_rows(g.search_with_centroids_and_remap(q, probes, k), want, len(q))   # COARSE 0
                assert _scored(ctx) == ref_scored, cap
                assert_result_rows(g.search(q[:7], k, P), o.search(q[:7], k, num_probes=P), 7)
        if len(shapes) == 2 and c is shapes[1][0]:
            with ctx.option("MDB_IVF_COARSE_MFMA", 0):   # the 1 024-list index through ivf_prep_kernel's distances
                assert_result_rows(g.search(q, k, P), want, len(q))
                assert _scored(ctx) == ref_scored


# masks: the tombstone / allow reads are not template-dependent beyond `no_masks`, so one dot cell per scan form and the
# narrowest and widest L2 cell of each form
MASK_CASES = [("dot-pq2-sd8-mw2", DOT, 8, 2, 8, dict(MDB_PQ_NO_FUSED=1), 24),
              ("dot-pq2-narrow-sd16-mw8", DOT, 16, 8, 5, dict(MDB_PQ_NO_FUSED=1), 24),
              ("dot-generic-lds-sd8-mw2", DOT, 8, 2, 8, dict(MDB_PQ_NO_FAST=1), 24),
              ("dot-generic-hbm-sd32-mw8", DOT, 32, 8, 8, dict(), 24),
              ("l2-pq2-sd4-mw1", L2, 4, 1, 8, dict(MDB_PQ_NO_FUSED=1), 24),
              ("l2-pq2-narrow-sd32-mw8", L2, 32, 8, 4, dict(MDB_PQ_NO_FUSED=1), 24),
              ("l2-generic-hbm-sd32-mw8", L2, 32, 8, 8, dict(MDB_PQ_NO_FUSED=1), 24),
              ("l2-two-phase-sd4-mw1", L2, 4, 1, 8, dict(MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1), 40),
              ("l2-two-phase-narrow-sd32-mw8", L2, 32, 8, 4, dict(MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1), 40),
              ("l2-fused-sd4-mw1", L2, 4, 1, 8, dict(), 24),
              ("l2-fused-sd32-mw8", L2, 32, 8, 8, dict(), 24)]


@pytest.mark.parametrize("name,metric,sd,mw,bits,opts,b", MASK_CASES, ids=[c[0] for c in MASK_CASES])
def test_pq_scan_masks_on_new_cells(ctx, oracle, name, metric, sd, mw, bits, opts, b):
    """clean index, shared filter, per-query filters, tombstones — each with and without MDB_SCAN_MASKS_ALWAYS"""
    d, n = sd * 4 * mw, 3000
    o, g, q, v, _ = _ivf_case(oracle, ctx, n, d, 12, seed=sd + mw + bits, quant=(sd, bits), metric=metric)
    q = _batch(v, b, 5, d)
    with options(ctx, **opts):
        _three_states(ctx, oracle, o, g, q, 10, 6, n)
    g.close()


# ----------------------------------------------------------------------------------- dot-metric PQ lists through SPANN
@pytest.fixture(scope="module")
def dot_spann(oracle):
    """SPANN over PQ posting lists read under the dot metric (the centroid graph is always L2: mdb_spann.hip, spann/index.rs:19;
    the lists take the quantizer's metric in the loader and in the oracle).  8-bit codes of 8 subspaces (ivf_scan_pq2_kernel<1, 8, 2>)
    and 6-bit codes (FULL = false)."""
    from muopdb_amd.index import ProductQuantizer
    n, d = 4000, 64
    v = H.sift_like(n, d, n_clusters=30, seed=17)
    v[n - 50:] = v[:50]
    out = {}
    for bits in (8, 6):
        cb = H.train_pq_codebook(v[:1000], 8, bits, iters=1)
        opq = oracle.ProductQuantizer(d, 8, bits, cb)
        files, _, _ = H.build_spann_files(oracle, v, list(range(n)), 40, quantize=opq.quantize, max_neighbors=8, max_layers=3,
                                          ef_construction=50)
        out[bits] = dict(files=files, quant=ProductQuantizer(d, 8, bits, cb, DOT), oquant=oracle.Quant(oracle.QUANT_PQ, DOT, 8, bits, cb))
    q = (v[np.random.default_rng(5).integers(0, n, 300)] + np.random.default_rng(6).normal(0, 3, (300, d))).astype(np.float32)
    q[:8] = v[:8]
    return dict(d=d, q=q, cases=out)


@pytest.mark.parametrize("bits", [8, 6])
@pytest.mark.parametrize("opts", [dict(), dict(MDB_PQ_NO_FAST=1), dict(MDB_PQ_NO_FULL=1)], ids=["default", "generic", "no_full"])
def test_dot_metric_pq_spann(ctx, oracle, dot_spann, bits, opts):
    """Spann and MultiSpannIndex with dot-metric PQ lists: ivf_scan_pq2_kernel<1, ..> and ivf_scan_pq_kernel<1, true> behind the
    centroid traversal and the ratio filter, at batches 300 and 24"""
    from muopdb_amd import formats as F
    from muopdb_amd.index import MultiSpannIndex, SearchParams, Spann
    cs, q = dot_spann["cases"][bits], dot_spann["q"]
    f = cs["files"]
    sp = Spann(ctx, f["hnsw_index"], f["hnsw_vectors"], f["ivf_index"], f["ivf_vectors"], cs["quant"])
    osp = oracle.Spann(f["hnsw_index"], f["hnsw_vectors"], f["ivf_index"], f["ivf_vectors"], cs["oquant"])
    p, op = SearchParams(10, 50).with_num_explored_centroids(8), oracle.SearchParams(10, 50, num_explored_centroids=8)
    pr = SearchParams(10, 50).with_num_explored_centroids(8).with_centroid_distance_ratio(0.3)
    opr = oracle.SearchParams(10, 50, num_explored_centroids=8, centroid_distance_ratio=0.3)
    for b in (300, 24):
        for pp, oo in ((p, op), (pr, opr)):
            want = osp.search(q[:b], oo)
            with options(ctx, **opts):
                assert_result_rows(sp.search(q[:b], pp), want, b)
    sp.close()
    cat = F.concat_multi_spann({5: f, 9: f})
    margs = (cat["user_table"], dot_spann["d"], cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    ms = MultiSpannIndex(ctx, *margs, cs["quant"])
    oms = oracle.MultiSpannIndex(*margs, cs["oquant"])
    users = [5 if i % 2 else 9 for i in range(40)]
    want = oms.search_for_user(users, q[:40], op)
    with options(ctx, **opts):
        assert_result_rows(ms.search_for_user(users, q[:40], p), want, 40)
    ms.close()


# ----------------------------------------------------------------------------------- HNSW layer 0 (mdb_hnsw.hip)
# hnsw_beam_kernel<METRIC, VIS_LDS, N16T, ROW64, L0, NB> / hnsw_search_kernel<METRIC, VIS_LDS, N16T>.  N16T: 8 at d = 128, 48 at
# d = 768, 0 at every other dimension.  VIS_LDS: the visited bitmap in LDS — false from ~1.19 M points on (148 KB of bitmap).
# L0 (behind the upper-layer table path, which wants an upper layer): NB 4 while ef + MDB_HNSW_NB4_SLACK <= 256, 5 up to ef = 256,
# 8 up to 448.  Not L0: MDB_HNSW_NO_TABLE (ROW64) and MDB_HNSW_NO_ROW64.  General kernel: MDB_HNSW_NO_BEAM.
HNSW_FORMS = [("nb4-ef64", 64, dict()), ("nb4-ef200", 200, dict()), ("nb5-ef230", 230, dict()), ("nb5-slack0-ef64", 64, dict(MDB_HNSW_NB4_SLACK=0)),
              ("nb8-ef300", 300, dict()), ("no_table-row64-ef100", 100, dict(MDB_HNSW_NO_TABLE=1)),
              ("no_row64-ef100", 100, dict(MDB_HNSW_NO_ROW64=1)), ("general-ef100", 100, dict(MDB_HNSW_NO_BEAM=1)),
              ("general-ef300", 300, dict(MDB_HNSW_NO_WIDE=1)), ("general-ef600", 600, dict())]


def _hnsw_pair(oracle, ctx, index, vf, d, metric):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    return (BlockBasedHnsw(ctx, index, vf, d, NoQuantizer(d, metric)),
            oracle.BlockBasedHnsw(index, vf, d, oracle.Quant(oracle.QUANT_NONE, metric)))


def _nf(d):
    """N16T of the layer-0 kernels"""
    return {768: 48, 128: 8}.get(d, 0)


def _tf(v):
    return "true" if v else "false"


def _l0_key(form, d, metric, vis_lds):
    """the layer-0 kernel key of a form of HNSW_FORMS, written out from the comment above them"""
    head = "%d, %s, %d" % (metric, _tf(vis_lds), _nf(d))
    nb = {"nb4-ef64": 4, "nb4-ef200": 4, "nb5-ef230": 5, "nb5-slack0-ef64": 5, "nb8-ef300": 8}.get(form)
    if nb:
        return "hnsw_beam_kernel<%s, true, true, %d>" % (head, nb)
    if form.startswith("general"):
        return "hnsw_search_kernel<%s>" % head
    return "hnsw_beam_kernel<%s, %s, false, 5>" % (head, _tf(form.startswith("no_table")))


def _hnsw_check(ctx, g, o, q, k, ef, opts, keys=None):
    """keys: the kernel keys mdb_hnsw_describe_search names for this call under `opts`, in launch order (a str: the last one's)"""
    o.stats()
    want = o.ann_search(q, k, ef)
    evals, expanded = o.stats()
    ctx.stats()
    with options(ctx, **opts):
        got = g.ann_search(q, k, ef)
        described = [key for _, key, _, _, _ in g.describe_search(len(q), k, ef)[1]]
    if keys is not None:
        assert (described[-1] if isinstance(keys, str) else described) == keys, (ef, opts, described)
    st = ctx.stats()
    assert_result_rows(got, want, len(q))
    assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (ef, opts)


@pytest.fixture(scope="module", params=[768, 128, 100], ids=lambda d: "d%d" % d)
def hnsw_graph(request, oracle):
    """3 000 points (far more than any ef below: the beam kernels traverse it, not the closure kernel), built by the oracle's builder
    under L2; unit rows, so that the dot metric ranks them sensibly too"""
    d = request.param
    n = 3000
    v = H.sift_like(n, d, n_clusters=20, seed=d)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    v[n - 30:] = v[:30]
    hidx, hvec = H.build_hnsw_files(oracle, v, list(range(n)), max_neighbors=12, max_layers=4, ef_construction=40)
    rng = np.random.default_rng(d)
    q = (v[rng.integers(0, n, 20)] + rng.normal(0, 0.02, (20, d))).astype(np.float32)
    q[:3] = v[:3]
    return d, hidx, hvec, q


@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
@pytest.mark.parametrize("form,ef,opts", HNSW_FORMS, ids=[f[0] for f in HNSW_FORMS])
def test_hnsw_layer0_forms_lds_visited(ctx, oracle, hnsw_graph, form, ef, opts, metric):
    """every layer-0 form at N16T = 48 / 8 / 0 under both metrics, visited set in LDS: rows and traversal counters equal the oracle's"""
    d, hidx, hvec, q = hnsw_graph
    g, o = _hnsw_pair(oracle, ctx, hidx, hvec, d, metric)
    for b in (20, 3):
        _hnsw_check(ctx, g, o, q[:b], 10, ef, opts, _l0_key(form, d, metric, True))
    g.close()


def _ring_layer(rng, pts):
    """a connected layer over `pts`: both ring neighbours and four random members"""
    m = len(pts)
    nb = np.stack([np.roll(pts, -1), np.roll(pts, 1)] + [pts[rng.integers(0, m, m)] for _ in range(4)], 1)
    return {int(p): [int(x) for x in row] for p, row in zip(pts, nb)}


@pytest.fixture(scope="module", params=[768, 128, 4], ids=lambda d: "d%d" % d)
def hnsw_big_graph(request):
    """1 220 000 points: above ~1.19 M (d = 768) / ~1.21 M (d = 4) the visited bitmap no longer fits LDS beside the beam kernel's
    fixed layout.  A cheap valid graph, as test_hnsw_large_graph_uses_hbm_visited builds it (ring + random long links: parity needs
    no quality), with two small upper layers so that the table path and its layer-0 instances run."""
    from muopdb_amd import formats as F
    d = request.param
    n = 1_220_000
    rng = np.random.default_rng(d)
    v = rng.random((n, d), dtype=np.float32)
    ar = np.arange(n)
    nb = np.stack([(ar + 1) % n, (ar - 1) % n, rng.integers(0, n, n), rng.integers(0, n, n)], 1)
    indptr = np.arange(n + 1, dtype=np.uint64) * 4
    p1 = np.arange(0, n, n // 300)[:300]
    layers = [(None, indptr, nb.reshape(-1).astype(np.uint32)), _ring_layer(rng, p1), _ring_layer(rng, p1[::12])]
    index = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d)
    vf = F.write_vector_file(v)
    q = rng.random((6, d), dtype=np.float32)
    q[0] = v[12345]
    del v, nb
    return d, index, vf, q


@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
def test_hnsw_layer0_forms_hbm_visited(ctx, oracle, hnsw_big_graph, metric):
    """the same forms with the visited set in HBM (VIS_LDS = false), at N16T = 48 / 8 / 0"""
    d, index, vf, q = hnsw_big_graph
    g, o = _hnsw_pair(oracle, ctx, index, vf, d, metric)
    for form, ef, opts in HNSW_FORMS:
        _hnsw_check(ctx, g, o, q, 10, ef, opts, _l0_key(form, d, metric, False))
    g.close()


@pytest.mark.parametrize("d", [768, 128, 100])
def test_hnsw_closure_forms_dot(ctx, oracle, d):
    """hnsw_closure_kernel<METRIC, N16T, BLOCK> (graphs no larger than ef) under both metrics: the 1024-thread form at batch <= 256,
    the 256-thread form beyond (and by MDB_CLOSURE_BLOCK)"""
    n = 150
    v = H.sift_like(n, d, n_clusters=5, seed=d + 1)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    hidx, hvec = H.build_hnsw_files(oracle, v, list(range(n)), max_neighbors=8, max_layers=3, ef_construction=40)
    rng = np.random.default_rng(d)
    q = (v[rng.integers(0, n, 300)] + rng.normal(0, 0.02, (300, d))).astype(np.float32)
    for metric in (L2, DOT):
        g, o = _hnsw_pair(oracle, ctx, hidx, hvec, d, metric)
        _hnsw_check(ctx, g, o, q[:40], 10, 200, dict(), ["hnsw_closure_kernel<%d, %d, 1024>" % (metric, _nf(d))])
        _hnsw_check(ctx, g, o, q[:40], 10, 200, dict(MDB_CLOSURE_BLOCK=256), ["hnsw_closure_kernel<%d, %d, 256>" % (metric, _nf(d))])
        _hnsw_check(ctx, g, o, q, 10, 200, dict(), ["hnsw_closure_kernel<%d, %d, 256>" % (metric, _nf(d))])
        g.close()


# ----------------------------------------------------------------------------------- HNSW upper layers (mdb_hnsw_upper.hip)
@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
@pytest.mark.parametrize("n16", [1, 2, 3, 4, 5, 6, 7, 8])
def test_hnsw_upper_layer_kernels_by_dimension(ctx, oracle, n16, metric):
    """the lane = query kernels are compiled per 16-chunk count (d = 16 .. 128), at batch >= MDB_HNSW_TABLE64_MIN_B (32) on a graph
    with two upper layers: hnsw_upper_top_rank_kernel<METRIC, N16, 1> by default (at most 2 048 points above layer 1) — in the frontier
    form whatever MDB_HNSW_RANK says —, hnsw_upper_top_kernel<METRIC, N16, 4 | 5> with MDB_HNSW_RANK=0 and MDB_HNSW_CLOSURE=0
    (ef + 48 <= 256 | beyond), hnsw_upper_table64_kernel<METRIC, N16> with MDB_HNSW_NO_SPLIT.  The route (mdb_hnsw_describe_search)
    names exactly these; under the dot metric d = 16 is a remainder chunk (n16 = 0): the generic table kernel, no top launch."""
    d, n = 16 * n16, 2500
    v = H.sift_like(n, d, n_clusters=16, seed=n16)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    hidx, hvec = H.build_hnsw_files(oracle, v, list(range(n)), max_neighbors=8, max_layers=4, ef_construction=40)
    g, o = _hnsw_pair(oracle, ctx, hidx, hvec, d, metric)
    rng = np.random.default_rng(n16)
    q = (v[rng.integers(0, n, 40)] + rng.normal(0, 0.03, (40, d))).astype(np.float32)
    whole16 = not (metric == DOT and n16 == 1)
    m_n = "%d, %d" % (metric, n16)
    for ef in (100, 230):
        nb = 4 if ef + 48 <= 256 else 5
        rank1, upper = "hnsw_upper_rank_kernel<1>", "hnsw_upper_kernel<true, %d>" % nb
        l0 = "hnsw_beam_kernel<%d, true, %d, true, true, %d>" % (metric, _nf(d), nb)
        table = "hnsw_upper_table64_kernel<%s>" % m_n if whole16 else "hnsw_upper_table_kernel<1, 2>"
        top = "hnsw_upper_top_rank_kernel<%s, 1>" % m_n if whole16 else table
        top_beam = "hnsw_upper_top_kernel<%s, %d>" % (m_n, nb) if whole16 else table
        for opts, keys in ((dict(), [top, rank1, upper, l0]), (dict(MDB_HNSW_RANK=0), [top, rank1, upper, l0]),
                           (dict(MDB_HNSW_NO_SPLIT=1), [table, rank1, upper, l0]),
                           (dict(MDB_HNSW_RANK=0, MDB_HNSW_NO_SPLIT=1), [table, rank1, upper, l0]),
                           (dict(MDB_HNSW_CLOSURE=0), [top, upper, l0]), (dict(MDB_HNSW_RANK=0, MDB_HNSW_CLOSURE=0), [top_beam, upper, l0])):
            _hnsw_check(ctx, g, o, q, 10, ef, opts, keys)
    g.close()


@pytest.mark.parametrize("n16", [1, 2, 3, 4, 5, 6, 7, 8])
def test_hnsw_upper_rank_kernels_wide_top(ctx, oracle, n16):
    """more than 2 048 points above layer 1 (2 500 of 6 000 upper-layer points, 40 000 in all): hnsw_upper_top_rank_kernel<METRIC,
    N16, 4> under both metrics (the sequential form, MDB_HNSW_CLOSURE=0: the frontier form's top launch is the <.., 1> instance, its
    blocks then leave the flagged queries to the fallback launch), and hnsw_upper_rank_kernel<4> (MDB_HNSW_RANK=3: 2 049 .. 8 192
    upper-layer points) behind it.  The route (mdb_hnsw_describe_search) names exactly these."""
    from muopdb_amd import formats as F
    d, n = 16 * n16, 40_000
    rng = np.random.default_rng(100 + n16)
    v = rng.random((n, d), dtype=np.float32)
    ar = np.arange(n)
    nb = np.stack([(ar + 1) % n, (ar - 1) % n] + [rng.integers(0, n, n) for _ in range(4)], 1)
    layers = [(None, np.arange(n + 1, dtype=np.uint64) * 6, nb.reshape(-1).astype(np.uint32)),
              _ring_layer(rng, np.arange(6000)), _ring_layer(rng, np.arange(2500)), _ring_layer(rng, np.arange(40))]
    index, vf = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d), F.write_vector_file(v)
    q = (v[rng.integers(0, n, 40)] + rng.normal(0, 0.02, (40, d))).astype(np.float32)
    for metric in (L2, DOT):
        g, o = _hnsw_pair(oracle, ctx, index, vf, d, metric)
        whole16 = not (metric == DOT and n16 == 1)
        table = "hnsw_upper_table_kernel<1, 2>"
        top1, top4 = [("hnsw_upper_top_rank_kernel<%d, %d, %d>" % (metric, n16, nw)) if whole16 else table for nw in (1, 4)]
        rank1, rank4, upper = "hnsw_upper_rank_kernel<1>", "hnsw_upper_rank_kernel<4>", "hnsw_upper_kernel<true, 4>"
        l0 = "hnsw_beam_kernel<%d, true, %d, true, true, 4>" % (metric, _nf(d))
        for opts, keys in ((dict(), [top1, rank1, upper, l0]), (dict(MDB_HNSW_RANK=3), [top1, rank1, rank4, l0]),
                           (dict(MDB_HNSW_CLOSURE=0), [top4, upper, l0]), (dict(MDB_HNSW_CLOSURE=0, MDB_HNSW_RANK=3), [top4, rank4, l0])):
            _hnsw_check(ctx, g, o, q, 10, 100, opts, keys)
        g.close()


def test_select_neighbors_heuristic_dot(ctx, oracle):
    """hnsw_select_kernel<1>: the builder's neighbour selection under the dot metric (tests/test_gpu_build.py restates it for L2)"""
    from muopdb_amd import build as B
    rng = np.random.default_rng(9)
    n, d, M, W = 600, 24, 8, 40
    x = H.sift_like(n, d, n_clusters=6, seed=5)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x[100] = x[7]; x[200] = x[7]
    cand = np.full((50, W), 0xFFFFFFFF, np.uint32)
    dist = np.full((50, W), np.inf, np.float32)
    for r in range(50):
        c = rng.choice(n, size=int(rng.integers(1, W + 1)), replace=False)
        if r % 5 == 0:
            c = np.unique(np.concatenate([c[:W - 3], [7, 100, 200]]))[:W]
        dd = np.array([oracle.dot(x[r], x[j]) for j in c], np.float32)
        order = np.lexsort((-c.astype(np.int64), dd))
        cand[r, :len(c)], dist[r, :len(c)] = c[order], dd[order]
    ids, ds, cnt = B.select_neighbors(ctx, x, cand, dist, M, metric=DOT)
    for r in range(50):
        kept = []
        for j in range(W):
            e = int(cand[r, j])
            if e == 0xFFFFFFFF or len(kept) == M:
                break
            if all(not (np.float32(oracle.dot(x[e], x[k_])) < dist[r, j]) for k_, _ in kept):
                kept.append((e, dist[r, j]))
        assert int(cnt[r]) == len(kept) and ids[r, :len(kept)].tolist() == [e for e, _ in kept]
        assert np.array_equal(ds[r, :len(kept)].view(np.uint32), np.array([v for _, v in kept], np.float32).view(np.uint32))


# ----------------------------------------------------------------------------------- flat exact kernels (mdb_flat.hip)
@pytest.mark.parametrize("n16", [1, 2, 3, 4, 5, 6, 7, 8])
def test_flat_small_base_kernels_by_dimension(ctx, oracle, n16):
    """bases of at most 1 024 tiles, batches of at most 4, d = 16 N16: flat_small_scan_kernel<METRIC, N16, SORTED> (sorted lists by
    default, unordered keys with MDB_FLAT_NO_SMALL=2) and the one-launch flat_small_block_kernel<METRIC, N16> (MDB_FLAT_NO_SMALL=4,
    k <= 16) for L2 and dot through FlatIndex, and for the squared L2 of the IVF builder's assignment (METRIC 2) through ivf_assign
    with at most 4 vectors"""
    from muopdb_amd.index import FlatIndex, ivf_assign
    d, n = 16 * n16, 3001
    rng = np.random.default_rng(n16)
    base = np.rint(rng.standard_normal((n, d)) * 3).astype(np.float32)
    base[n - 20:] = base[:20]                               # ties
    q = (base[rng.integers(0, n, 4)] + rng.normal(0, 1, (4, d))).astype(np.float32)
    q[0] = base[3]
    for metric in (L2, DOT):
        idx = FlatIndex(ctx, base, metric)
        for b in (1, 3, 4):
            for k in (1, 16, 64):
                oids, odist = oracle.flat_topk(metric, base, q[:b], k)
                for mode in (0, 2, 4):
                    with ctx.option("MDB_FLAT_NO_SMALL", mode):
                        ids, dist, counts = idx.search(q[:b], k)
                    assert counts.tolist() == [k] * b and np.array_equal(ids, oids), (metric, b, k, mode)
                    assert_scores(dist, odist)
    cent = base[:2000]
    for b in (1, 4):
        for mc in (1, 8, 16):
            want = oracle.ivf_assign(cent, q[:b], mc, 0.5)
            for mode in (0, 2, 4):
                with ctx.option("MDB_FLAT_NO_SMALL", mode):
                    ids, cnt = ivf_assign(ctx, cent, q[:b], mc, 0.5)
                assert np.array_equal(cnt, want[1]) and np.array_equal(ids, want[0]), (b, mc, mode)


def test_ivf_assign_scan_queries_per_block(ctx, oracle):
    """flat_scan_kernel<2, QT> (squared L2): one vector (QT 1), and four queries per block (MDB_FLAT_QT=4; without the option a
    centroid set that stays in L2 takes two)"""
    from muopdb_amd.index import ivf_assign
    rng = np.random.default_rng(4)
    cent = H.sift_like(3000, 40, n_clusters=20, seed=4)
    v = (cent[rng.integers(0, 3000, 64)] + rng.normal(0, 3, (64, 40))).astype(np.float32)
    for b, opts in ((1, dict()), (64, dict(MDB_FLAT_QT=4)), (64, dict(MDB_FLAT_QT=1)), (64, dict())):
        want = oracle.ivf_assign(cent, v[:b], 5, 0.3)
        with options(ctx, **opts):
            ids, cnt = ivf_assign(ctx, cent, v[:b], 5, 0.3)
        assert np.array_equal(cnt, want[1]) and np.array_equal(ids, want[0]), (b, opts)


def test_lane_conforming_dot_eight_lanes(ctx, oracle):
    """lane_conforming_kernel<1, 8>"""
    rng = np.random.default_rng(8)
    for d in (8, 24, 100, 128):
        a = (rng.standard_normal((50, d)) * 10).astype(np.float32)
        b = (rng.standard_normal((50, d)) * 10).astype(np.float32)
        got = ctx.lane_conforming_distance(a, b, 8, DOT)
        want = np.array([oracle.lane_conforming(DOT, 8, a[i], b[i]) for i in range(50)], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ----------------------------------------------------------------------------------- flat batched path (mdb_flat_mfma.hip)
@pytest.fixture(scope="module")
def filter_bases():
    base = H.sift_like(65_536, 128, n_clusters=40, seed=3)
    base[65_536 - 64:] = base[:64]
    return base


@pytest.mark.parametrize("rows", [1, 0], ids=["rows", "no_rows"])
@pytest.mark.parametrize("d", [128, 96], ids=["nk8-d128", "nk0-d96"])
@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
def test_bf16_filter_instantiations(ctx, oracle, filter_bases, metric, d, rows):
    """flat_bf16_filter_kernel<METRIC, QB, NKT, SMP, APX, X1>.  QB: query blocks of 32 per block — 1 / 2 / 4 / 8 at batches up to
    32 / 64 / 128 / beyond (MDB_BF_QB=8 lifts the default cap of 4).  NKT: 8 at d = 113 .. 128, 0 elsewhere.  SMP: the pass over the
    sample that bounds the k-th distance, and the filter pass proper.  APX: the filter hands its products to the one-block-per-query
    refine, which wants the row-major copy (MDB_FLAT_ROWS, read at load).  X1: one bf16 product per pair (MDB_BF_X1=2) or three (0).
    MDB_BF_BLOCK_MIN_B keeps large batches off the block-shared kernel.  Without the row-major copy the refine runs by slices:
    flat_refine_kernel<METRIC, false, 256 | 64> (64: from MDB_REFINE_WAVE_MIN_B = 512 queries on)."""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(d + metric + rows)
    base = np.ascontiguousarray(filter_bases[:, :d])
    with options(ctx, MDB_FLAT_ROWS=rows, MDB_BF_X1=0):   # (MDB_BF_X1=0 at load: the store keeps the lo halves that three products read)
        idx = FlatIndex(ctx, base, metric)
    for b in (24, 48, 100, 200) + ((520,) if not rows else ()):
        q = (base[rng.integers(0, len(base), b)] + rng.normal(0, 10, (b, d))).astype(np.float32)
        q[:2] = base[:2]
        exact = _exact(ctx, idx, q, 10)
        _check_oracle(oracle, metric, base, q, 10, exact)
        for x1 in (0, 2):
            with options(ctx, MDB_BF_X1=x1, MDB_BF_QB=8, MDB_BF_BLOCK_MIN_B=1 << 30, MDB_MF_COOLDOWN=0):
                _same(idx.search(q, 10), exact, (b, x1))


@pytest.mark.parametrize("metric", [L2, DOT], ids=["l2", "dot"])
def test_block_filter_instantiations(ctx, oracle, filter_bases, metric):
    """flat_bf16x1_block_kernel<METRIC, QB, BOUND, APX> at batch >= 512 of d = 128: MDB_BF_BLOCK_QB 1 / 2 / 4 query blocks per wave,
    with the products handed to the group refine (APX: a store with the row-major copy) and without (MDB_FLAT_ROWS=0 at load)"""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(40 + metric)
    base = filter_bases
    q = (base[rng.integers(0, len(base), 600)] + rng.normal(0, 10, (600, 128))).astype(np.float32)
    q[:2] = base[:2]
    for rows in (1, 0):
        with ctx.option("MDB_FLAT_ROWS", rows):
            idx = FlatIndex(ctx, base, metric)
        exact = _exact(ctx, idx, q, 10)
        _check_oracle(oracle, metric, base, q, 10, exact)
        for qb in (1, 2, 4):
            with options(ctx, MDB_BF_X1=2, MDB_BF_BLOCK_QB=qb, MDB_MF_COOLDOWN=0):
                _same(idx.search(q, 10), exact, (rows, qb))


# ----------------------------------------------------------------------------------- IVF coarse search and f32 lists
@pytest.mark.parametrize("d", [64, 96, 128, 192, 256])
def test_coarse_mfma_four_tiles_per_wave(ctx, oracle, d):
    """ivf_coarse_mfma_kernel<NK = d / 16, J, TW>: four tiles per wave above 8 192 centroids (two below: tests/test_gpu_coarse_mfma.py),
    J = 1 / 2 / 4 / 8 pooled values per lane at up to 8 / 16 / 32 / 64 probes"""
    from tests.test_gpu_coarse_mfma import _check_probes, _index
    rng = np.random.default_rng(d)
    L_ = 8500
    cent = H.sift_like(L_, d, n_clusters=64, seed=d)
    cent[L_ - 10:] = cent[:10]
    o, g, v = _index(oracle, ctx, cent, seed=d)
    q = (cent[rng.integers(0, L_, 40)] + rng.normal(0, 6.0, (40, d))).astype(np.float32)
    _check_probes(ctx, o, g, q, probes=(8, 16, 32, 64))
    g.close()


def test_ivf_f32_scan_dot_block_sizes(ctx, oracle):
    """ivf_scan_f32_kernel<1, BLOCK>: dot-metric f32 lists at 64 / 128 / 256 threads per block (MDB_SCAN_F32_BLK; by default 128 up to
    batch 256 and 256 beyond)"""
    from muopdb_amd.index import BlockBasedIvf, NoQuantizer
    n, d, L_, P, k = 3000, 48, 12, 6, 10
    v = H.sift_like(n, d, n_clusters=6, seed=48)
    v[n - 30:] = v[:30]
    cent = H.kmeans(v, L_, iters=3, seed=2)
    index, vec, _ = H.build_ivf_files(v, [7 + 2 * i for i in range(n)], cent)
    g = BlockBasedIvf(ctx, index, vec, NoQuantizer(d, DOT))
    o = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_NONE, DOT))
    q = _batch(v, 300, 1, d)
    q[:4] = v[:4]
    for b in (300, 24):
        want = o.search(q[:b], k, num_probes=P)
        for blk in (0, 64, 128, 256):
            with ctx.option("MDB_SCAN_F32_BLK", blk):
                assert_result_rows(g.search(q[:b], k, P), want, b)
    g.close()

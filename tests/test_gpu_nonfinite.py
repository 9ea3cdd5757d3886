"""NaN, infinite and zero distances on every search and build path (-m gpu).

The C ABI promises that a NaN distance — where the reference panics in NotNan::new(..).unwrap() — comes back as MDB_ERR_NAN, and that
every other value orders as the reference orders it.  A kernel that forgets its flag does not crash: the key image f32_orderable puts
a positive NaN above +inf and a negative one below every distance, so the row comes back plausible and wrong.  A kernel that flags
where it BUILDS a table (upper-layer distance tables, PQ bound tables, the [B][L] centroid distances, the matrix-core filters)
reports an error the reference would never raise.  So every path gets three outcomes on one index:

  hit    a batch in which the oracle raises for at least one query gives status 5;
  miss   a batch in which it raises for none gives MDB_OK and the oracle's rows, counts and score bits (HNSW: counters too);
  clean  after the error the same handle serves the miss batch, and another index on the same context its own, as if nothing happened.

Non-finite values are planted into tame data (|x| <= 1e3): no partial sum overflows, so the class of a (query, row) pair — finite,
+inf, -inf, NaN — does not depend on the summation order, and a float64 numpy evaluation gives it independently of the oracle.  Graphs
and posting lists are built from the clean data and the vector file (or the PQ codebook) is overwritten afterwards: the topology is
known and the planted point's position is chosen.  The oracle is never handed NaN centroids or NaN queries through search(): its
centroid sort is undefined there.  hit and miss groups are chosen by running the oracle per query and hold at least 8 queries each.

The second half pins +-inf and signed zeros: rows, counts and score BITS against the oracle.  +0.0 and -0.0 cannot meet in one ranking
(every accumulator starts at +0.0: an L2 sum is never -0.0, and a dot score is -(+0.0 + ...) — -0.0 exactly when the sum is +0.0, and
the sum of products is never -0.0 unless every product is), so the test that would catch a kernel negating differently is the bit
comparison, not the order.

MDB_HNSW_L0_BLOCK and MDB_HNSW_BOUND_COMPACT are compile-time constants of the library, not options: the beam cases run the compiled
values.
"""
import contextlib
import ctypes as C
import threading

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

ERR_NAN = 5

# Every kernel or device function that raises MDB_FLAG_NAN (tests/test_nan_sites.py lists them from the source), the number of raises
# in it, and a test that reaches it with a planted NaN.  The tripwire checks functions and counts; which case reaches which raise of
# the functions with several is stated here, by the branch each raise sits in:
#   hnsw_beam_kernel      the closure of a layer of <= 64 points (no table path, ef >= 64): test_hnsw_nan_in_a_small_upper_layer_every_query_hits
#                         [MDB_HNSW_NO_TABLE=1] — the only case of this list that is not test_hnsw_nan_hit_miss_clean's;
#                         two neighbours per 16-lane group (16-lane rows, more new neighbours than groups) and one prefetched
#                         neighbour per group (16-lane rows): the d128 cases; the generic distance: the d32 cases and generic_dist;
#                         the block's final report (entry-point distances, and the flag handed over by the upper-layer launches): the
#                         `upper` plant behind the table path
#   upper_traverse_rank / upper_traverse_rank1 (one raise each, fed by three tests of the rank each): the closure of a small layer by
#                         test_hnsw_nan_in_a_small_upper_layer_every_query_hits[default | RANK=3 | NO_SPLIT,RANK=1] and the last block of
#                         test_hnsw_wide_upper_layer_rank_kernel_nan
#   hnsw_closure_kernel   the tail that ranks by counting (<= 512 keys): test_closure_kernel_..[120-128-*]; the bitonic tail: [1200-1280-*]
#   flat_refine_kernel    test_flat_batched_refine_forms_nan: a slice of at most one candidate per thread (MDB_REFINE_SLICES=3), a slice of
#                         more (500 copies, MDB_REFINE_SLICES=1), an overflowed candidate list scanned from the base (3 000 copies)
#   the raises removed one at a time on scratch builds and seen to fail their case: ivf_scan_f32_kernel, the beam's three distance forms,
#   its small-layer closure (caught by the [MDB_HNSW_NO_TABLE=1] cases only), the closure kernel's bitonic tail, ivf_pq_fused_kernel;
#   the others are covered by construction.
SITES = {
    "mdb_flat.hip::flat_scan_kernel": (1, "tests.test_gpu_parity::test_flat_nan_is_an_error"),
    "mdb_flat.hip::small_tile_key": (1, "tests.test_gpu_nonfinite::test_coarse_search_nan_centroid_is_an_error"),
    "mdb_flat_mfma.hip::flat_mfma_filter_kernel": (1, "tests.test_gpu_nonfinite::test_flat_batched_refine_forms_nan"),
    "mdb_flat_mfma.hip::flat_refine_kernel": (3, "tests.test_gpu_nonfinite::test_flat_batched_refine_forms_nan"),
    "mdb_flat_mfma.hip::flat_refine_group_kernel": (1, "tests.test_gpu_parity::test_flat_batched_path_nan_and_inf"),
    "mdb_hnsw.hip::hnsw_general_traverse": (1, "tests.test_gpu_nonfinite::test_hnsw_nan_hit_miss_clean"),
    "mdb_hnsw.hip::hnsw_closure_kernel": (2, "tests.test_gpu_nonfinite::test_closure_kernel_reachable_and_unreachable_nan"),
    "mdb_hnsw.hip::hnsw_beam_kernel": (5, "tests.test_gpu_nonfinite::test_hnsw_nan_hit_miss_clean"),
    "mdb_hnsw_build.hip::hnsw_select_kernel": (1, "tests.test_gpu_nonfinite::test_select_neighbors_nan_candidate"),
    "mdb_hnsw_rank.hip.h::upper_traverse_rank": (1, "tests.test_gpu_nonfinite::test_hnsw_wide_upper_layer_rank_kernel_nan"),
    "mdb_hnsw_rank.hip.h::upper_traverse_rank1": (1, "tests.test_gpu_nonfinite::test_hnsw_nan_hit_miss_clean"),
    "mdb_hnsw_upper.hip::upper_traverse_wave0": (1, "tests.test_gpu_nonfinite::test_hnsw_nan_hit_miss_clean"),
    "mdb_ivf_coarse.hip.h::ivf_coarse_rank_kernel": (1, "tests.test_gpu_coarse_mfma::test_coarse_mfma_nan_is_reported"),
    "mdb_ivf_fused.hip.h::ivf_prep_kernel": (1, "tests.test_gpu_nonfinite::test_coarse_search_nan_centroid_is_an_error"),
    "mdb_ivf_fused.hip.h::ivf_pq_fused_kernel": (1, "tests.test_gpu_nonfinite::test_pq_scan_nan_codebook_row"),
    "mdb_ivf_pq2.hip.h::ivf_scan_pq2_kernel": (1, "tests.test_gpu_nonfinite::test_pq_scan_nan_codebook_row"),
    "mdb_ivf_pq2.hip.h::ivf_pq3_refine_kernel": (1, "tests.test_gpu_nonfinite::test_pq_scan_nan_codebook_row"),
    "mdb_ivf_scan.hip.h::ivf_scan_f32_kernel": (1, "tests.test_gpu_nonfinite::test_ivf_f32_scan_nan_row"),
    "mdb_ivf_scan.hip.h::ivf_scan_pq_kernel": (1, "tests.test_gpu_nonfinite::test_pq_scan_nan_codebook_row"),
}


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


# ----------------------------------------------------------------------------------- helpers
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_rows_equal(res, ores, b, what=""):
    """counts, doc ids and score BITS (infinities and zeros with their signs included) of the first b rows"""
    for i in range(b):
        c = int(ores.counts[i])
        assert int(res.counts[i]) == c, (what, i, int(res.counts[i]), c)
        assert res.doc_ids(i) == ores.doc_ids(i), (what, i)
        assert np.array_equal(bits(res.scores[i, :c]), bits(ores.scores[i, :c])), (what, i)


def expect_nan(call):
    from muopdb_amd import lib as L
    with pytest.raises(L.MuopdbError) as e:
        call()
    assert e.value.status == ERR_NAN, e.value


def oracle_raises(search_one, q):
    """per query: does the oracle raise (the reference panics) on that query alone?"""
    out = np.zeros(len(q), bool)
    for i in range(len(q)):
        try:
            search_one(q[i:i + 1])
        except ValueError:
            out[i] = True
    return out


def groups(raises, what):
    """(hit, miss) query indices; both hold at least 8 queries, or the case would be vacuous"""
    hit, miss = np.flatnonzero(raises), np.flatnonzero(~raises)
    assert len(hit) >= 8 and len(miss) >= 8, "%s: %d queries hit, %d miss" % (what, len(hit), len(miss))
    return hit, miss


def pair_classes(q, rows, metric):
    """the class of every (query, row) distance in float64: 'f' finite, 'p' +inf, 'm' -inf, 'n' NaN (L2: sum (a-b)^2, dot: -sum ab)"""
    q, rows = np.asarray(q, np.float64), np.asarray(rows, np.float64)
    with np.errstate(all="ignore"):
        if metric == 0:
            d = ((q[:, None, :] - rows[None, :, :]) ** 2).sum(-1)
        else:
            d = -(q[:, None, :] * rows[None, :, :]).sum(-1)
    out = np.full(d.shape, "f")
    out[np.isposinf(d)] = "p"
    out[np.isneginf(d)] = "m"
    out[np.isnan(d)] = "n"
    return out


def near_queries(v, b, seed, sigma):
    rng = np.random.default_rng(seed)
    return (v[rng.integers(0, len(v), b)] + rng.normal(0, sigma, (b, v.shape[1]))).astype(np.float32)


def best_split_list(probes, pls, target=24):
    """the posting list whose number of probing queries is nearest `target` (so that hit and miss groups are both large)"""
    counts = np.bincount(probes.reshape(-1), minlength=len(pls)).astype(np.int64)
    counts[[i for i, p in enumerate(pls) if len(p) < 8]] = 10 ** 6
    return int(np.argmin(np.abs(counts - target)))


def split_lists(probes, pls, target):
    """posting lists (in id order, non-empty) that together are probed by at most `target` of the queries"""
    chosen, hit = [], np.zeros(len(probes), bool)
    for c in range(len(pls)):
        mine = (probes == c).any(1)
        if len(pls[c]) and mine.any() and int((hit | mine).sum()) <= target:
            chosen.append(c)
            hit |= mine
    return chosen


# =================================================================================== 1. NaN: IVF f32 scan
N_IVF, D, L_IVF, P_IVF, K = 2048, 32, 16, 4, 10


@pytest.fixture(scope="module")
def ivf32(ctx, oracle):
    """2 048 x 32 in 16 lists; the `bad` copy has a NaN coordinate in one row of list c, chosen so that about a third of the 64
    queries probe c"""
    from muopdb_amd.index import BlockBasedIvf
    v = H.sift_like(N_IVF, D, n_clusters=20, seed=3)
    cent = H.kmeans(v, L_IVF, iters=3, seed=4)
    docs = [100 + 3 * i for i in range(N_IVF)]
    index, vec, pls = H.build_ivf_files(v, docs, cent)
    q = near_queries(v, 64, 5, 3.0)
    o = oracle.BlockBasedIvf(index, vec)
    probes = o.find_nearest_centroids(q, P_IVF)
    c = best_split_list(probes, pls)
    pid = int(pls[c][len(pls[c]) // 2])
    bad = v.copy()
    bad[pid, 5] = np.nan
    vec_bad = F.write_vector_file(bad)
    w = dict(v=v, bad=bad, docs=docs, index=index, vec=vec, vec_bad=vec_bad, pls=pls, q=q, probes=probes, c=c, pid=pid, cent=cent,
             o=o, o_bad=oracle.BlockBasedIvf(index, vec_bad), g=BlockBasedIvf(ctx, index, vec), g_bad=BlockBasedIvf(ctx, index, vec_bad))
    raises = oracle_raises(lambda x: w["o_bad"].search(x, K, num_probes=P_IVF), q)
    # the oracle raises exactly for the queries that probe list c, and float64 agrees: the planted row is NaN against every query
    assert np.array_equal(raises, (probes == c).any(1))
    assert np.all(pair_classes(q, bad[pid:pid + 1], 0) == "n") and np.all(pair_classes(q, np.delete(bad, pid, 0)[::7], 0) == "f")
    w["hit"], w["miss"] = groups(raises, "ivf f32")
    yield w
    w["g"].close()
    w["g_bad"].close()


@pytest.mark.parametrize("nsplit,blk", [(0, 0), (1, 0), (3, 0), (16, 0), (5, 64), (4, 128)])
def test_ivf_f32_scan_nan_row(ctx, oracle, ivf32, nsplit, blk):
    """ivf_scan_f32_kernel at one and several blocks per query and every block size: a NaN row in list c is an error for the queries
    that probe c, and for them only"""
    w = ivf32
    q, hit, miss = w["q"], w["hit"], w["miss"]
    with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit, MDB_SCAN_F32_BLK=blk):
        expect_nan(lambda: w["g_bad"].search(q[hit], K, P_IVF))
        expect_nan(lambda: w["g_bad"].search(q, K, P_IVF))                  # one batch with both kinds
        for i in hit[:8]:                                                   # one query per call
            expect_nan(lambda: w["g_bad"].search(q[i:i + 1], K, P_IVF))
        assert_rows_equal(w["g_bad"].search(q[miss], K, P_IVF), w["o_bad"].search(q[miss], K, num_probes=P_IVF), len(miss), "miss")
        expect_nan(lambda: w["g_bad"].search(q[hit], K, P_IVF))
        assert_rows_equal(w["g_bad"].search(q[miss], K, P_IVF), w["o_bad"].search(q[miss], K, num_probes=P_IVF), len(miss), "clean")
        assert_rows_equal(w["g"].search(q, K, P_IVF), w["o"].search(q, K, num_probes=P_IVF), len(q), "other index")
        # explicit probe lists: the same list reached without the coarse search
        pr = w["probes"]
        expect_nan(lambda: w["g_bad"].search_with_centroids_and_remap(q[hit], pr[hit], K))
        assert_rows_equal(w["g_bad"].search_with_centroids_and_remap(q[miss], pr[miss], K), w["o_bad"].search(q[miss], K, probes=pr[miss]),
                          len(miss), "probes")


def test_ivf_f32_scan_nan_row_tombstoned_or_filtered(ctx, oracle, ivf32):
    """A tombstoned point is skipped before its distance on both sides: after invalidate(doc of the NaN row) every query is served.
    DEVIATION (HISTORY.md section 9): under a planner bitmap that excludes the NaN row the reference still evaluates it
    (scan_posting_list filters AFTER the distances, index.rs:214-226) and panics; the library skips filtered points before the
    distance, as its header states, and returns the rows the reference returns on the clean copy under the same bitmap."""
    from muopdb_amd.index import BlockBasedIvf, allow_bitmap
    w = ivf32
    q, hit = w["q"], w["hit"]
    bm = allow_bitmap(np.delete(np.arange(N_IVF), w["pid"]), N_IVF)
    with oracle.planner_filter(bm):
        assert oracle_raises(lambda x: w["o_bad"].search(x, K, num_probes=P_IVF), q[hit]).all()    # the reference's behaviour
        want = w["o"].search(q, K, num_probes=P_IVF)
    assert_rows_equal(w["g_bad"].search(q, K, P_IVF, planner=bm), want, len(q), "filtered")
    per_query = np.repeat(bm[None, :], len(q), 0)
    assert_rows_equal(w["g_bad"].search(q, K, P_IVF, planner=per_query), want, len(q), "filtered per query")
    expect_nan(lambda: w["g_bad"].search(q, K, P_IVF))             # no filter: the row counts again
    g2, o2 = BlockBasedIvf(ctx, w["index"], w["vec_bad"]), oracle.BlockBasedIvf(w["index"], w["vec_bad"])
    expect_nan(lambda: g2.search(q, K, P_IVF))
    doc = w["docs"][w["pid"]]
    assert g2.invalidate(doc) and o2.invalidate(doc)
    assert_rows_equal(g2.search(q, K, P_IVF), o2.search(q, K, num_probes=P_IVF), len(q), "tombstoned")
    g2.close()


# =================================================================================== 1. NaN: PQ scans
S_STAR = 1     # the subspace of the NaN codebook row


def _pq_world(ctx, oracle, n, d, sub, nlists, probes_n, seed, cent=None, nq=64, sigma=3.0):
    """An L2 PQ index with 8-bit codes whose codebook row (S_STAR, c*) holds a NaN.  Stored codes are written directly: `unused` holds
    c* in no vector at all, `planted` in up to 5 vectors of each of a few lists (chosen so that about a third of the queries probe one)."""
    from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
    v = H.sift_like(n, d, n_clusters=20, seed=seed)
    if cent is None:
        cent = H.kmeans(v, nlists, iters=3, seed=seed + 1)
    else:
        rng = np.random.default_rng(seed)
        v = (cent[rng.integers(0, len(cent), n)] + rng.normal(0, 3.0, (n, d))).astype(np.float32)
    cb = H.train_pq_codebook(v[:1500], sub, 8, iters=2, seed=seed).reshape(d // sub, 256, sub)
    docs = [10 + 7 * i for i in range(n)]
    codes = oracle.ProductQuantizer(d, sub, 8, cb).quantize(v)
    col = codes[:, S_STAR]
    c_star = int(np.bincount(col, minlength=256)[1:].argmax()) + 1           # a code in use, not code 0
    others = np.delete(np.arange(256), c_star)
    c_alt = int(others[((cb[S_STAR, others] - cb[S_STAR, c_star]) ** 2).sum(1).argmin()])
    unused = codes.copy()
    unused[col == c_star, S_STAR] = c_alt
    cb_nan = cb.copy()
    cb_nan[S_STAR, c_star, sub // 2] = np.nan
    opq = oracle.ProductQuantizer(d, sub, 8, cb_nan)
    q = near_queries(v, nq, seed + 2, sigma)
    assert not (opq.quantize(q)[:, S_STAR] == c_star).any(), "a query quantizes to the NaN row itself"
    index, _, pls = H.build_ivf_files(v, docs, cent, quantize=lambda x: unused)
    o_probe = oracle.BlockBasedIvf(index, F.write_vector_file(unused), oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, sub, 8, cb))
    probes = o_probe.find_nearest_centroids(q, probes_n)
    chosen = split_lists(probes, pls, target=len(q) // 3)
    planted = unused.copy()
    for c in chosen:
        planted[pls[c][:: max(1, len(pls[c]) // 5)][:5].astype(np.int64), S_STAR] = c_star
    oq = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, sub, 8, cb_nan)
    gq = ProductQuantizer(d, sub, 8, cb_nan)
    w = dict(q=q, probes=probes, chosen=chosen, P=probes_n, index=index, gq=gq, oq=oq, cent=cent, pls=pls, docs=docs, d=d)
    for name, cd in (("unused", unused), ("planted", planted)):
        vec = F.write_vector_file(cd)
        w["vec_" + name] = vec
        w["o_" + name] = oracle.BlockBasedIvf(index, vec, oq)
        w["g_" + name] = BlockBasedIvf(ctx, index, vec, gq)
    raises = oracle_raises(lambda x: w["o_planted"].search(x, K, num_probes=probes_n), q)
    assert np.array_equal(raises, np.isin(probes, chosen).any(1))
    assert not oracle_raises(lambda x: w["o_unused"].search(x, K, num_probes=probes_n), q).any()
    w["hit"], w["miss"] = groups(raises, "pq")
    return w


@pytest.fixture(scope="module")
def pq(ctx, oracle):
    w = _pq_world(ctx, oracle, N_IVF, D, 8, L_IVF, P_IVF, seed=21)
    yield w
    w["g_unused"].close()
    w["g_planted"].close()


PQ_FORMS = {
    "one_phase_filter": dict(MDB_PQ_NO_FUSED=1),                                    # ivf_scan_pq2_kernel<.., FILT = true>
    "one_phase_no_filter": dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FILTER=1),             # ivf_scan_pq2_kernel<.., FILT = false>
    "one_phase_one_block": dict(MDB_PQ_NO_FUSED=1, MDB_PQ_BLOCKS=1),
    "generic": dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FAST=1),                           # ivf_scan_pq_kernel
    "two_phase": dict(MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1),                   # ivf_scan_pq3_kernel + ivf_pq3_refine_kernel
    "two_phase_overflow": dict(MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1, MDB_PQ3_CAP=8),   # ... and the gated one-phase re-run
    "fused": dict(),                                                                # ivf_prep_kernel + ivf_pq_fused_kernel<.., 1>
    "fused_quant_in_prep": dict(MDB_PQF_QUANT_IN_PREP=1),
    "fused_overflow": dict(MDB_PQF_CAP=8),
    "fused_no_sdc": dict(MDB_PQ_SDC_MAX_MB=0),                                      # the code-to-code table built inside the block
    "fused_masks": dict(MDB_SCAN_MASKS_ALWAYS=1),
}


def _pq_hit_miss_clean(ctx, w, opts, explicit_probes=False):
    q, hit, miss, P = w["q"], w["hit"], w["miss"], w["P"]

    def g_search(g, sel):
        if explicit_probes:
            return g.search_with_centroids_and_remap(q[sel], w["probes"][sel], K)
        return g.search(q[sel], K, P)

    def o_search(o, sel):
        if explicit_probes:
            return o.search(q[sel], K, probes=w["probes"][sel])
        return o.search(q[sel], K, num_probes=P)
    everyone = np.arange(len(q))
    with options(ctx, **opts):
        # miss (b), the table-build trap: the NaN row is in every bound / code-to-code table, and in no stored vector
        assert_rows_equal(g_search(w["g_unused"], everyone), o_search(w["o_unused"], everyone), len(q), "no vector holds c*")
        # hit: a vector of a probed list holds c*; twice, so that the fused step's alternating counter sets both see an error
        expect_nan(lambda: g_search(w["g_planted"], hit))
        expect_nan(lambda: g_search(w["g_planted"], everyone))
        # miss (a) and clean: only un-probed lists hold c*
        assert_rows_equal(g_search(w["g_planted"], miss), o_search(w["o_planted"], miss), len(miss), "miss")
        for i in hit[:8]:           # one query per call: no other query's flag can stand in for this one's
            expect_nan(lambda: g_search(w["g_planted"], np.array([i])))
        assert_rows_equal(g_search(w["g_planted"], miss), o_search(w["o_planted"], miss), len(miss), "clean")
        assert_rows_equal(g_search(w["g_unused"], everyone), o_search(w["o_unused"], everyone), len(q), "other index")


@pytest.mark.parametrize("form", sorted(PQ_FORMS))
def test_pq_scan_nan_codebook_row(ctx, oracle, pq, form):
    """The one-phase scan with and without its bound filter, the generic kernel, the two-phase scan and the fused step: a NaN codebook
    row (s, c*) is an error exactly when a stored vector of a PROBED list holds c* — never because a table was built over it"""
    _pq_hit_miss_clean(ctx, pq, PQ_FORMS[form])


def test_pq_scan_nan_codebook_row_explicit_probes(ctx, oracle, pq):
    """the fused step and the unfused one with the probe lists handed in (no coarse search in the step: ivf_pq_fused_kernel<.., 0>)"""
    _pq_hit_miss_clean(ctx, pq, dict(), explicit_probes=True)
    _pq_hit_miss_clean(ctx, pq, dict(MDB_PQ_NO_FUSED=1), explicit_probes=True)


def test_pq_scan_odd_subvector_width_nan_codebook_row(ctx, oracle):
    """subvectors of 6 floats: no compiled fast path, the generic kernel (ivf_scan_pq_kernel) by dispatch, not by option"""
    w = _pq_world(ctx, oracle, 1536, 30, 6, 12, 3, seed=33)
    _pq_hit_miss_clean(ctx, w, dict())
    w["g_unused"].close()
    w["g_planted"].close()


@pytest.fixture(scope="module")
def pq_cm(ctx, oracle):
    """1 024 centroids of d = 64 (the matrix-core coarse search's smallest shape), 8 subspaces of 8-bit codes, 48 queries"""
    cent = H.sift_like(1024, 64, n_clusters=32, seed=11)
    w = _pq_world(ctx, oracle, 4000, 64, 8, 1024, 16, seed=44, cent=cent, nq=48, sigma=4.0)
    yield w
    w["g_unused"].close()
    w["g_planted"].close()


@pytest.mark.parametrize("opts", [dict(), dict(MDB_CM_SPLIT=1), dict(MDB_CM_GLOBAL_BOUND=0), dict(MDB_PQF_NO_QUANT_IN_COARSE=1),
                                  dict(MDB_IVF_COARSE_MFMA=0)], ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "default")
def test_fused_step_behind_matrix_core_coarse_nan(ctx, oracle, pq_cm, opts):
    """ivf_pq_fused_kernel<.., 2> (candidates of the matrix-core coarse filter ranked inside the step), the coarse search as launches
    of its own (MDB_CM_SPLIT: ivf_coarse_rank_kernel) and every distance exactly (MDB_IVF_COARSE_MFMA=0): the NaN codebook row as in
    test_pq_scan_nan_codebook_row; then a NaN CENTROID with finite queries, which the library reports whichever list it is"""
    from muopdb_amd.index import BlockBasedIvf
    w = pq_cm
    _pq_hit_miss_clean(ctx, w, opts)
    bad_cent = w["cent"].copy()
    bad_cent[500, 1] = np.nan
    gi = BlockBasedIvf(ctx, F.write_ivf_index(bad_cent, w["docs"], w["pls"], quantized_dimension=8), w["vec_unused"], w["gq"])
    with options(ctx, **opts):
        expect_nan(lambda: gi.search(w["q"], K, 16))
        expect_nan(lambda: gi.find_nearest_centroids(w["q"], 16))
        assert_rows_equal(w["g_unused"].search(w["q"], K, 16), w["o_unused"].search(w["q"], K, num_probes=16), len(w["q"]), "clean")
    gi.close()


# =================================================================================== 1. NaN: coarse search
def test_coarse_search_nan_centroid_is_an_error(ctx, oracle, ivf32, pq):
    """DEVIATION (HISTORY.md section 9): the reference's find_nearest_centroids orders with total_cmp
    (ivf/block_based/index.rs:158-161) and never panics on a NaN centroid distance; the library's stated rule is stricter — a NaN
    distance anywhere in the coarse search is MDB_ERR_NAN.  No oracle call (its `<` sort is no strict weak order with a NaN).
    Finite queries, one NaN centroid, through every exact form the small shapes reach: the one-wave-per-tile kernels of batches <= 4
    (small_tile_key), flat_scan_kernel beyond, and the fused step's own [B][L] pass (ivf_prep_kernel)."""
    from muopdb_amd.index import BlockBasedIvf
    w = ivf32
    q = w["q"]
    bad_cent = w["cent"].copy()
    bad_cent[3, 7] = np.nan
    gi = BlockBasedIvf(ctx, F.write_ivf_index(bad_cent, w["docs"], w["pls"]), w["vec"])
    for b in (1, 2, 4):                                                  # flat_small_scan_kernel
        expect_nan(lambda: gi.find_nearest_centroids(q[:b], P_IVF))
    with ctx.option("MDB_FLAT_NO_SMALL", 4):                             # flat_small_block_kernel
        expect_nan(lambda: gi.find_nearest_centroids(q[:2], P_IVF))
    for b in (5, 24, 64):                                                # flat_scan_kernel
        expect_nan(lambda: gi.find_nearest_centroids(q[:b], P_IVF))
    expect_nan(lambda: gi.search(q[:24], K, P_IVF))
    # ... and the probes of a clean index are still the oracle's
    assert np.array_equal(w["g"].find_nearest_centroids(q, P_IVF), w["o"].find_nearest_centroids(q, P_IVF))
    gi.close()
    p = pq
    bad_cent = p["cent"].copy()
    bad_cent[9, 0] = np.nan
    gp = BlockBasedIvf(ctx, F.write_ivf_index(bad_cent, p["docs"], p["pls"], quantized_dimension=4), p["vec_unused"], p["gq"])
    for b in (1, 24, 64):                                                # ivf_prep_kernel: every (query, centroid) distance
        expect_nan(lambda: gp.search(p["q"][:b], K, p["P"]))
    with ctx.option("MDB_PQF_QUANT_IN_PREP", 1):
        expect_nan(lambda: gp.search(p["q"][:24], K, p["P"]))
    assert_rows_equal(p["g_unused"].search(p["q"], K, p["P"]), p["o_unused"].search(p["q"], K, num_probes=p["P"]), len(p["q"]), "clean")
    gp.close()


def test_flat_batched_refine_forms_nan(ctx):
    """70 000 x 16 (the batched path's smallest base): a NaN row is an error whichever refine form meets it — by query groups
    (flat_refine_group_kernel), by slices of a few candidates, one slice of several hundred candidates (500 stored copies of the
    queries' neighbour: more candidates than the slice has threads), a candidate list that overflows (3 000 copies: the slices scan
    the whole base exactly) — and behind the f32 matrix-core filter (MDB_MF_F32 at load: flat_mfma_filter_kernel).  The next search
    of a clean index on the same context is served."""
    from muopdb_amd.index import FlatIndex
    rng = np.random.default_rng(9)
    base = rng.standard_normal((70000, 16)).astype(np.float32)
    q = rng.standard_normal((40, 16)).astype(np.float32)
    g = FlatIndex(ctx, base)
    with ctx.option("MDB_FLAT_NO_MFMA", 1):
        want = g.search(q, 10)

    def clean_ok(opts):
        got = g.search(q, 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2]), opts
    bad = base.copy()
    bad[65000, 7] = np.nan
    gb = FlatIndex(ctx, bad)
    with ctx.option("MDB_MF_F32", 1):
        gb32 = FlatIndex(ctx, bad)
    for opts in (dict(), dict(MDB_REFINE_GROUP_BIG=1), dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=3), dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=1),
                 dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_WAVE_MIN_B=0)):
        with options(ctx, MDB_MF_COOLDOWN=0, **opts):
            expect_nan(lambda: gb.search(q, 10))
            expect_nan(lambda: gb.search(q[:9], 10))
            expect_nan(lambda: gb32.search(q, 10))
            clean_ok(opts)
    gb.close()
    gb32.close()
    for copies in (500, 3000):
        ties = bad.copy()
        ties[:copies] = q[0] + np.float32(0.25)
        qt = (q[0] + rng.normal(0, 0.01, (40, 16))).astype(np.float32)
        gt = FlatIndex(ctx, ties)
        for opts in (dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=1), dict(MDB_REFINE_NO_GROUPS=1, MDB_REFINE_SLICES=3), dict()):
            with options(ctx, MDB_MF_COOLDOWN=0, **opts):
                expect_nan(lambda: gt.search(qt, 10))
                clean_ok(opts)
        gt.close()
    g.close()


# =================================================================================== 1. NaN: HNSW
def _graph(oracle, v, M, max_layers, efc, metric=0, seed=1):
    """(index bytes, layers) of the oracle's builder; the builder's entry point first in the top layer (the reader's rule)"""
    b = oracle.HnswBuilder(v.shape[1], M, max_layers, efc, metric, seed)
    b.insert(v)
    layers, eps = b.layers(), b.entry_points()
    if len(layers) > 1:
        top = layers[-1]
        layers[-1] = {eps[0]: top[eps[0]], **{p: e for p, e in top.items() if p != eps[0]}}
    return F.write_hnsw_index(layers, list(range(len(v))), v.shape[1]), layers


# (name, ef, options, plants): "upper" = the NaN sits in a point of layer 1, "l0" = in a point of layer 0 only.  ef beyond the upper
# layers' sizes evaluates every upper-layer point for every query: no miss group exists there, only the layer-0 plant is run.
HNSW_FORMS = [
    ("beam", 16, dict(), ("upper", "l0")),                                   # split path: top rank kernel, hnsw_upper_kernel, layer-0 beam
    ("beam_ef100", 100, dict(), ("upper", "l0")),
    ("rank0", 16, dict(MDB_HNSW_RANK=0), ("upper", "l0")),                   # hnsw_upper_top_kernel
    ("rank1", 16, dict(MDB_HNSW_RANK=1), ("upper", "l0")),                   # hnsw_upper_rank_kernel behind the top kernel
    ("rank3", 16, dict(MDB_HNSW_RANK=3), ("upper", "l0")),
    ("no_split", 16, dict(MDB_HNSW_NO_SPLIT=1), ("upper", "l0")),            # table kernels + one upper launch
    ("no_split_rank1", 16, dict(MDB_HNSW_NO_SPLIT=1, MDB_HNSW_RANK=1), ("upper", "l0")),
    ("table64_never", 16, dict(MDB_HNSW_TABLE64_MIN_B=1 << 30), ("upper", "l0")),   # hnsw_upper_table_kernel / table16
    ("table_no_lds", 16, dict(MDB_HNSW_TABLE_NO_LDS=1, MDB_HNSW_NO_SPLIT=1), ("upper", "l0")),
    ("five_registers", 16, dict(MDB_HNSW_NB4_SLACK=0), ("upper", "l0")),
    ("no_table", 16, dict(MDB_HNSW_NO_TABLE=1), ("upper", "l0")),            # the all-in-one beam kernel over every layer
    ("no_table_ef64", 64, dict(MDB_HNSW_NO_TABLE=1), ("upper", "l0")),       # ... with the small top layer as a closure
    ("no_row64", 16, dict(MDB_HNSW_NO_ROW64=1), ("upper", "l0")),
    ("generic_dist", 16, dict(MDB_HNSW_GENERIC_DIST=1), ("upper", "l0")),
    ("general", 16, dict(MDB_HNSW_NO_BEAM=1), ("upper", "l0")),              # hnsw_search_kernel
    ("wide_ef300", 300, dict(), ("l0",)),                                    # the 8-register beam
    ("general_ef300", 300, dict(MDB_HNSW_NO_WIDE=1), ("l0",)),
    ("general_ef600", 600, dict(), ("l0",)),                                 # ef above the beam limit
]
HNSW_EFS = sorted({f[1] for f in HNSW_FORMS})
MIN_MISS = 32      # MDB_HNSW_TABLE64_MIN_B: the smallest batch of the split path


@pytest.fixture(scope="module", params=[32, 128], ids=lambda d: "d%d" % d)
def hnsw_world(request, ctx, oracle):
    """The 2 000-point, M = 8, 3-layer graph of test_gpu_scratch.py (d = 32: the generic distance of the beam kernel; d = 128: its
    16-lane forms), built from the clean rows; `upper` has a NaN in a layer-1 point, `l0` in a point of layer 0 only.  64 near-data
    queries; for the layer-0 plant 16 of them sit next to the planted point.  hit / miss groups per ef come from the oracle."""
    from muopdb_amd.index import BlockBasedHnsw
    d = request.param
    n = 2000
    v = H.sift_like(n, d, n_clusters=20, seed=3)
    hidx, layers = _graph(oracle, v, 8, 3, 40)
    assert len(layers) >= 3
    q = near_queries(v, 64, 7, 3.0)
    w = dict(d=d, v=v, hidx=hidx, groups={})
    w["g"], w["o"] = BlockBasedHnsw(ctx, hidx, F.write_vector_file(v), d), oracle.BlockBasedHnsw(hidx, F.write_vector_file(v), d)
    upper_pts = [p for p in layers[1] if p not in layers[2]]
    l0_pts = [p for p in range(n) if p not in layers[1]]

    def plant(p):
        bad = v.copy()
        bad[p, d // 2] = np.nan
        return F.write_vector_file(bad)

    def raises_for(vf, qq, ef):
        o = oracle.BlockBasedHnsw(hidx, vf, d)
        return oracle_raises(lambda x: o.ann_search(x, K, ef), qq)
    # upper: per ef the first layer-1 point that at least 8 queries meet and at least 32 do not (MIN_MISS: the split path, the top
    # kernels and hnsw_upper_table64_kernel serve batches of >= 32 only, and the miss batch is the sharp case there)
    for ef in (16, 64, 100):
        for p in upper_pts:
            vf = plant(p)
            r = raises_for(vf, q, ef)
            if 8 <= int(r.sum()) <= 64 - MIN_MISS:
                w["upper", ef] = dict(p=p, vf=vf, q=q, raises={ef: r})
                break
        assert ("upper", ef) in w, "no layer-1 point splits the queries at ef %d" % ef
    # small: a point of layer 2 (at most 64 points: with ef >= 64 the all-in-one beam kernel takes that layer as a closure)
    assert 2 < len(layers[2]) <= 64
    p = [x for x in layers[2] if x not in layers[3]][1] if len(layers) > 3 else list(layers[2])[1]
    w["small"] = dict(p=p, vf=plant(p), q=q)
    # l0: a layer-0-only point with 16 queries next to it; the other 48 mostly never meet it, at any ef
    rng = np.random.default_rng(11)
    for p in l0_pts[100::37]:
        qq = q.copy()
        qq[:16] = v[p] + rng.normal(0, 0.5, (16, d)).astype(np.float32)
        vf = plant(p)
        r = {ef: raises_for(vf, qq, ef) for ef in HNSW_EFS}
        if all(8 <= int(x.sum()) <= 64 - (MIN_MISS if ef <= 448 else 8) for ef, x in r.items()):
            w["l0"] = dict(p=p, vf=vf, q=qq, raises=r)
            break
    assert "l0" in w, "no layer-0 point splits the queries at every ef"
    plants = [k for k in w if k in ("l0", "small") or isinstance(k, tuple)]
    for kind in plants:
        w[kind]["g"] = BlockBasedHnsw(ctx, hidx, w[kind]["vf"], d)
        w[kind]["o"] = oracle.BlockBasedHnsw(hidx, w[kind]["vf"], d)
        assert np.all(pair_classes(w[kind]["q"], v[w[kind]["p"]:w[kind]["p"] + 1] * np.nan, 0) == "n")
    w["upper"] = w["upper", 16]
    yield w
    for g in [w["g"]] + [w[kind]["g"] for kind in plants]:
        g.close()


def _hnsw_counters(ctx, o, g, q, k, ef, what):
    """rows AND both traversal counters of one batch against the oracle's"""
    o.stats()
    want = o.ann_search(q, k, ef)
    evals, expanded = o.stats()
    ctx.stats()
    got = g.ann_search(q, k, ef)
    st = ctx.stats()
    assert_rows_equal(got, want, len(q), what)
    assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), what


@pytest.mark.parametrize("form,ef,opts,plants", HNSW_FORMS, ids=[f[0] for f in HNSW_FORMS])
def test_hnsw_nan_hit_miss_clean(ctx, oracle, hnsw_world, form, ef, opts, plants):
    """Every traversal form: a NaN point is an error for the queries whose traversal evaluates it and for no other.  For the
    upper-layer plant the miss batch is the sharp case: the point's NaN sits in every query's distance table."""
    w = hnsw_world
    for kind in plants:
        pw = w["upper", ef] if kind == "upper" else w[kind]
        q = pw["q"]
        hit, miss = groups(pw["raises"][ef], "hnsw %s ef %d" % (kind, ef))
        if ef <= 448 and "MDB_HNSW_NO_BEAM" not in opts and "MDB_HNSW_NO_WIDE" not in opts:   # every form that may take the table path
            assert len(miss) >= MIN_MISS, (form, kind, len(miss))
        with options(ctx, **opts):
            expect_nan(lambda: pw["g"].ann_search(q[hit], K, ef))
            expect_nan(lambda: pw["g"].ann_search(q, K, ef))
            _hnsw_counters(ctx, pw["o"], pw["g"], q[miss], K, ef, (form, kind, "miss"))
            for i in hit[:8]:           # one query per call: no other query's flag can stand in for this one's
                expect_nan(lambda: pw["g"].ann_search(q[i:i + 1], K, ef))
            _hnsw_counters(ctx, pw["o"], pw["g"], q[miss], K, ef, (form, kind, "clean"))
            _hnsw_counters(ctx, w["o"], w["g"], q, K, ef, (form, kind, "other index"))


@pytest.mark.parametrize("ef,opts", [(64, dict(MDB_HNSW_NO_TABLE=1)), (100, dict(MDB_HNSW_NO_TABLE=1)), (64, dict(MDB_HNSW_NO_TABLE=1, MDB_HNSW_NO_ROW64=1)),
                                     (64, dict()), (100, dict()), (64, dict(MDB_HNSW_RANK=0)), (64, dict(MDB_HNSW_RANK=3)), (64, dict(MDB_HNSW_NO_SPLIT=1)),
                                     (64, dict(MDB_HNSW_NO_SPLIT=1, MDB_HNSW_RANK=1)), (64, dict(MDB_HNSW_NO_BEAM=1))],
                         ids=lambda x: (",".join("%s=%d" % kv for kv in x.items()) or "default") if isinstance(x, dict) else "ef%d" % x)
def test_hnsw_nan_in_a_small_upper_layer_every_query_hits(ctx, oracle, hnsw_world, ef, opts):
    """A NaN in a point of layer 2 (38 points) at ef >= 64: every query's traversal evaluates the whole layer, so every query errors —
    hit only.  With MDB_HNSW_NO_TABLE the all-in-one beam kernel takes a layer of at most 64 points as a closure of its entry point,
    and that branch has a raise of its own; one query per call, so that nothing but that raise can report it.  On the table path the
    upper-layer kernels take such a layer as a closure too; the ones on sorted positions keep the LOWEST rank met, and a NaN ranks
    last.  Then the clean copy."""
    w = hnsw_world
    pw, q, d = w["small"], w["small"]["q"], w["d"]
    assert oracle_raises(lambda x: pw["o"].ann_search(x, K, ef), q).all()
    with options(ctx, **opts):
        expect_nan(lambda: pw["g"].ann_search(q, K, ef))
        for i in range(8):
            expect_nan(lambda: pw["g"].ann_search(q[i:i + 1], K, ef))
        _hnsw_counters(ctx, w["o"], w["g"], q, K, ef, "clean copy")
    # The sign of the NaN a distance comes out with decides where its key image sorts: a negative NaN below every distance — the
    # closure's nearest point, so the next layer's entry-point check meets it again — a positive one above +inf, where only the
    # closure's own check sees it.  Both signs of the stored NaN under both metrics (the subtraction of L2 and the negation of dot
    # flip it): whichever the arithmetic produces, one of the four ranks last.
    for sign_bits in (0x7FC00000, 0xFFC00000):
        bad = w["v"].copy()
        bad[pw["p"], d // 2] = np.array([sign_bits], np.uint32).view(np.float32)[0]
        vf = F.write_vector_file(bad)
        for metric in (0, 1):
            g, o = _hnsw_pair(ctx, oracle, w["hidx"], vf, metric, d)
            assert oracle_raises(lambda x: o.ann_search(x, K, ef), q[:8]).all()
            with options(ctx, **opts):
                expect_nan(lambda: g.ann_search(q, K, ef))
                for i in range(8):
                    expect_nan(lambda: g.ann_search(q[i:i + 1], K, ef))
            g.close()


def _ring_layer(rng, pts):
    m = len(pts)
    nb = np.stack([np.roll(pts, -1), np.roll(pts, 1)] + [pts[rng.integers(0, m, m)] for _ in range(4)], 1)
    return {int(p): [int(x) for x in row] for p, row in zip(pts, nb)}


def test_hnsw_wide_upper_layer_rank_kernel_nan(ctx, oracle):
    """More than 2 048 points in layer 1 (2 060 of 4 400, a hand-written ring graph; the table path wants four points per upper-layer
    point): MDB_HNSW_RANK=3 runs the layer-1 traversal on sorted positions with four waves per block (hnsw_upper_rank_kernel<4>:
    upper_traverse_rank).  A NaN in a layer-1 point: hit and miss by the oracle."""
    from muopdb_amd.index import BlockBasedHnsw
    n, d, ef = 4400, 32, 16
    rng = np.random.default_rng(5)
    v = H.sift_like(n, d, n_clusters=20, seed=8)
    ar = np.arange(n)
    nb = np.stack([(ar + 1) % n, (ar - 1) % n] + [rng.integers(0, n, n) for _ in range(4)], 1)
    layers = [(None, np.arange(n + 1, dtype=np.uint64) * 6, nb.reshape(-1).astype(np.uint32)),
              _ring_layer(rng, np.arange(2060)), _ring_layer(rng, np.arange(40))]
    hidx = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d)
    q = near_queries(v, 64, 9, 3.0)
    found = None
    for p in range(41, 2060, 53):
        bad = v.copy()
        bad[p, 3] = np.nan
        vf = F.write_vector_file(bad)
        o = oracle.BlockBasedHnsw(hidx, vf, d)
        r = oracle_raises(lambda x: o.ann_search(x, K, ef), q)
        if 8 <= int(r.sum()) <= 56:
            found = (vf, o, r)
            break
    assert found, "no layer-1 point splits the queries"
    vf, o, r = found
    hit, miss = groups(r, "wide upper layer")
    g = BlockBasedHnsw(ctx, hidx, vf, d)
    for opts in (dict(MDB_HNSW_RANK=3), dict(MDB_HNSW_RANK=1), dict()):
        with options(ctx, **opts):
            expect_nan(lambda: g.ann_search(q[hit], K, ef))
            _hnsw_counters(ctx, o, g, q[miss], K, ef, (opts, "miss"))
            for i in hit[:8]:
                expect_nan(lambda: g.ann_search(q[i:i + 1], K, ef))
            _hnsw_counters(ctx, o, g, q[miss], K, ef, (opts, "clean"))
    # a NaN in a point of the 40-point top layer at ef 64: every query's closure of that layer evaluates it, whichever rank it gets (a
    # NaN ranks last, the closure keeps the LOWEST rank) — in one upper launch over every layer (MDB_HNSW_NO_SPLIT: upper_traverse_rank's
    # own closure), behind the top launch, and by default
    bad = v.copy()
    bad[17, 3] = np.nan
    vf2 = F.write_vector_file(bad)
    o2 = oracle.BlockBasedHnsw(hidx, vf2, d)
    assert oracle_raises(lambda x: o2.ann_search(x, K, 64), q).all()
    g2 = BlockBasedHnsw(ctx, hidx, vf2, d)
    for opts in (dict(MDB_HNSW_NO_SPLIT=1, MDB_HNSW_RANK=1), dict(MDB_HNSW_RANK=3), dict(), dict(MDB_HNSW_RANK=0)):
        with options(ctx, **opts):
            expect_nan(lambda: g2.ann_search(q, K, 64))
            for i in range(8):
                expect_nan(lambda: g2.ann_search(q[i:i + 1], K, 64))
            _hnsw_counters(ctx, o, g, q[miss], K, ef, (opts, "clean after the top-layer NaN"))
    g2.close()
    g.close()


def test_hnsw_rows_over_pq_codes_nan_codebook_row(ctx, oracle):
    """BlockBasedHnsw<ProductQuantizer>: a NaN codebook row (s, c*) held by ONE stored point; the queries whose traversal evaluates that
    point error, the others return the oracle's rows and counters"""
    from muopdb_amd.index import BlockBasedHnsw, ProductQuantizer
    n, d, sub, bits_, ef = 1500, 32, 8, 6, 16
    v = H.sift_like(n, d, n_clusters=20, seed=13)
    cb = H.train_pq_codebook(v[:1000], sub, bits_, iters=3).reshape(d // sub, 1 << bits_, sub)
    codes = oracle.ProductQuantizer(d, sub, bits_, cb).quantize(v)
    col = codes[:, S_STAR]
    c_star = int(np.bincount(col, minlength=1 << bits_)[1:].argmax()) + 1
    others = np.delete(np.arange(1 << bits_), c_star)
    c_alt = int(others[((cb[S_STAR, others] - cb[S_STAR, c_star]) ** 2).sum(1).argmin()])
    unused = codes.copy()
    unused[col == c_star, S_STAR] = c_alt
    cb_nan = cb.copy()
    cb_nan[S_STAR, c_star, 2] = np.nan
    opq = oracle.ProductQuantizer(d, sub, bits_, cb_nan)
    _, layers = _graph(oracle, v, 10, 3, 60, seed=3)
    hidx = F.write_hnsw_index(layers, list(range(n)), d // sub)
    rng = np.random.default_rng(17)
    oq, gq = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, sub, bits_, cb_nan), ProductQuantizer(d, sub, bits_, cb_nan)
    found = None
    for p in [x for x in range(200, n, 41) if x not in layers[1]]:
        q = near_queries(v, 64, 19, 3.0)
        q[:16] = v[p] + rng.normal(0, 0.5, (16, d)).astype(np.float32)
        if (opq.quantize(q)[:, S_STAR] == c_star).any():
            continue
        planted = unused.copy()
        planted[p, S_STAR] = c_star
        vf = F.write_vector_file(planted)
        o = oracle.BlockBasedHnsw(hidx, vf, d, oq)
        r = oracle_raises(lambda x: o.ann_search(x, K, ef), q)
        if 8 <= int(r.sum()) <= 56:
            found = (vf, o, r, q)
            break
    assert found, "no point splits the queries"
    vf, o, r, q = found
    hit, miss = groups(r, "hnsw over pq codes")
    g = BlockBasedHnsw(ctx, hidx, vf, d, gq)
    vf_unused = F.write_vector_file(unused)
    g2, o2 = BlockBasedHnsw(ctx, hidx, vf_unused, d, gq), oracle.BlockBasedHnsw(hidx, vf_unused, d, oq)
    for opts in (dict(), dict(MDB_HNSW_NO_BEAM=1)):
        with options(ctx, **opts):
            _hnsw_counters(ctx, o2, g2, q, K, ef, (opts, "no point holds c*"))
            expect_nan(lambda: g.ann_search(q[hit], K, ef))
            _hnsw_counters(ctx, o, g, q[miss], K, ef, (opts, "miss"))
            for i in hit[:8]:
                expect_nan(lambda: g.ann_search(q[i:i + 1], K, ef))
            _hnsw_counters(ctx, o, g, q[miss], K, ef, (opts, "clean"))
    g.close()
    g2.close()


@pytest.mark.parametrize("opts", [dict(), dict(MDB_CLOSURE_NO_STAGE=1), dict(MDB_CLOSURE_BLOCK=256), dict(MDB_HNSW_NO_CLOSURE=1)],
                         ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "default")
@pytest.mark.parametrize("n,ef", [(120, 128), (1200, 1280)])
def test_closure_kernel_reachable_and_unreachable_nan(ctx, oracle, opts, n, ef):
    """Graphs no larger than ef (hnsw_closure_kernel: whole frontiers, every point's distance staged up front).  A NaN point reachable
    from the entry point: every query errors.  The same point with no in-edge in any layer (the graph writer permits it): no query
    errors, although the staging pass computed its distance; rows and counters equal the oracle's.  120 points: the kernel ranks its
    working list by counting (at most 512 keys); 1 200 points, more than 512 of them reachable: the bitonic tail, which raises on its own."""
    from muopdb_amd.index import BlockBasedHnsw
    d = 32
    v = H.sift_like(n, d, n_clusters=6, seed=23)
    hidx0, layers = _graph(oracle, v, 6, 3, 30, seed=2)
    upper = set().union(*[set(l) for l in layers[1:]]) if len(layers) > 1 else set()
    reach = oracle.BlockBasedHnsw(hidx0, F.write_vector_file(v), d).ann_search(v[:1], n, ef).doc_ids(0)   # the closure of the entry point
    assert len(reach) > (512 if n > 512 else 64)
    p = next(x for x in reach[len(reach) // 2:] if x not in upper)
    bad = v.copy()
    bad[p, 9] = np.nan
    vf = F.write_vector_file(bad)
    q = near_queries(v, 24, 29, 3.0)
    docs = list(range(n))
    # reachable
    hidx = F.write_hnsw_index(layers, docs, d)
    o = oracle.BlockBasedHnsw(hidx, vf, d)
    assert oracle_raises(lambda x: o.ann_search(x, K, ef), q).all()
    g = BlockBasedHnsw(ctx, hidx, vf, d)
    # no in-edges
    cut = [{a: [e for e in row if e != p] for a, row in layers[0].items()}] + layers[1:]
    hidx2 = F.write_hnsw_index(cut, docs, d)
    o2 = oracle.BlockBasedHnsw(hidx2, vf, d)
    assert not oracle_raises(lambda x: o2.ann_search(x, K, ef), q).any()
    g2 = BlockBasedHnsw(ctx, hidx2, vf, d)
    with options(ctx, **opts):
        expect_nan(lambda: g.ann_search(q, K, ef))
        for i in range(8):
            expect_nan(lambda: g.ann_search(q[i:i + 1], K, ef))
        _hnsw_counters(ctx, o2, g2, q, K, ef, "no in-edges")
        expect_nan(lambda: g.ann_search(q, n, n))
        _hnsw_counters(ctx, o2, g2, q, n, n, "no in-edges, k = ef = n")
    g.close()
    g2.close()


# =================================================================================== 1. NaN: SPANN, multi-user SPANN
def test_spann_nan_in_a_kept_or_a_pruned_list(ctx, oracle):
    """Spann::search scans the lists the centroid_distance_ratio filter keeps (the default 0.1 of the K10 case): a NaN posting-list
    vector is an error for the queries whose filter keeps its list — not for those that reach the centroid among the num_explored
    nearest and prune it.  Through the closure kernel's own filter tail and through spann_filter_kernel (MDB_CLOSURE_NO_FILTER)."""
    from muopdb_amd.index import SearchParams, Spann
    n, d, nl, ne = 2000, 32, 12, 4
    v = H.sift_like(n, d, n_clusters=12, seed=31)
    files, cent, pls = H.build_spann_files(oracle, v, list(range(n)), nl, seed=3, max_neighbors=8, max_layers=3, ef_construction=40)
    q = near_queries(v, 64, 37, 12.0)
    p, op = SearchParams(K, 40).with_num_explored_centroids(ne), oracle.SearchParams(K, 40, num_explored_centroids=ne)
    ocent = oracle.BlockBasedHnsw(files["hnsw_index"], files["hnsw_vectors"], d)
    near = ocent.ann_search(q, ne, 40)
    explored = np.array([[int(x) for x in near.doc_ids(i)] + [-1] * (ne - int(near.counts[i])) for i in range(len(q))])
    found = None
    for c in np.argsort([-len(x) for x in pls]):
        bad = v.copy()
        bad[pls[c].astype(np.int64)[::3], 1] = np.nan           # every third vector of list c
        fb = dict(files, ivf_vectors=F.write_vector_file(bad))
        o = oracle.Spann(fb["hnsw_index"], fb["hnsw_vectors"], fb["ivf_index"], fb["ivf_vectors"])
        r = oracle_raises(lambda x: o.search(x, op), q)
        pruned = (explored == c).any(1) & ~r
        if 8 <= int(r.sum()) <= 56 and pruned.sum() >= 2:
            found = (fb, o, r, pruned)
            break
    assert found, "no list is kept by some queries and pruned by others"
    fb, o, r, pruned = found
    hit, miss = groups(r, "spann")
    g = Spann(ctx, fb["hnsw_index"], fb["hnsw_vectors"], fb["ivf_index"], fb["ivf_vectors"])
    for opts in (dict(), dict(MDB_CLOSURE_NO_FILTER=1)):
        with options(ctx, **opts):
            expect_nan(lambda: g.search(q[hit], p))
            res, want = g.search(q[miss], p), o.search(q[miss], op)
            assert res.found[:len(miss)].tolist() == want.found.tolist()
            assert_rows_equal(res, want, len(miss), "miss")
            for i in hit[:8]:
                expect_nan(lambda: g.search(q[i:i + 1], p))
            assert_rows_equal(g.search(q[miss], p), want, len(miss), "clean")
    g.close()


def test_multi_user_spann_nan_in_one_users_data(ctx, oracle):
    """NaN rows in user A's posting lists only: a batch of user-B queries is clean, a mixed batch errors, the next user-B batch is
    clean again — host calls and one submit / wait"""
    from muopdb_amd.index import MultiSpannIndex, SearchParams
    d, A, B = 32, 5, 9
    per_user, qs = {}, {}
    for j, u in enumerate((A, B)):
        uv = H.sift_like(600, d, n_clusters=10, seed=41 + j)
        f, _, _ = H.build_spann_files(oracle, uv, [1000 * u + i for i in range(len(uv))], 8, seed=j, max_neighbors=8, max_layers=3,
                                      ef_construction=40)
        if u == A:
            bad = uv.copy()
            bad[::5, 2] = np.nan
            f = dict(f, ivf_vectors=F.write_vector_file(bad), ivf_raw_vectors=F.write_vector_file(bad))
        per_user[u] = f
        qs[u] = near_queries(uv, 16, 43 + j, 3.0)
    cat = F.concat_multi_spann(per_user)
    margs = (cat["user_table"], d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    g, o = MultiSpannIndex(ctx, *margs), oracle.MultiSpannIndex(*margs)
    p, op = SearchParams(K, 40).with_num_explored_centroids(4), oracle.SearchParams(K, 40, num_explored_centroids=4)
    assert oracle_raises(lambda x: o.search_for_user([A], x, op), qs[A]).sum() >= 8
    want_b = o.search_for_user([B] * 16, qs[B], op)
    mixed_users = [A if i % 2 else B for i in range(32)]
    mixed_q = np.stack([qs[A][i // 2] if i % 2 else qs[B][i // 2] for i in range(32)])
    assert_rows_equal(g.search_for_user([B] * 16, qs[B], p), want_b, 16, "user B first")
    expect_nan(lambda: g.search_for_user(mixed_users, mixed_q, p))
    assert_rows_equal(g.search_for_user([B] * 16, qs[B], p), want_b, 16, "user B after the mixed batch")
    expect_nan(lambda: g.search_for_user([A] * 16, qs[A], p))
    expect_nan(lambda: g.search_for_user_submit(mixed_users, mixed_q, p).wait())
    assert_rows_equal(g.search_for_user_submit([B] * 16, qs[B], p).wait(), want_b, 16, "user B after the failed wait")
    g.close()


# =================================================================================== 1. NaN: build entries
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "dot"])
def test_select_neighbors_nan_candidate(ctx, oracle, metric):
    """mdb_hnsw_select_neighbors: a NaN vector among a row's candidates (behind the first kept one, so that a kept point's distance to
    it is evaluated) is MDB_ERR_NAN — in the reference the builder has panicked before, where search_layer wrapped that candidate's
    distance in NotNan.  The same vector present in `vectors` but named by no candidate list: MDB_OK and the rows of the clean copy."""
    from muopdb_amd import build as B
    rng = np.random.default_rng(8 + metric)
    n, d, M, W = 400, 24, 8, 24
    x = H.sift_like(n, d, n_clusters=6, seed=5)
    if metric:
        x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    dist_fn = oracle.dot if metric else oracle.l2
    nan_pt = 399
    cand = np.full((40, W), 0xFFFFFFFF, np.uint32)
    dist = np.full((40, W), np.inf, np.float32)
    for r in range(40):
        c = rng.choice(nan_pt, size=int(rng.integers(4, W + 1)), replace=False)      # never the NaN point
        dd = np.array([dist_fn(x[r], x[j]) for j in c], np.float32)
        order = np.lexsort((-c.astype(np.int64), dd))
        cand[r, :len(c)], dist[r, :len(c)] = c[order], dd[order]
    want = B.select_neighbors(ctx, x, cand, dist, M, metric=metric)
    bad = x.copy()
    bad[nan_pt, 4] = np.nan
    got = B.select_neighbors(ctx, bad, cand, dist, M, metric=metric)                 # present, in no list
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    cand2, dist2 = cand.copy(), dist.copy()
    cand2[7, 1] = nan_pt                                                             # second in pop order: d(kept[0], NaN point) is evaluated
    expect_nan(lambda: B.select_neighbors(ctx, bad, cand2, dist2, M, metric=metric))
    again = B.select_neighbors(ctx, bad, cand, dist, M, metric=metric)               # the flag does not survive the error
    for a, b in zip(again, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.isnan(B.select_neighbors(ctx, x, cand2, dist2, M, metric=metric)[1]).any()   # the same lists over clean rows


def test_ivf_assign_nan(ctx, oracle):
    """mdb_ivf_assign: a NaN vector row errors, as the oracle's "NaN distance" does.  A NaN CENTROID is not pinned by the oracle (its
    restatement skips NaN distances of a row and reports them at the end, the reference's select_nth over NotNan panics): the library
    evaluates every (vector, centroid) pair and reports MDB_ERR_NAN, at a batch of <= 4 vectors and beyond"""
    from muopdb_amd.index import ivf_assign
    v = H.sift_like(300, D, n_clusters=8, seed=51)
    cent = H.kmeans(v, 12, iters=3, seed=5)
    bad = v.copy()
    bad[123, 0] = np.nan
    with pytest.raises(ValueError):
        oracle.ivf_assign(cent, bad, 2, 0.1)
    expect_nan(lambda: ivf_assign(ctx, cent, bad, 2, 0.1))
    expect_nan(lambda: ivf_assign(ctx, cent, bad[122:125], 2, 0.1))
    ids, cnt = ivf_assign(ctx, cent, v, 2, 0.1)
    oids, ocnt = oracle.ivf_assign(cent, v, 2, 0.1)
    assert np.array_equal(ids, oids) and np.array_equal(cnt, ocnt)
    bad_cent = cent.copy()
    bad_cent[11, 3] = np.nan
    expect_nan(lambda: ivf_assign(ctx, bad_cent, v, 2, 0.1))
    expect_nan(lambda: ivf_assign(ctx, bad_cent, v[:3], 2, 0.1))
    ids, cnt = ivf_assign(ctx, cent, v[:3], 2, 0.1)
    assert np.array_equal(ids, oids[:3]) and np.array_equal(cnt, ocnt[:3])


# =================================================================================== 1. NaN: calling conventions
def _dev_outs(torch, dev, b, k):
    t = (torch.zeros((b, k, 2), dtype=torch.int64, device=dev), torch.zeros((b, k), dtype=torch.float32, device=dev),
         torch.zeros(b, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    return t


def _dev_result(ids, sc, cn):
    from muopdb_amd.index import SearchResult
    h = ids.cpu().numpy().view(np.uint64)
    return SearchResult(h.shape[0], h.shape[1], h[:, :, 0], h[:, :, 1], sc.cpu().numpy(), cn.cpu().numpy().view(np.uint32))


def test_device_memory_calls_defer_the_error_to_sync(ctx, oracle, pq, hnsw_world):
    """MDB_MEM_DEVICE: the call returns MDB_OK, mdb_sync returns MDB_ERR_NAN once, the next mdb_sync MDB_OK — IVF-PQ and HNSW"""
    torch = pytest.importorskip("torch")
    from muopdb_amd import lib as L
    dev = torch.device("cuda", torch.cuda.current_device())
    w = pq
    q, hit, miss, P = w["q"], w["hit"], w["miss"], w["P"]

    def ivf_call(sel):
        qd = torch.from_numpy(np.ascontiguousarray(q[sel])).to(dev)
        outs = _dev_outs(torch, dev, len(sel), K)
        ctx.check(ctx.lib.mdb_ivf_search(w["g_planted"].h, C.c_void_p(qd.data_ptr()), C.c_size_t(len(sel)), None, C.c_size_t(P), C.c_size_t(K),
                                         C.c_int(L.MEM_DEVICE), *[C.c_void_p(t.data_ptr()) for t in outs]))      # MDB_OK here
        return outs, qd
    for opts in (dict(), dict(MDB_PQ_NO_FUSED=1)):
        with options(ctx, **opts):
            keep = ivf_call(hit)
            expect_nan(ctx.sync)
            ctx.sync()
            outs, keep = ivf_call(miss)
            ctx.sync()
            assert_rows_equal(_dev_result(*outs), w["o_planted"].search(q[miss], K, num_probes=P), len(miss), "ivf-pq device miss")
    hw = hnsw_world["upper"]
    hq = hw["q"]
    hhit, hmiss = groups(hw["raises"][16], "hnsw device")

    def hnsw_call(sel):
        qd = torch.from_numpy(np.ascontiguousarray(hq[sel])).to(dev)
        outs = _dev_outs(torch, dev, len(sel), K)
        hw["g"].ann_search_device(qd.data_ptr(), len(sel), K, 16, *[t.data_ptr() for t in outs])
        return outs, qd
    keep = hnsw_call(hhit)
    expect_nan(ctx.sync)
    ctx.sync()
    outs, keep = hnsw_call(hmiss)
    ctx.sync()
    assert_rows_equal(_dev_result(*outs), hw["o"].ann_search(hq[hmiss], K, 16), len(hmiss), "hnsw device miss")


def test_submit_wait_on_an_attached_handle_errors_alone(ctx, oracle, pq, hnsw_world):
    """submit / wait on a handle attached to a second context while the root handle serves the miss batch from another thread: only the
    attached context reports MDB_ERR_NAN"""
    from muopdb_amd import lib as L
    ctx2 = L.Context(0)
    try:
        for kind in ("ivf", "hnsw"):
            if kind == "ivf":
                w = pq
                q, hit, miss = w["q"], w["hit"], w["miss"]
                root, want = w["g_planted"], w["o_planted"].search(q[miss], K, num_probes=w["P"])
                att = root.attach(ctx2)
                submit = lambda sel: att.search_submit(q[sel], K, w["P"])                     # noqa: E731
                serve = lambda: root.search(q[miss], K, w["P"])                               # noqa: E731
            else:
                hw = hnsw_world["upper"]
                q = hw["q"]
                hit, miss = groups(hw["raises"][16], "hnsw attach")
                root, want = hw["g"], hw["o"].ann_search(q[miss], K, 16)
                att = root.attach(ctx2)
                submit = lambda sel: att.ann_search_submit(q[sel], K, 16)                     # noqa: E731
                serve = lambda: root.ann_search(q[miss], K, 16)                               # noqa: E731
            got = {}

            def worker():
                try:
                    got["rows"] = [serve() for _ in range(3)]
                except Exception as e:       # reported by the assertion below
                    got["error"] = e
            pending = submit(hit)
            t = threading.Thread(target=worker)
            t.start()
            expect_nan(pending.wait)
            t.join()
            assert "error" not in got, got.get("error")
            for res in got["rows"]:
                assert_rows_equal(res, want, len(miss), kind + " root handle")
            assert_rows_equal(submit(miss).wait(), want, len(miss), kind + " attached handle after its error")
            att.close()
    finally:
        ctx2.close()


# =================================================================================== 2. +-inf and zeros
N_INF, L_INF, P_INF = 2048, 64, 2


@pytest.fixture(scope="module")
def inf_world(oracle):
    """2 048 x 32 in 64 lists (about 32 points each: two probes reach about 64 points, 56 of them finite), rows >= 1 in every
    coordinate so that no product with an infinity is 0 x inf"""
    v = H.sift_like(N_INF, D, n_clusters=20, seed=61) + 1.0
    cent = H.kmeans(v, L_INF, iters=3, seed=6)
    docs = [5 + 2 * i for i in range(N_INF)]
    index, vec, pls = H.build_ivf_files(v, docs, cent)
    q = np.abs(near_queries(v, 40, 63, 3.0)) + 1.0
    return dict(v=v.astype(np.float32), index=index, vec=vec, pls=pls, q=q.astype(np.float32), docs=docs)


def _ivf_pair(ctx, oracle, index, vec, metric):
    from muopdb_amd.index import BlockBasedIvf, NoQuantizer
    return (BlockBasedIvf(ctx, index, vec, NoQuantizer(D, metric)), oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_NONE, metric)))


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "dot"])
def test_ivf_f32_infinite_rows(ctx, oracle, inf_world, metric):
    """One stored point in eight has an infinite coordinate (L2: +inf, every such distance +inf; dot: +inf or -inf, so that some
    points rank first with score -inf and some last with +inf).  k = 60 exceeds the finite points two probes reach: infinite points
    enter the rows and tie by id; a FULL row whose tail is +inf has counts == k — not a short row padded with +inf and the all-ones id"""
    w = inf_world
    v, q = w["v"].copy(), w["q"]
    rng = np.random.default_rng(67)
    rows = np.arange(3, N_INF, 8)
    cols = rng.integers(0, D, len(rows))
    v[rows, cols] = np.inf if metric == 0 else np.where(np.arange(len(rows)) % 2, np.inf, -np.inf)
    cls = pair_classes(q, v, metric)
    assert not (cls == "n").any() and (cls == "p").any() and ((cls == "m").any() == (metric == 1))
    g, o = _ivf_pair(ctx, oracle, w["index"], F.write_vector_file(v), metric)
    full_inf_tail = 0
    for k in (10, 60, 64, 100):
        for opts in (dict(), dict(MDB_SCAN_F32_NSPLIT=3), dict(MDB_SCAN_F32_NSPLIT=1, MDB_SCAN_F32_BLK=64)):
            with options(ctx, **opts):
                res = g.search(q, k, P_INF)
            want = o.search(q, k, num_probes=P_INF)
            assert_rows_equal(res, want, len(q), (k, opts))
        full_inf_tail += sum(1 for i in range(len(q)) if int(want.counts[i]) == k and np.isposinf(want.scores[i, k - 1]))
        if k == 100:
            assert (want.counts < k).any()           # short rows exist too: the padding behind them is not compared
    assert full_inf_tail >= 8, "no full row ends in +inf scores"
    if metric == 1:
        assert np.isneginf(want.scores[:, 0]).any()
    g.close()


def test_ivf_f32_infinite_query_coordinate(ctx, oracle, inf_world):
    """an infinite query coordinate over finite rows: every L2 distance is +inf, the row is the first k candidates in id order"""
    w = inf_world
    q = w["q"].copy()
    q[::3, 4] = np.inf
    q[1::6, 9] = -np.inf
    assert not (pair_classes(q, w["v"], 0) == "n").any()
    g, o = _ivf_pair(ctx, oracle, w["index"], w["vec"], 0)
    pr = o.find_nearest_centroids(w["q"], P_INF)          # (probes of the finite queries: the coarse search is not under test here)
    for k in (10, 60):
        want = o.search(q, k, probes=pr)
        assert_rows_equal(g.search_with_centroids_and_remap(q, pr, k), want, len(q), k)
        assert np.isposinf(want.scores[0, :int(want.counts[0])]).all()
        reach = np.sort(np.concatenate([w["pls"][c] for c in pr[0]]).astype(np.int64))
        assert want.doc_ids(0) == [w["docs"][p] for p in reach[:k]]
    # through the library's own coarse search: every centroid distance is +inf, the probes are the first lists by id
    res = g.search(q[:1], 10, P_INF)
    first = np.sort(np.concatenate([w["pls"][c] for c in range(P_INF)]).astype(np.int64))
    assert res.doc_ids(0) == [w["docs"][p] for p in first[:10]] and np.isposinf(res.scores[0, :10]).all()
    g.close()


def test_ivf_f32_exact_duplicates_of_the_query(ctx, oracle, inf_world):
    """several stored rows per probed list equal the query: L2 score bits 0x00000000, ties by id"""
    w = inf_world
    v, q = w["v"].copy(), w["q"]
    o0 = oracle.BlockBasedIvf(w["index"], w["vec"])
    pr = o0.find_nearest_centroids(q, P_INF)
    taken = set()
    for i in range(12):
        for c in pr[i]:
            cand = [int(p) for p in w["pls"][c] if int(p) not in taken][:3]
            taken.update(cand)
            v[cand] = q[i]
    g, o = _ivf_pair(ctx, oracle, w["index"], F.write_vector_file(v), 0)
    want = o.search(q, 10, probes=pr)
    assert_rows_equal(g.search_with_centroids_and_remap(q, pr, 10), want, len(q))
    for i in range(12):
        assert bits(want.scores[i, :3]).tolist() == [0, 0, 0] and want.doc_ids(i)[:3] == sorted(want.doc_ids(i)[:3])
    g.close()


def test_ivf_f32_dot_zeros_tiny_and_denormal_products(ctx, oracle, inf_world):
    """dot product: zero rows and rows orthogonal to the query by construction (disjoint supports) score -0.0 (bits 0x80000000),
    interleaved with rows whose dot is +-1e-30 and rows whose products are denormal: order and bits equal the oracle's"""
    w = inf_world
    rng = np.random.default_rng(71)
    v = rng.standard_normal((N_INF, D)).astype(np.float32)
    q = np.zeros((40, D), np.float32)
    q[:, :16] = rng.standard_normal((40, 16)).astype(np.float32)
    q[:, 2] = np.float32(1e-3) * np.sign(q[:, 2])
    kinds = np.arange(N_INF) % 8
    v[kinds == 0] = 0.0                                                   # zero rows
    v[kinds == 1, :16] = 0.0                                              # support disjoint from the queries'
    v[kinds == 2] = 0.0
    v[kinds == 2, 0] = np.float32(1e-30)                                  # dot = 1e-30 q0
    v[kinds == 3] = 0.0
    v[kinds == 3, 1] = np.float32(-1e-30)
    v[kinds == 4] = 0.0
    v[kinds == 4, 2] = np.float32(1e-38)                                  # product 1e-41: denormal
    v[kinds == 5] = 0.0
    v[kinds == 5, 2] = np.float32(-1e-38)
    v[kinds == 5, 0] = np.float32(1e-44)                                  # a denormal operand too
    g, o = _ivf_pair(ctx, oracle, w["index"], F.write_vector_file(v), 1)
    pr = np.stack([rng.choice(L_INF, P_INF, replace=False) for _ in range(40)]).astype(np.uint32)
    for k in (10, 64):
        want = o.search(q, k, probes=pr)
        assert_rows_equal(g.search_with_centroids_and_remap(q, pr, k), want, len(q), k)
    allbits = np.concatenate([bits(want.scores[i, :int(want.counts[i])]) for i in range(40)])
    assert (allbits == 0x80000000).sum() >= 40 and ((allbits & 0x7F800000) == 0).sum() > (allbits == 0x80000000).sum()   # -0.0, and denormals
    g.close()


HNSW_INF_FORMS = [("beam", dict()), ("rank0", dict(MDB_HNSW_RANK=0)), ("rank3", dict(MDB_HNSW_RANK=3)), ("no_table", dict(MDB_HNSW_NO_TABLE=1)),
                  ("general", dict(MDB_HNSW_NO_BEAM=1)), ("no_split", dict(MDB_HNSW_NO_SPLIT=1))]


@pytest.fixture(scope="module")
def hnsw_inf_world(oracle):
    """280 points, M = 8, 3 layers: ef = 256 exceeds the finite points a traversal can reach (about 190 of the 215 reachable ones), and
    stays below n (no closure kernel)"""
    n = 280
    v = H.sift_like(n, D, n_clusters=6, seed=73) + 1.0
    graphs = {m: _graph(oracle, v, 8, 3, 40, metric=m)[0] for m in (0, 1)}
    q = (np.abs(near_queries(v, 40, 79, 3.0)) + 1.0).astype(np.float32)
    return dict(n=n, v=v.astype(np.float32), graphs=graphs, q=q)


def _hnsw_pair(ctx, oracle, hidx, vf, metric, d=D):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    return BlockBasedHnsw(ctx, hidx, vf, d, NoQuantizer(d, metric)), oracle.BlockBasedHnsw(hidx, vf, d, oracle.Quant(oracle.QUANT_NONE, metric))


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "dot"])
@pytest.mark.parametrize("form,opts", HNSW_INF_FORMS, ids=[f[0] for f in HNSW_INF_FORMS])
def test_hnsw_infinite_rows(ctx, oracle, hnsw_inf_world, form, opts, metric):
    """One point in eight has an infinite coordinate; ef = 256 exceeds the finite points a traversal reaches, so it walks
    `d < furthest || len < ef` with furthest = +inf and the beam compacts by a bound at the image of +inf (0xFF800000, next to the
    empty-slot sentinel 0xFFFFFFFF): rows with +inf tails tied by id — full ones (counts == k = 200) and short ones (k = 256) — and
    both counters equal the oracle's"""
    w = hnsw_inf_world
    v, q, n = w["v"].copy(), w["q"], w["n"]
    rows = np.arange(5, n, 8)
    cols = np.random.default_rng(83).integers(0, D, len(rows))
    v[rows, cols] = np.inf if metric == 0 else np.where(np.arange(len(rows)) % 2, np.inf, -np.inf)
    assert not (pair_classes(q, v, metric) == "n").any()
    g, o = _hnsw_pair(ctx, oracle, w["graphs"][metric], F.write_vector_file(v), metric)
    with options(ctx, **opts):
        for k, ef in ((256, 256), (200, 256), (10, 16), (64, 100)):
            _hnsw_counters(ctx, o, g, q, k, ef, (form, k, ef))
    want = o.ann_search(q, 200, 256)
    if metric == 0:     # the cases above are not vacuous: full rows that end in +inf scores
        assert int(((want.counts == 200) & np.isposinf(want.scores[:, -1])).sum()) >= 8
    else:               # ... rows that begin with -inf scores
        assert int(np.isneginf(want.scores[:, 0]).sum()) >= 8
    g.close()


@pytest.mark.parametrize("form,opts", HNSW_INF_FORMS, ids=[f[0] for f in HNSW_INF_FORMS])
def test_hnsw_infinite_query_and_duplicates_of_the_query(ctx, oracle, hnsw_inf_world, form, opts):
    """an infinite query coordinate (every L2 distance +inf: the whole traversal runs on ties) and stored duplicates of the query
    (distance bits 0x00000000, ties by id) — rows and counters"""
    w = hnsw_inf_world
    v, n = w["v"].copy(), w["n"]
    q = w["q"].copy()
    near = oracle.BlockBasedHnsw(w["graphs"][0], F.write_vector_file(v), D).ann_search(q, 40, 256)
    dup, taken = {}, set()
    for i in range(0, 24, 2):      # three reachable points near query i become copies of it
        dup[i] = sorted([p for p in near.doc_ids(i) if p not in taken][:3])
        taken.update(dup[i])
        v[dup[i]] = q[i]
    q[1::4, 6] = np.inf
    assert not (pair_classes(q, v, 0) == "n").any()
    g, o = _hnsw_pair(ctx, oracle, w["graphs"][0], F.write_vector_file(v), 0)
    with options(ctx, **opts):
        for k, ef in ((10, 16), (20, 100), (256, 256)):
            _hnsw_counters(ctx, o, g, q, k, ef, (form, k, ef))
    want = o.ann_search(q, 256, 256)
    for i, pts in dup.items():
        assert want.doc_ids(i)[:3] == pts and bits(want.scores[i, :3]).tolist() == [0, 0, 0]
    assert np.isposinf(want.scores[1, :int(want.counts[1])]).all()
    g.close()


@pytest.mark.parametrize("form,opts", HNSW_INF_FORMS, ids=[f[0] for f in HNSW_INF_FORMS])
def test_hnsw_dot_zeros_tiny_and_denormal_products(ctx, oracle, hnsw_inf_world, form, opts):
    """dot product over the graph built from the clean rows: zero rows and rows orthogonal to the queries by construction (score -0.0,
    bits 0x80000000) interleaved with rows whose dot is +-1e-30 and rows whose products are denormal — the traversal's order (ties
    by id), the rows' score bits and both counters equal the oracle's"""
    w = hnsw_inf_world
    n = w["n"]
    rng = np.random.default_rng(89)
    v = rng.standard_normal((n, D)).astype(np.float32)
    q = np.zeros((40, D), np.float32)
    q[:, :16] = rng.standard_normal((40, 16)).astype(np.float32)
    q[:, 2] = np.float32(1e-3) * np.sign(q[:, 2])
    kinds = np.arange(n) % 8
    v[kinds == 0] = 0.0
    v[kinds == 1, :16] = 0.0
    for kind, col, val in ((2, 0, 1e-30), (3, 1, -1e-30), (4, 2, 1e-38), (5, 2, -1e-38)):
        v[kinds == kind] = 0.0
        v[kinds == kind, col] = np.float32(val)
    v[kinds == 5, 0] = np.float32(1e-44)
    g, o = _hnsw_pair(ctx, oracle, w["graphs"][1], F.write_vector_file(v), 1)
    with options(ctx, **opts):
        for k, ef in ((10, 16), (64, 100), (256, 256)):
            _hnsw_counters(ctx, o, g, q, k, ef, (form, k, ef))
    want = o.ann_search(q, 256, 256)
    allbits = np.concatenate([bits(want.scores[i, :int(want.counts[i])]) for i in range(40)])
    assert (allbits == 0x80000000).sum() >= 40 and ((allbits & 0x7F800000) == 0).sum() > (allbits == 0x80000000).sum()
    g.close()

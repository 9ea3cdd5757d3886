"""Parity at the k, ef, probe and shard-merge capacity limits (-m gpu).

Every search path sizes its on-chip state from the caller's k, ef, num_probes or world: BlockSelect<BLOCK>::cap_for(k) (the smallest
power of two >= k + BLOCK, mdb_device.hip.h:312-317), the HNSW working set and candidate ring (mdb_hnsw.hip:1749-1752), the three
merges behind a split scan (mdb_ivf.hip:559-570), the PQ scans' LDS budgets (mdb_ivf.hip:436-442, 471-473) and the shard merges'
(mdb_ivf.hip:750-751, mdb_spann.hip:314-315).  The C ABI accepts k <= MDB_MAX_K = 2048, ef <= 4096, num_probes <= 2048 where the
probes are SELECTED (explicit probe lists may be longer), node degree <= 256, <= 255 layers, max_neighbors <= 64.  A bug at one of
these edges leaves small-k parity intact, so every form is crossed with the size axis here: rows, counts and score bits against
the oracle (HNSW: the traversal counters too), at the smallest shapes at which the limit is reachable, and one step past every
limit the refusal — status and mdb_last_error text — followed by a valid call on the same handle.

Every refusal tested here is decided on the host before a launch; nothing here overflows a kernel's state on purpose (the HNSW
rows are integer-valued with a range wide enough that ties stay far below the candidate ring's slack of 192).

Thresholds (recomputed from the formulas cited next to each parametrization; LDS budgets in bytes):
  f32 scan merges      nsplit * k * 8 <= 49152 -> merge_sorted_rows (nsplit = 3 at k = 2048: exactly 49152), else merge_keys
                       (nsplit * k >= 2048 keys per query: its 1024-thread form); on a device-memory SPANN call
                       nsplit * k * 8 + k * 28 + 16 <= 49152 -> merge_rows_remap_kernel: k <= 1116 / 818 / 534 at nsplit 2 / 4 / 8
  PQ, 128 KB codebook  pq2 (+ bound filter, L2) up to k = 1024; ivf_scan_pq_kernel<.., LUT = true> up to k = 1792; LUT = false above
  PQ, 64 KB codebook   pq2 for every k <= 2048
  HNSW                 cand_cap = 1024 up to ef = 832, 2048 up to 1856, 4096 up to 3904, 8192 above; closure kernel: n <= ef, n <= 4096
  mdb_*_merge_shards   world * k * 8 + k * 20 + (world + 1) * 4 + 16 <= 153600: k <= 2048 (MDB_MAX_K) at world 2 and 4, 1827 at world 8
  mdb_merge_shards     world * k * 20 + (world + 1) * 4 + 16 <= 153600: k <= 3839 / 1919 / 959 at world 2 / 4 / 8 (no MDB_MAX_K check)
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H
from tests.test_gpu_parity import assert_result_rows

pytestmark = pytest.mark.gpu

UNSUPPORTED, OUT_OF_RANGE = 7, 8          # MDB_ERR_UNSUPPORTED, MDB_ERR_OUT_OF_RANGE
MAX_K, MAX_EF = 2048, 4096
ALL_ONES = 0xFFFFFFFFFFFFFFFF
INF_BITS = 0x7F800000


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
def refused(ctx, call, status, text):
    """`call` fails with `status`, and the context's mdb_last_error holds `text`"""
    from muopdb_amd import lib as L
    with pytest.raises(L.MuopdbError) as e:
        call()
    assert e.value.status == status, e.value
    assert text in str(e.value), e.value
    assert text in (ctx.lib.mdb_last_error(ctx.h) or b"").decode()


def assert_padding(res, b, k):
    """behind its count a row holds doc id 2^128 - 1 and score +inf"""
    for i in range(b):
        c = int(res.counts[i])
        if c < k:
            assert np.all(np.asarray(res.doc_lo[i, c:k]) == ALL_ONES) and np.all(np.asarray(res.doc_hi[i, c:k]) == ALL_ONES), i
            assert np.all(np.ascontiguousarray(res.scores[i, c:k], np.float32).view(np.uint32) == INF_BITS), i


def near(v, b, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    return (v[rng.integers(0, len(v), b)] + rng.normal(0, sigma, (b, v.shape[1]))).astype(np.float32)


def doc_ids_for(n, base=100):
    return [base + 3 * i + ((i % 7) << 70) for i in range(n)]


def hnsw_parity(ctx, g, o, q, k, ef):
    """rows, counts, score bits and the traversal counters of one ann_search against the oracle's"""
    o.stats()
    want = o.ann_search(q, k, ef)
    evals, expanded = o.stats()
    ctx.stats()
    got = g.ann_search(q, k, ef)
    st = ctx.stats()
    assert_result_rows(got, want, len(q))
    assert (st["distance_evals"], st["expanded_nodes"]) == (evals, expanded), (k, ef)


def device_rows(torch, b, k):
    dev = torch.device("cuda", torch.cuda.current_device())
    ke = max(k, 1)
    return (torch.zeros((b, ke, 2), dtype=torch.int64, device=dev), torch.zeros((b, ke), dtype=torch.float32, device=dev),
            torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.uint8, device=dev))


def rows_to_result(b, k, ids, sc, cn, fo=None):
    from muopdb_amd.index import SearchResult
    h = ids.cpu().numpy().view(np.uint64)
    return SearchResult(b, k, h[:, :, 0], h[:, :, 1], sc.cpu().numpy(), cn.cpu().numpy().view(np.uint32),
                        None if fo is None else fo.cpu().numpy())


def spann_search_device(ctx, handle, q, params, users=None):
    """mdb_spann_search / mdb_multi_spann_search with device-resident queries and outputs; the status is returned at once, the
    rows after mdb_sync"""
    import torch
    from muopdb_amd import lib as L
    b, k = len(q), params.top_k
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    ids, sc, cn, fo = device_rows(torch, b, k)
    torch.cuda.synchronize()
    pc = params.to_c()
    tail = [C.c_void_p(qd.data_ptr()), C.c_size_t(b), C.byref(pc), C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()),
            C.c_void_p(sc.data_ptr()), C.c_void_p(cn.data_ptr()), C.c_void_p(fo.data_ptr())]
    if users is None:
        ctx.check(ctx.lib.mdb_spann_search(handle.h, *tail))
    else:
        ctx.check(ctx.lib.mdb_multi_spann_search(handle.h, L.u128_array(list(users)), *tail))
    ctx.sync()
    return rows_to_result(b, k, ids, sc, cn, fo)


# =================================================================================== 2. IVF, f32 posting lists
# every step of cap_for(k) = pow2 >= k + BLOCK for BLOCK = 64, 128, 256 (mdb_device.hip.h:312-317), and both ends
K_SWEEP = [0, 1, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 448, 449, 768, 769, 896, 897, 960, 961, 1024, 1025, 1792, 1793,
           1920, 1921, 1984, 1985, 2047, 2048]
N_F32, D_F32, L_F32 = 5000, 20, 8


def _f32_world(ctx, oracle, v, cent, docs, cpv=1):
    from muopdb_amd.index import BlockBasedIvf, NoQuantizer
    index, vec, pls = H.build_ivf_files(v, docs, cent, clusters_per_vector=cpv)
    w = dict(index=index, vec=vec, pls=pls, v=v, cent=cent, docs=docs)
    for name, m in (("l2", 0), ("dot", 1)):
        w["o_" + name] = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_NONE, m))
        w["g_" + name] = BlockBasedIvf(ctx, index, vec, NoQuantizer(v.shape[1], m))
    return w


@pytest.fixture(scope="module")
def f32(ctx, oracle):
    """5 000 x 20 (d not a multiple of 4) in 8 lists; with all 8 probed every row fills to 2 048.  `dup`: the same vectors with
    max_clusters_per_vector = 2 (every point in two lists); `short`: 300 points."""
    v = H.sift_like(N_F32, D_F32, n_clusters=8, seed=41)
    cent = H.kmeans(v, L_F32, iters=3, seed=42)
    docs = doc_ids_for(N_F32)
    w = _f32_world(ctx, oracle, v, cent, docs)
    w["dup"] = _f32_world(ctx, oracle, v, cent, docs, cpv=2)
    w["short"] = _f32_world(ctx, oracle, v[:300], cent, docs[:300])
    w["q"] = near(v, 8, 43)
    yield w
    for x in (w, w["dup"], w["short"]):
        x["g_l2"].close()
        x["g_dot"].close()


@pytest.mark.parametrize("blk", [64, 128, 256, 0])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ivf_f32_k_sweep(ctx, f32, metric, blk):
    """ivf_scan_f32_kernel<M, 64 | 128 | 256> (MDB_SCAN_F32_BLK) over every step of its selector's capacity.  0 is the default: the
    128-thread block at batch <= 256 and the 256-thread one above (mdb_ivf.hip:548), so 256 is forced here to stay at batch 8."""
    g, o, q = f32["g_" + metric], f32["o_" + metric], f32["q"]
    with options(ctx, MDB_SCAN_F32_BLK=blk):
        for k in K_SWEEP:
            got = g.search(q, k, L_F32)
            assert_result_rows(got, o.search(q, k, num_probes=L_F32), len(q))
            if k:
                assert np.all(got.counts == k), k          # 5 000 candidates: every row is full


@pytest.mark.parametrize("nsplit,cols", [(3, 8),      # 3 * 2048 * 8 = 49 152 bytes: the last case of merge_sorted_rows (mdb_ivf.hip:568)
                                         (4, 8),      # 65 536 bytes: merge_keys (:569), 8 192 keys per query
                                         (16, 16)])   # 32 768 keys per query: merge_keys_kernel<1024>.  nsplit is capped by the number
#                                                       of probe columns (:430), so each of the 8 lists is probed twice (no dedup)
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ivf_f32_merge_forms_at_k_2048(ctx, f32, metric, nsplit, cols):
    g, o, q = f32["g_" + metric], f32["o_" + metric], f32["q"]
    probes = np.tile(np.arange(L_F32, dtype=np.uint32), (len(q), cols // L_F32))
    with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit):
        for k in (MAX_K, MAX_K - 1):
            assert_result_rows(g.search_with_centroids_and_remap(q, probes, k), o.search(q, k, probes=probes), len(q))


def test_ivf_f32_short_rows_are_padded(ctx, f32):
    """k = 2 048 over 300 scanned points (and over one list of them): counts and the padding behind them, in every merge form"""
    w, q = f32["short"], f32["q"]
    one = np.full((len(q), 1), int(np.argmax([len(p) for p in w["pls"]])), np.uint32)
    for metric in ("l2", "dot"):
        g, o = w["g_" + metric], w["o_" + metric]
        for nsplit in (0, 1, 3, 4, 8):
            with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit):
                got, want = g.search(q, MAX_K, L_F32), o.search(q, MAX_K, num_probes=L_F32)
                assert_result_rows(got, want, len(q))
                assert np.all(got.counts == 300)
                assert_padding(got, len(q), MAX_K)
        got = g.search_with_centroids_and_remap(q, one, MAX_K)
        assert_result_rows(got, o.search(q, MAX_K, probes=one), len(q))
        assert 0 < int(got.counts[0]) < 300
        assert_padding(got, len(q), MAX_K)


@pytest.mark.parametrize("nsplit", [0, 3, 4])
def test_ivf_f32_duplicates_at_k_2048(ctx, f32, nsplit):
    """max_clusters_per_vector = 2: every point sits in two probed lists and is returned twice, with equal keys"""
    w, q = f32["dup"], f32["q"]
    with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit):
        for metric in ("l2", "dot"):
            for k in (MAX_K, 1025):
                got = w["g_" + metric].search(q, k, L_F32)
                assert_result_rows(got, w["o_" + metric].search(q, k, num_probes=L_F32), len(q))
    assert len(set(got.doc_ids(0))) < len(got.doc_ids(0))


def test_ivf_f32_masks_at_k_2048(ctx, oracle, f32):
    """tombstones, and a per-query filter that leaves fewer than k points, at k = 2 048"""
    from muopdb_amd.index import BlockBasedIvf, allow_bitmap
    q = f32["q"]
    g, o = BlockBasedIvf(ctx, f32["index"], f32["vec"]), oracle.BlockBasedIvf(f32["index"], f32["vec"])
    first = o.search(q, MAX_K, num_probes=L_F32)
    dead = sorted({d for i in range(len(q)) for d in first.doc_ids(i)[:40:3]})
    for doc in dead:
        assert g.invalidate(doc) and o.invalidate(doc)
    rng = np.random.default_rng(7)
    bms = np.stack([allow_bitmap(np.sort(rng.choice(N_F32, 1500 + 10 * i, replace=False)), N_F32) for i in range(len(q))])
    for nsplit in (0, 3, 4):
        with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit):
            assert_result_rows(g.search(q, MAX_K, L_F32), o.search(q, MAX_K, num_probes=L_F32), len(q))
            with oracle.planner_filter(bms):
                want = o.search(q, MAX_K, num_probes=L_F32)
            got = g.search(q, MAX_K, L_F32, planner=bms)
            assert_result_rows(got, want, len(q))
            assert np.all(got.counts < 1600) and np.all(got.counts > 1000)
            assert_padding(got, len(q), MAX_K)
    g.close()


@pytest.fixture(scope="module")
def spann8(ctx, oracle, f32):
    """the 8 lists of `f32` behind an 8-point centroid graph: a SPANN whose every call scans all 5 000 points"""
    from muopdb_amd.index import Spann
    files, _, _ = H.build_spann_files(oracle, f32["v"], f32["docs"], L_F32, centroids=f32["cent"], max_neighbors=4, max_layers=2,
                                      ef_construction=20)
    sp = Spann(ctx, files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"])
    osp = oracle.Spann(files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"])
    yield sp, osp
    sp.close()


# nsplit * k * 8 + k * 28 + 16 <= 48 KB (mdb_ivf.hip:560-561): the largest k of the fused merge + remap launch, and one past it
@pytest.mark.parametrize("nsplit,k", [(2, 1116), (2, 1117), (4, 818), (4, 819), (8, 534), (8, 535)])
def test_spann_device_call_fused_merge_remap_threshold(ctx, oracle, f32, spann8, nsplit, k):
    """a device-memory SPANN call merges the splits' rows and remaps them in one launch (merge_rows_remap_kernel) while they fit
    48 KB of LDS, and in two (merge_sorted_rows + remap_kernel) from one k further on"""
    pytest.importorskip("torch")
    from muopdb_amd.index import SearchParams
    sp, osp = spann8
    q = f32["q"]
    p = SearchParams(k, 16).with_num_explored_centroids(L_F32).with_centroid_distance_ratio(1e9)
    want = osp.search(q, oracle.SearchParams(k, 16, num_explored_centroids=L_F32, centroid_distance_ratio=1e9))
    assert np.all(want.counts == k)
    with options(ctx, MDB_SCAN_F32_NSPLIT=nsplit):
        got = spann_search_device(ctx, sp, q, p)
        assert_result_rows(got, want, len(q))
        assert np.all(got.found == 1)
        assert_result_rows(sp.search(q, p), want, len(q))


# =================================================================================== 3. IVF-PQ
def _pq_world(ctx, oracle, d, sub, n, nlists, seed):
    from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
    v = H.sift_like(n, d, n_clusters=12, seed=seed)
    cent = H.kmeans(v, nlists, iters=3, seed=seed + 1)
    cb = H.train_pq_codebook(v[:1200], sub, 8, iters=1, seed=seed)
    codes = oracle.ProductQuantizer(d, sub, 8, cb).quantize(v)
    index, vec, pls = H.build_ivf_files(v, doc_ids_for(n, 7), cent, quantize=lambda x: codes)
    w = dict(v=v, q=near(v, 4, seed + 2, 3.0), P=nlists, d=d)
    for name, m in (("l2", 0), ("dot", 1)):
        w["o_" + name] = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_PQ, m, sub, 8, cb))
        w["g_" + name] = BlockBasedIvf(ctx, index, vec, ProductQuantizer(d, sub, 8, cb, m))
    return w


@pytest.fixture(scope="module")
def pq128(ctx, oracle):
    """d = 128, subvectors of 8, 8 bits: a 128 KB codebook (16 x 256 x 8 floats); 3 000 points in 4 lists, all probed"""
    w = _pq_world(ctx, oracle, 128, 8, 3000, 4, seed=51)
    yield w
    w["g_l2"].close()
    w["g_dot"].close()


@pytest.fixture(scope="module")
def pq64(ctx, oracle):
    """d = 64, subvectors of 8, 8 bits: a 64 KB codebook, which leaves the fast path room for every k"""
    w = _pq_world(ctx, oracle, 64, 8, 3000, 4, seed=61)
    yield w
    w["g_l2"].close()
    w["g_dot"].close()


# mdb_ivf.hip:436-442: pq2_lds = align16(cap_for<1024>(k) * 8 + 24) + 4 160 + 512 + 131 072 <= 163 584 holds for cap 2 048 (k <= 1 024) only,
# and with the bound table (+ 8 192) too; :471-473: lds_lut = align16(cap_for<256>(k) * 8 + 24) + 131 072 <= 153 600 for cap 2 048 (k <= 1 792)
@pytest.mark.parametrize("k", [1024,     # ivf_scan_pq2_kernel (L2: with its bound filter)
                               1025,     # ivf_scan_pq_kernel<M, LUT = true>
                               1792,     # the last k with the table
                               1793,     # ivf_scan_pq_kernel<M, LUT = false>
                               2048])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ivf_pq_128k_codebook_scan_forms_fall_off_with_k(ctx, pq128, metric, k):
    g, o, q, P = pq128["g_" + metric], pq128["o_" + metric], pq128["q"], pq128["P"]
    with options(ctx, MDB_PQ_NO_FUSED=1):
        got = g.search(q, k, P)
        assert_result_rows(got, o.search(q, k, num_probes=P), len(q))
        assert np.all(got.counts == k)


@pytest.mark.parametrize("k", [64, 65, 1024, 1025, 2048])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ivf_pq_64k_codebook_stays_on_the_fast_path(ctx, pq64, metric, k):
    """ivf_scan_pq2_kernel at every step of cap_for<1024>; MDB_PQ_BLOCKS = 16 per query: 16 splits (mdb_ivf.hip:447-448) — at
    k = 2 048 that is 32 768 keys per query for merge_keys_kernel<1024>; = 1: one block per query writes the rows in place"""
    g, o, q, P = pq64["g_" + metric], pq64["o_" + metric], pq64["q"], pq64["P"]
    want = o.search(q, k, num_probes=P)
    for blocks in (16 * len(q), 1):
        with options(ctx, MDB_PQ_NO_FUSED=1, MDB_PQ_NO_TWO_PHASE=1, MDB_PQ_BLOCKS=blocks):
            assert_result_rows(g.search(q, k, P), want, len(q))


@pytest.mark.parametrize("world", ["pq128", "pq64"])
def test_ivf_pq_fused_step_and_two_phase_scan_stop_at_k_64(ctx, request, world):
    """ivf_pq_fused_kernel (IvfSet::fused_ok: k <= 64, mdb_ivf.hip:580) and the two-phase scan (k <= 64, :479) on a batch each
    takes at k = 64, and the one-phase scan they hand k = 65 to"""
    w = request.getfixturevalue(world)
    g, o, q, P = w["g_l2"], w["o_l2"], w["q"], w["P"]
    for k in (64, 65):
        want = o.search(q, k, num_probes=P)
        assert_result_rows(g.search(q, k, P), want, len(q))                                   # the fused step (small batch, defaults)
        with options(ctx, MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1):                         # ivf_scan_pq3_kernel + ivf_pq3_refine_kernel
            assert_result_rows(g.search(q, k, P), want, len(q))


# =================================================================================== 4. coarse search
N_CENT, D_CENT = 2100, 16


@pytest.fixture(scope="module")
def coarse(ctx, oracle):
    """2 100 centroids of d = 16 with two points each"""
    from muopdb_amd.index import BlockBasedIvf
    rng = np.random.default_rng(71)
    cent = (rng.standard_normal((N_CENT, D_CENT)) * 10).astype(np.float32)
    v = (np.repeat(cent, 2, 0) + rng.normal(0, 0.5, (2 * N_CENT, D_CENT))).astype(np.float32)
    docs = doc_ids_for(len(v), 11)
    index, vec, pls = H.build_ivf_files(v, docs, cent)
    w = dict(cent=cent, v=v, q=near(v, 6, 72, 1.0), g=BlockBasedIvf(ctx, index, vec), o=oracle.BlockBasedIvf(index, vec))
    yield w
    w["g"].close()


def test_coarse_search_at_the_probe_limit(ctx, coarse):
    g, o, q = coarse["g"], coarse["o"], coarse["q"]
    for P in (64, 65, MAX_K):
        assert np.array_equal(g.find_nearest_centroids(q, P), o.find_nearest_centroids(q, P)), P
    # num_probes = 2 049 <= num_clusters: the selection is refused (flat_topk_keys, mdb_flat.hip:704), in find_nearest_centroids and
    # in a search that selects its probes
    refused(ctx, lambda: g.find_nearest_centroids(q, MAX_K + 1), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    assert np.array_equal(g.find_nearest_centroids(q, MAX_K), o.find_nearest_centroids(q, MAX_K))
    refused(ctx, lambda: g.search(q, 10, MAX_K + 1), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    assert_result_rows(g.search(q, 10, MAX_K), o.search(q, 10, num_probes=MAX_K), len(q))
    refused(ctx, lambda: g.find_nearest_centroids(q, N_CENT + 1), OUT_OF_RANGE, "num_probes=2101 out of range")


def test_search_with_explicit_probe_lists_of_2048_columns_and_more(ctx, coarse):
    """explicit probes are not selected, so their number has no limit: the scans walk them in chunks (TileMap, mdb_ivf_scan.hip.h)"""
    g, o, q = coarse["g"], coarse["o"], coarse["q"]
    rng = np.random.default_rng(73)
    for cols in (MAX_K, N_CENT, 2 * N_CENT):
        probes = np.stack([np.resize(rng.permutation(N_CENT), cols) for _ in range(len(q))]).astype(np.uint32)
        for k in (10, MAX_K):
            got = g.search_with_centroids_and_remap(q, probes, k)
            assert_result_rows(got, o.search(q, k, probes=probes), len(q))
            assert_padding(got, len(q), k)


def test_coarse_keys_and_their_merge_at_the_probe_limit(ctx, coarse):
    from muopdb_amd.distributed import coarse_range
    g, o, q = coarse["g"], coarse["o"], coarse["q"]
    want = o.find_nearest_centroids(q, MAX_K)
    for world in (1, 2, 8):
        rows = [g.coarse_keys(q, MAX_K, *coarse_range(N_CENT, r, world)) for r in range(world)]
        assert np.array_equal(g.merge_coarse_keys(np.stack(rows, axis=1), MAX_K), want), world
    refused(ctx, lambda: g.coarse_keys(q, MAX_K + 1, 0, N_CENT), OUT_OF_RANGE, "coarse_keys: num_probes=2049")
    keys = np.zeros((len(q), 1, MAX_K + 1), np.uint64)
    refused(ctx, lambda: g.merge_coarse_keys(keys, MAX_K + 1), UNSUPPORTED, "num_probes=2049 exceeds MDB_MAX_K=2048")
    rows = [g.coarse_keys(q, MAX_K, 0, N_CENT)]
    assert np.array_equal(g.merge_coarse_keys(np.stack(rows, axis=1), MAX_K), want)


def test_ivf_assign_at_the_cluster_limit(ctx, oracle, coarse):
    from muopdb_amd.index import ivf_assign
    cent, v = coarse["cent"], coarse["v"][:48]
    ids, cnt = ivf_assign(ctx, cent, v, MAX_K, 1e9)
    oids, ocnt = oracle.ivf_assign(cent, v, MAX_K, 1e9)
    assert np.array_equal(cnt, ocnt) and np.array_equal(ids, oids) and int(cnt.max()) == MAX_K
    refused(ctx, lambda: ivf_assign(ctx, cent, v, MAX_K + 1, 1e9), UNSUPPORTED, "max_clusters_per_vector=2049 exceeds 2048")
    ids, cnt = ivf_assign(ctx, cent, v, 3, 0.1)
    oids, ocnt = oracle.ivf_assign(cent, v, 3, 0.1)
    assert np.array_equal(cnt, ocnt) and np.array_equal(ids, oids)


# =================================================================================== 5. HNSW
D_HNSW = 16


def _hnsw_world(ctx, oracle, n, metric, seed, M=8, layers=3):
    from muopdb_amd.index import BlockBasedHnsw, NoQuantizer
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 8, (n, D_HNSW)).astype(np.float32)         # integer rows: equal distances are plentiful
    v[n // 2] = v[3]
    v[n // 3] = v[3]
    docs = [11 * i + 5 + ((i % 2) << 77) for i in range(n)]
    hidx, hvec = H.build_hnsw_files(oracle, v, docs, max_neighbors=M, max_layers=layers, ef_construction=40, seed=seed, metric=metric)
    q = (v[rng.integers(0, n, 6)] + rng.integers(-1, 2, (6, D_HNSW))).astype(np.float32)
    q[0] = v[3]
    return dict(g=BlockBasedHnsw(ctx, hidx, hvec, D_HNSW, NoQuantizer(D_HNSW, metric)),
                o=oracle.BlockBasedHnsw(hidx, hvec, D_HNSW, oracle.Quant(oracle.QUANT_NONE, metric)), q=q, v=v, n=n)


@pytest.fixture(scope="module", params=[0, 1], ids=["l2", "dot"])
def hnsw6000(request, ctx, oracle):
    w = _hnsw_world(ctx, oracle, 6000, request.param, seed=81 + request.param)
    yield w
    w["g"].close()


# mdb_hnsw.hip:1749-1752: ef_cap = ceil64(ef), cand_cap = the power of two >= ef_cap + 192 (at least 1 024): 832 | 833, 1 856 | 1 857 and
# 3 904 | 3 905 are its steps; 449 is the first ef past the wide beam (:1816); 6 000 points > ef: never the closure kernel (:1772)
@pytest.mark.parametrize("ef", [449, 832, 833, 1856, 1857, 2048, 3904, 3905, 4096])
def test_hnsw_general_kernel_over_the_ef_range(ctx, hnsw6000, ef):
    g, o, q = hnsw6000["g"], hnsw6000["o"], hnsw6000["q"]
    for k in (1, min(ef, MAX_K)):           # k = ef, or MDB_MAX_K from ef = 2 048 on
        hnsw_parity(ctx, g, o, q, k, ef)


def test_hnsw_k_larger_than_ef(ctx, hnsw6000):
    g, o, q = hnsw6000["g"], hnsw6000["o"], hnsw6000["q"]
    hnsw_parity(ctx, g, o, q, MAX_K, 100)
    got = g.ann_search(q, MAX_K, 100)
    assert np.all(got.counts <= 100)
    assert_padding(got, len(q), MAX_K)
    hnsw_parity(ctx, g, o, q, MAX_K, 600)


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "dot"])
@pytest.mark.parametrize("n", [4096, 4097])
def test_hnsw_closure_boundary_at_ef_4096(ctx, oracle, n, metric):
    """4 096 points at ef = 4 096: hnsw_closure_kernel at its largest working set (n <= ef and n <= 4 096, mdb_hnsw.hip:1772);
    4 097 points: the general kernel"""
    w = _hnsw_world(ctx, oracle, n, metric, seed=91 + n % 7)
    for k in (1, 10, MAX_K):
        hnsw_parity(ctx, w["g"], w["o"], w["q"], k, MAX_EF)
    w["g"].close()


def test_hnsw_refusals_leave_the_handle_usable(ctx, hnsw6000):
    """ef = 4 097 and k = 2 049: MDB_ERR_UNSUPPORTED from the synchronous call, from submit (nothing is left pending) and from a
    device-memory call (nothing is deferred to mdb_sync); rows and traversal counters before and after are the oracle's"""
    torch = pytest.importorskip("torch")
    g, o, q = hnsw6000["g"], hnsw6000["o"], hnsw6000["q"]
    hnsw_parity(ctx, g, o, q, 10, 600)
    refused(ctx, lambda: g.ann_search(q, 10, MAX_EF + 1), UNSUPPORTED, "ef=4097 exceeds 4096")
    hnsw_parity(ctx, g, o, q, 10, 600)
    refused(ctx, lambda: g.ann_search(q, MAX_K + 1, 600), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    hnsw_parity(ctx, g, o, q, 10, 600)
    for k, ef, text in ((MAX_K + 1, 600, "k=2049 exceeds MDB_MAX_K=2048"), (10, MAX_EF + 1, "ef=4097 exceeds 4096")):
        refused(ctx, lambda: g.ann_search_submit(q, k, ef), UNSUPPORTED, text)
        assert ctx.lib.mdb_wait(ctx.h) == 0                                       # the refused submit left nothing pending
        pend = g.ann_search_submit(q, 10, 600)
        assert_result_rows(pend.wait(), o.ann_search(q, 10, 600), len(q))
        qd = torch.from_numpy(q).to(torch.device("cuda", torch.cuda.current_device()))
        ids, sc, cn, _ = device_rows(torch, len(q), k)
        torch.cuda.synchronize()
        refused(ctx, lambda: g.ann_search_device(qd.data_ptr(), len(q), k, ef, ids.data_ptr(), sc.data_ptr(), cn.data_ptr()),
                UNSUPPORTED, text)
        ctx.sync()                                                                # decided on the host: no deferred status
        ids, sc, cn, _ = device_rows(torch, len(q), 10)
        torch.cuda.synchronize()   # torch's fills are not ordered with the context's stream
        g.ann_search_device(qd.data_ptr(), len(q), 10, 600, ids.data_ptr(), sc.data_ptr(), cn.data_ptr())
        ctx.sync()
        assert_result_rows(rows_to_result(len(q), 10, ids, sc, cn), o.ann_search(q, 10, 600), len(q))
        hnsw_parity(ctx, g, o, q, 10, 600)


def test_hnsw_over_pq_codes_at_ef_2048(ctx, oracle):
    from muopdb_amd.index import BlockBasedHnsw, ProductQuantizer
    n, d, sub, bits = 3000, 32, 8, 6
    v = H.sift_like(n, d, n_clusters=25, seed=33)
    cb = H.train_pq_codebook(v[:1000], sub, bits, iters=2)
    codes = oracle.ProductQuantizer(d, sub, bits, cb).quantize(v)
    b = oracle.HnswBuilder(d, 8, 3, 40, 0, 3)
    b.insert(v)
    layers, eps = b.layers(), b.entry_points()
    if len(layers) > 1:
        top = layers[-1]
        layers[-1] = {eps[0]: top[eps[0]], **{p: e for p, e in top.items() if p != eps[0]}}
    hidx, hvec = F.write_hnsw_index(layers, [11 * i + 5 for i in range(n)], d // sub), F.write_vector_file(codes)
    g = BlockBasedHnsw(ctx, hidx, hvec, d, ProductQuantizer(d, sub, bits, cb))
    o = oracle.BlockBasedHnsw(hidx, hvec, d, oracle.Quant(oracle.QUANT_PQ, 0, sub, bits, cb))
    q = near(v, 5, 34, 5.0)
    for k in (1, MAX_K):
        hnsw_parity(ctx, g, o, q, k, 2048)
    g.close()


# =================================================================================== 6. SPANN and multi-user SPANN
N_SPANN = 8000
BIG_USER = (1 << 70) + 5


@pytest.fixture(scope="module")
def spann(ctx, oracle, coarse):
    """8 000 points behind the 2 100 centroids of `coarse`, alone (Spann) and as the large one of three users (MultiSpannIndex)"""
    from muopdb_amd.index import MultiSpannIndex, Spann
    rng = np.random.default_rng(101)
    cent = coarse["cent"]
    v = (cent[rng.integers(0, N_CENT, N_SPANN)] + rng.normal(0, 0.5, (N_SPANN, D_CENT))).astype(np.float32)
    docs = doc_ids_for(N_SPANN, 13)
    files, _, _ = H.build_spann_files(oracle, v, docs, N_CENT, centroids=cent, max_neighbors=8, max_layers=3, ef_construction=40)
    small = [H.build_spann_files(oracle, v[:200 + 50 * i] + i, docs[:200 + 50 * i], 5, seed=i, max_neighbors=4, max_layers=2,
                                 ef_construction=20)[0] for i in (1, 2)]
    cat = F.concat_multi_spann({3: small[0], BIG_USER: files, 9: small[1]})
    margs = (cat["user_table"], D_CENT, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    sargs = (files["hnsw_index"], files["hnsw_vectors"], files["ivf_index"], files["ivf_vectors"])
    w = dict(sp=Spann(ctx, *sargs), osp=oracle.Spann(*sargs), ms=MultiSpannIndex(ctx, *margs), oms=oracle.MultiSpannIndex(*margs),
             margs=margs, q=near(v, 4, 102, 1.0), users=[BIG_USER, 3, BIG_USER, 9], v=v)
    yield w
    w["sp"].close()
    w["ms"].close()


def _params(oracle, k, ef, nexp, ratio=1e9):
    from muopdb_amd.index import SearchParams
    return (SearchParams(k, ef).with_num_explored_centroids(nexp).with_centroid_distance_ratio(ratio),
            oracle.SearchParams(k, ef, num_explored_centroids=nexp, centroid_distance_ratio=ratio))


# ef_construction >= 2 100 points of the centroid graph: hnsw_closure_kernel (mdb_hnsw.hip:1772); 600: hnsw_search_kernel, which
# returns at most ef centroids
@pytest.mark.parametrize("ef", [4096, 600])
def test_spann_at_2048_explored_centroids_and_top_k_2048(ctx, oracle, spann, ef):
    pytest.importorskip("torch")
    from muopdb_amd.index import allow_bitmap
    sp, osp, q = spann["sp"], spann["osp"], spann["q"]
    p, op = _params(oracle, MAX_K, ef, MAX_K)
    want = osp.search(q, op)
    assert np.all(want.counts == MAX_K) or ef < MAX_K
    got = sp.search(q, p)                                                            # host memory
    assert_result_rows(got, want, len(q))
    assert_padding(got, len(q), MAX_K)
    assert_result_rows(spann_search_device(ctx, sp, q, p), want, len(q))             # device memory
    bm = allow_bitmap(np.arange(0, N_SPANN, 5), N_SPANN)                             # a filter that leaves 1 600 points
    with oracle.planner_filter(bm):
        fwant = osp.search(q, op)
    fgot = sp.search(q, p, planner=bm)
    assert_result_rows(fgot, fwant, len(q))
    assert_padding(fgot, len(q), MAX_K)
    merged = sp.merge_shards([sp.search_shard(q, p)], len(q), MAX_K)                 # its own points block through the exact merge
    assert_result_rows(merged, want, len(q))
    assert np.all(merged.found == 1)


@pytest.mark.parametrize("ef", [4096, 600])
def test_multi_user_spann_at_2048_explored_centroids_and_top_k_2048(ctx, oracle, spann, ef):
    pytest.importorskip("torch")
    from muopdb_amd.index import MultiSpannIndex, allow_bitmap
    ms, oms, q, users = spann["ms"], spann["oms"], spann["q"], spann["users"]
    p, op = _params(oracle, MAX_K, ef, MAX_K)
    want = oms.search_for_user(users, q, op)
    got = ms.search_for_user(users, q, p)
    assert_result_rows(got, want, len(q))
    assert got.found.tolist() == want.found.tolist() == [1, 1, 1, 1]
    assert_padding(got, len(q), MAX_K)
    assert_result_rows(spann_search_device(ctx, ms, q, p, users), want, len(q))
    bms = np.stack([allow_bitmap(np.arange(i % 3, N_SPANN, 3 + i), N_SPANN) for i in range(len(q))])   # over each user's own point ids
    with oracle.planner_filter(bms):
        fwant = oms.search_for_user(users, q, op)
    fgot = ms.search_for_user(users, q, p, planner=bms)
    assert_result_rows(fgot, fwant, len(q))
    assert_padding(fgot, len(q), MAX_K)
    shards = [MultiSpannIndex(ctx, *spann["margs"], None, r, 2) for r in range(2)]   # two list shards on one GPU
    merged = shards[0].merge_shards(users, [s.search_shard(users, q, p) for s in shards], len(q), MAX_K)
    assert_result_rows(merged, want, len(q))
    for s in shards:
        s.close()


def test_spann_refusals_leave_the_handles_usable(ctx, oracle, spann):
    pytest.importorskip("torch")
    sp, osp, ms, oms, q, users = spann["sp"], spann["osp"], spann["ms"], spann["oms"], spann["q"], spann["users"]
    text = "top_k / num_explored_centroids exceed MDB_MAX_K=2048"
    ok, ook = _params(oracle, 10, 100, 8)
    want, mwant = osp.search(q, ook), oms.search_for_user(users, q, ook)
    for k, nexp in ((MAX_K + 1, 8), (10, MAX_K + 1)):
        bad, _ = _params(oracle, k, 100, nexp)
        refused(ctx, lambda: sp.search(q, bad), UNSUPPORTED, text)
        assert_result_rows(sp.search(q, ok), want, len(q))
        refused(ctx, lambda: ms.search_for_user(users, q, bad), UNSUPPORTED, text)
        assert_result_rows(ms.search_for_user(users, q, ok), mwant, len(q))
        refused(ctx, lambda: sp.search_submit(q, bad), UNSUPPORTED, text)             # through submit: nothing left pending
        assert ctx.lib.mdb_wait(ctx.h) == 0
        assert_result_rows(sp.search_submit(q, ok).wait(), want, len(q))
        refused(ctx, lambda: spann_search_device(ctx, ms, q, bad, users), UNSUPPORTED, text)   # device memory: refused at once,
        ctx.sync()                                                                             # nothing deferred to mdb_sync
        assert_result_rows(spann_search_device(ctx, ms, q, ok, users), mwant, len(q))
        refused(ctx, lambda: sp.search_shard(q, bad), UNSUPPORTED, text)
        assert_result_rows(sp.merge_shards([sp.search_shard(q, ok)], len(q), 10), want, len(q))
    bad_ef, _ = _params(oracle, 10, MAX_EF + 1, 8)                                    # ef_construction is the centroid graph's ef
    refused(ctx, lambda: sp.search(q, bad_ef), UNSUPPORTED, "ef=4097 exceeds 4096")
    assert_result_rows(sp.search(q, ok), want, len(q))
    refused(ctx, lambda: ms.search_for_user(users, q, bad_ef), UNSUPPORTED, "ef=4097 exceeds 4096")
    assert_result_rows(ms.search_for_user(users, q, ok), mwant, len(q))
    blocks = [np.zeros(int(ctx.lib.mdb_points_block_bytes(C.c_size_t(len(q)), C.c_size_t(MAX_K + 1))), np.uint8)]
    refused(ctx, lambda: sp.merge_shards(blocks, len(q), MAX_K + 1), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    refused(ctx, lambda: ms.merge_shards(users, blocks, len(q), MAX_K + 1), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    assert_result_rows(ms.merge_shards(users, [ms.search_shard(users, q, ok)], len(q), 10), mwant, len(q))


# =================================================================================== 7. shard merges
def merge_points_capacity(world):
    """largest k of mdb_*_merge_shards: world * k * 8 + k * 20 + (world + 1) * 4 + 16 <= 150 KB (mdb_ivf.hip:750-751), and k <= MDB_MAX_K"""
    return min(MAX_K, (150 * 1024 - (world + 1) * 4 - 16) // (world * 8 + 20))


def merge_shards_capacity(world):
    """largest k of mdb_merge_shards[_packed]: world * k * 20 + (world + 1) * 4 + 16 <= 150 KB (mdb_spann.hip:314-315)"""
    return (150 * 1024 - (world + 1) * 4 - 16) // (world * 20)


def test_capacity_formulas():
    assert [merge_points_capacity(w) for w in (2, 4, 8)] == [2048, 2048, 1827]
    assert [merge_shards_capacity(w) for w in (2, 4, 8)] == [3839, 1919, 959]


@pytest.mark.parametrize("world", [2, 4, 8])
def test_ivf_merge_shards_at_its_capacity(ctx, f32, world):
    pytest.importorskip("torch")
    from muopdb_amd.index import BlockBasedIvf
    q, g, o = f32["q"], f32["g_l2"], f32["o_l2"]
    k = merge_points_capacity(world)
    probes = g.find_nearest_centroids(q, L_F32)
    shards = [BlockBasedIvf(ctx, f32["index"], f32["vec"], shard_rank=r, shard_world=world) for r in range(world)]
    merged = shards[0].merge_shards([s.search_shard(q, k, probes=probes) for s in shards], len(q), k)
    want = o.search(q, k, num_probes=L_F32)
    assert_result_rows(merged, want, len(q))
    assert_result_rows(g.search(q, k, L_F32), want, len(q))
    assert np.all(merged.counts == k)
    over = k + 1    # one past: the capacity message where the LDS formula decides, MDB_MAX_K's where k = 2 049 does
    blocks = [np.zeros(int(ctx.lib.mdb_points_block_bytes(C.c_size_t(len(q)), C.c_size_t(over))), np.uint8) for _ in range(world)]
    text = "k=2049 exceeds MDB_MAX_K=2048" if over > MAX_K else "world*k=%d rows exceed the on-chip merge capacity" % (world * over)
    refused(ctx, lambda: shards[0].merge_shards(blocks, len(q), over), UNSUPPORTED, text)
    merged = shards[-1].merge_shards([s.search_shard(q, k, probes=probes) for s in shards], len(q), k)
    assert_result_rows(merged, want, len(q))
    for s in shards:
        s.close()


def _merge_rows(ctx, torch, sets, b, k, packed):
    """mdb_merge_shards (three arrays) or mdb_merge_shards_packed (one block per rank) over `sets`: per rank (lo, hi, scores, counts)
    of stride <= k, re-laid at stride k"""
    from muopdb_amd import distributed as D
    world = len(sets)
    dev = torch.device("cuda", torch.cuda.current_device())
    docs = np.full((world, b, k, 2), ALL_ONES, np.uint64)
    sc = np.full((world, b, k), np.inf, np.float32)
    cn = np.zeros((world, b), np.uint32)
    for w, (lo, hi, s, c) in enumerate(sets):
        kk = min(k, lo.shape[1])
        docs[w, :, :kk, 0], docs[w, :, :kk, 1], sc[w, :, :kk] = lo[:, :kk], hi[:, :kk], s[:, :kk]
        cn[w] = np.minimum(c, kk)
    t_docs, t_sc, t_cn = (torch.from_numpy(docs.view(np.int64)).to(dev), torch.from_numpy(sc).to(dev),
                          torch.from_numpy(cn.view(np.int32)).to(dev))
    ids, osc, ocn, _ = device_rows(torch, b, k)
    if packed:
        nb = int(ctx.lib.mdb_shard_block_bytes(C.c_size_t(b), C.c_size_t(k)))
        recv = torch.zeros(world * nb, dtype=torch.uint8, device=dev)
        for w in range(world):
            vi, vs, vc = D.block_views(recv[w * nb:(w + 1) * nb], b, k)
            vi.copy_(t_docs[w]); vs.copy_(t_sc[w]); vc.copy_(t_cn[w])
        torch.cuda.synchronize()
        ctx.check(ctx.lib.mdb_merge_shards_packed(ctx.h, C.c_void_p(recv.data_ptr()), C.c_size_t(world), C.c_size_t(b), C.c_size_t(k),
                                                  C.c_void_p(ids.data_ptr()), C.c_void_p(osc.data_ptr()), C.c_void_p(ocn.data_ptr())))
    else:
        torch.cuda.synchronize()
        ctx.check(ctx.lib.mdb_merge_shards(ctx.h, C.c_void_p(t_docs.data_ptr()), C.c_void_p(t_sc.data_ptr()), C.c_void_p(t_cn.data_ptr()),
                                           C.c_size_t(world), C.c_size_t(b), C.c_size_t(k), C.c_void_p(ids.data_ptr()),
                                           C.c_void_p(osc.data_ptr()), C.c_void_p(ocn.data_ptr())))
    ctx.sync()
    return rows_to_result(b, k, ids, osc, ocn), docs, sc, cn


@pytest.mark.parametrize("packed", [False, True], ids=["arrays", "packed"])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_merge_shards_of_remapped_rows_at_its_capacity(ctx, f32, world, packed):
    """mdb_merge_shards / mdb_merge_shards_packed over the remapped rows of `world` real list shards, at the largest k their LDS
    formula admits (rows longer than MDB_MAX_K are the shards' 2 048 results re-laid at the wider stride), against a plain sort
    by (score, doc id); with every point on one shard and k within the total that is also the oracle's unsharded row"""
    torch = pytest.importorskip("torch")
    from muopdb_amd.index import BlockBasedIvf
    q, o = f32["q"], f32["o_l2"]
    b, k = len(q), merge_shards_capacity(world)
    probes = f32["g_l2"].find_nearest_centroids(q, L_F32)
    sets = []
    for r in range(world):
        s = BlockBasedIvf(ctx, f32["index"], f32["vec"], shard_rank=r, shard_world=world)
        res = s.search_with_centroids_and_remap(q, probes, min(k, MAX_K))
        sets.append((np.array(res.doc_lo), np.array(res.doc_hi), np.array(res.scores), np.array(res.counts)))
        s.close()
    got, docs, sc, cn = _merge_rows(ctx, torch, sets, b, k, packed)
    for i in range(b):
        rows = sorted((float(sc[w, i, j]), (int(docs[w, i, j, 1]) << 64) | int(docs[w, i, j, 0])) for w in range(world)
                      for j in range(int(cn[w, i])))[:k]
        assert int(got.counts[i]) == len(rows), i
        assert got.doc_ids(i) == [d for _, d in rows], i
        assert np.array_equal(np.asarray(got.scores[i, :len(rows)], np.float32), np.asarray([s for s, _ in rows], np.float32)), i
    if k <= MAX_K:
        # every shard returned its k best, so the merge holds the k best overall: the oracle's row up to ties in (score, doc id) order,
        # which the oracle breaks by point id BEFORE the remap — compare the score rows
        want = o.search(q, k, num_probes=L_F32)
        for i in range(b):
            assert np.array_equal(np.asarray(got.scores[i, :k], np.float32).view(np.uint32), np.asarray(want.scores[i, :k], np.float32).view(np.uint32))
    text = "world*k=%d rows exceed the on-chip merge capacity" % (world * (k + 1))
    refused(ctx, lambda: _merge_rows(ctx, torch, sets, b, k + 1, packed), UNSUPPORTED, text)
    again, _, _, _ = _merge_rows(ctx, torch, sets, b, k, packed)
    for i in range(b):
        assert again.doc_ids(i) == got.doc_ids(i)


# =================================================================================== 8. load-time and build limits
def _star_graph(n, degree):
    """one layer: point 0 has `degree` neighbours, every other point its two ring neighbours and 0"""
    layer = {0: list(range(1, degree + 1))}
    for p in range(1, n):
        layer[p] = [0, p - 1 if p > 1 else n - 1, p + 1 if p + 1 < n else 1]
    return [layer]


def test_hnsw_node_degree_256_loads_and_257_is_refused(ctx, oracle):
    """HNSW_MAX_STRIDE = 256 (mdb_hnsw.hip:32, :1503): a hand-written graph whose point 0 has exactly 256 neighbours is searched by
    every traversal kernel (rows of four 64-edge chunks) equal to the oracle; 257 neighbours are refused at load"""
    from muopdb_amd.index import BlockBasedHnsw
    n = 700
    rng = np.random.default_rng(111)
    v = rng.integers(0, 16, (n, D_HNSW)).astype(np.float32)
    docs = list(range(1000, 1000 + n))
    vec = F.write_vector_file(v)
    hidx = F.write_hnsw_index(_star_graph(n, 256), docs, D_HNSW)
    g, o = BlockBasedHnsw(ctx, hidx, vec, D_HNSW), oracle.BlockBasedHnsw(hidx, vec, D_HNSW)
    q = (v[rng.integers(0, n, 6)] + rng.integers(-1, 2, (6, D_HNSW))).astype(np.float32)
    for k, ef in ((10, 50), (10, 256), (10, 400), (20, 600), (700, 700), (MAX_K, MAX_EF)):   # beam, wide beam, general, closure
        hnsw_parity(ctx, g, o, q, k, ef)
    bad = F.write_hnsw_index(_star_graph(n, 257), docs, D_HNSW)
    refused(ctx, lambda: BlockBasedHnsw(ctx, bad, vec, D_HNSW), UNSUPPORTED, "node degree 257 exceeds 256")
    hnsw_parity(ctx, g, o, q, 10, 600)
    g.close()


def _tower(n, num_layers):
    """layer 0: a ring over n points; every upper layer: points 0 and 1"""
    ring = {p: [(p + 1) % n, (p - 1) % n] for p in range(n)}
    return [ring] + [{0: [1], 1: [0]} for _ in range(num_layers - 1)]


def test_hnsw_255_layers_load_and_256_are_refused(ctx, oracle):
    """mdb_hnsw.hip:1412: a 255-layer file (two points in each upper layer) loads and searches equal to the oracle; 256 layers are
    refused"""
    from muopdb_amd.index import BlockBasedHnsw
    n = 40
    rng = np.random.default_rng(112)
    v = rng.integers(0, 16, (n, D_HNSW)).astype(np.float32)
    docs = list(range(n))
    vec = F.write_vector_file(v)
    hidx = F.write_hnsw_index(_tower(n, 255), docs, D_HNSW)
    g, o = BlockBasedHnsw(ctx, hidx, vec, D_HNSW), oracle.BlockBasedHnsw(hidx, vec, D_HNSW)
    assert o.num_layers == 255
    q = v[:5] + 0.25
    for k, ef in ((5, 8), (5, 30), (40, 64), (10, 600)):
        hnsw_parity(ctx, g, o, q, k, ef)
    bad = F.write_hnsw_index(_tower(n, 256), docs, D_HNSW)
    refused(ctx, lambda: BlockBasedHnsw(ctx, bad, vec, D_HNSW), UNSUPPORTED, "more than 255 HNSW layers")
    hnsw_parity(ctx, g, o, q, 5, 30)
    g.close()


def test_select_neighbors_at_max_neighbors_64(ctx, oracle):
    """mdb_hnsw_select_neighbors keeps up to 64 neighbours (one lane each, mdb_hnsw_build.hip:57): parity with the heuristic of
    hnsw/builder.rs:339-375 restated with the oracle's distance; 65 and 0 are refused"""
    from muopdb_amd import build as B
    rng = np.random.default_rng(113)
    n, d, M, W, R = 400, 96, 64, 200, 6
    x = (rng.standard_normal((n, d)) * 4).astype(np.float32)
    x[:R] = rng.normal(0, 0.01, (R, d))                                              # the rows' own points: near the origin
    x[100:196] = np.eye(d) * (10 + 0.05 * np.arange(d))[:, None] + rng.normal(0, 0.01, (d, d))   # 96 points on the axes: each further from
    x[300:360] = x[300] + rng.normal(0, 0.1, (60, d))                                # a tight cluster: its first point shadows the rest
    cand = np.full((R, W), 0xFFFFFFFF, np.uint32)                                    # the others than from the origin, so all are kept
    dist = np.full((R, W), np.inf, np.float32)
    for r, axes in enumerate((96, 10, 64, 0, 63, 65)):
        c = np.concatenate([100 + rng.choice(96, axes, replace=False), 200 + rng.choice(100, int(rng.integers(60, 100)), replace=False)])
        if axes == 0:
            c = np.arange(300, 360)
        dd = np.array([oracle.l2(x[r], x[j]) for j in c], np.float32)
        order = np.lexsort((-c.astype(np.int64), dd))
        cand[r, :len(c)], dist[r, :len(c)] = c[order], dd[order]

    ids, ds, cnt = B.select_neighbors(ctx, x, cand, dist, M)
    for r in range(R):
        kept = []
        for j in range(W):
            e = int(cand[r, j])
            if e == 0xFFFFFFFF or len(kept) == M:
                break
            if all(not (np.float32(oracle.l2(x[e], x[k_])) < dist[r, j]) for k_, _ in kept):
                kept.append((e, dist[r, j]))
        assert int(cnt[r]) == len(kept) and ids[r, :len(kept)].tolist() == [e for e, _ in kept], r
        assert np.array_equal(ds[r, :len(kept)].view(np.uint32), np.array([v_ for _, v_ in kept], np.float32).view(np.uint32))
    assert cnt[0] == cnt[2] == cnt[5] == M and cnt[4] >= 63 and cnt[3] < 8          # all 64 lanes in use, and rows that stop short
    text = "max_neighbors must be 1..64"
    for bad in (65, 0):
        refused(ctx, lambda: B.select_neighbors(ctx, x, cand, dist, bad), UNSUPPORTED, text)
        ids2, ds2, cnt2 = B.select_neighbors(ctx, x, cand, dist, M)
        assert np.array_equal(ids2, ids) and np.array_equal(ds2.view(np.uint32), ds.view(np.uint32)) and np.array_equal(cnt2, cnt)


def test_pq_num_bits_8_loads_and_9_is_refused(ctx, oracle, pq64):
    from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
    rng = np.random.default_rng(114)
    d, sub, n = 16, 8, 64
    v = rng.standard_normal((n, d)).astype(np.float32)
    cent = v[:2].copy()
    index, vec, _ = H.build_ivf_files(v, list(range(n)), cent, quantize=lambda x: np.zeros((n, d // sub), np.uint8))
    cb9 = rng.standard_normal((d // sub) * 512 * sub).astype(np.float32)
    refused(ctx, lambda: BlockBasedIvf(ctx, index, vec, ProductQuantizer(d, sub, 9, cb9)), UNSUPPORTED, "num_bits must be 1..8")
    g, o, q, P = pq64["g_l2"], pq64["o_l2"], pq64["q"], pq64["P"]                 # an 8-bit index on the same context still serves
    assert_result_rows(g.search(q, 10, P), o.search(q, 10, num_probes=P), len(q))


# =================================================================================== 9. refusals on the IVF paths
def test_ivf_refusals_leave_the_handle_usable(ctx, f32):
    """k = 2 049 on every IVF entry point — synchronous, filtered, submit, the shard block — then the oracle's rows again"""
    from muopdb_amd.index import allow_bitmap
    g, o, q = f32["g_l2"], f32["o_l2"], f32["q"]
    text = "k=2049 exceeds MDB_MAX_K=2048"
    want = o.search(q, MAX_K, num_probes=L_F32)
    bm = allow_bitmap(np.arange(N_F32), N_F32)
    for call in (lambda: g.search(q, MAX_K + 1, L_F32),
                 lambda: g.search(q, MAX_K + 1, L_F32, planner=bm),
                 lambda: g.search_points(q, MAX_K + 1, L_F32),
                 lambda: g.search_shard(q, MAX_K + 1, L_F32),
                 lambda: g.search_submit(q, MAX_K + 1, L_F32)):
        refused(ctx, call, UNSUPPORTED, text)
        assert ctx.lib.mdb_wait(ctx.h) == 0
        assert_result_rows(g.search(q, MAX_K, L_F32), want, len(q))
    assert_result_rows(g.search_submit(q, MAX_K, L_F32).wait(), want, len(q))


def test_flat_refusal_leaves_the_handle_usable(ctx, oracle, f32):
    from muopdb_amd.index import FlatIndex
    base, q = f32["v"], f32["q"]
    fi = FlatIndex(ctx, base)
    refused(ctx, lambda: fi.search(q, MAX_K + 1), UNSUPPORTED, "k=2049 exceeds MDB_MAX_K=2048")
    ids, dist, counts = fi.search(q, MAX_K)
    oids, odist = oracle.flat_topk(0, base, q, MAX_K)
    assert np.array_equal(ids, oids) and np.array_equal(dist.view(np.uint32), odist.view(np.uint32)) and np.all(counts == MAX_K)
    fi.close()

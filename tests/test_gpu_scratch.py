"""The per-call scratch arena under the search entries (-m gpu): ONE context serves flat, IVF-PQ, HNSW and multi-user SPANN calls
interleaved at growing and shrinking batch sizes — host and device memory, with and without planner bitmaps, through submit / wait —
so a call's buffers are carved next to each other out of chunks that earlier, different calls sized.  Every result is checked
against the oracle (ids exact, score bits), and the whole sequence run again on the same context must give the same bytes.
"""
import ctypes as C

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H
from tests.test_gpu_parity import assert_result_rows, assert_scores

pytestmark = pytest.mark.gpu

BATCHES = (1, 9, 70, 3, 300, 9)   # growth, then shrink
D, K, P, EF = 32, 10, 6, 48
USERS = (5, 9, 12)


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def world(ctx, oracle):
    """the four tiny indexes on ONE context, their oracle twins and a cache of oracle results"""
    from muopdb_amd.index import (BlockBasedHnsw, BlockBasedIvf, FlatIndex, MultiSpannIndex, ProductQuantizer, allow_bitmap)
    rng = np.random.default_rng(77)
    w = dict(want={})
    w["q"] = (H.sift_like(300, D, n_clusters=20, seed=3) + rng.normal(0, 3, (300, D))).astype(np.float32)
    # flat 4 096 x 32
    w["base"] = H.sift_like(4096, D, n_clusters=20, seed=3)
    w["flat"] = FlatIndex(ctx, w["base"])
    # IVF-PQ 2 048 x 32, 16 lists, m = 8
    n = 2048
    v = H.sift_like(n, D, n_clusters=20, seed=3)
    cent = H.kmeans(v, 16, iters=3, seed=4)
    cb = H.train_pq_codebook(v[:1500], 4, 6, iters=3)
    opq = oracle.ProductQuantizer(D, 4, 6, cb)
    index, vec, _ = H.build_ivf_files(v, [100 + 3 * i for i in range(n)], cent, quantize=opq.quantize)
    w["ivf"] = BlockBasedIvf(ctx, index, vec, ProductQuantizer(D, 4, 6, cb))
    w["oivf"] = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 4, 6, cb))
    w["ivf_bm"] = np.stack([allow_bitmap(np.sort(rng.choice(n, n // 3, replace=False)), n) for _ in range(300)])
    # HNSW 2 000 x 32
    hv = H.sift_like(2000, D, n_clusters=20, seed=3)
    hidx, hvec = H.build_hnsw_files(oracle, hv, list(range(2000)), max_neighbors=8, max_layers=3, ef_construction=40)
    w["hnsw"] = BlockBasedHnsw(ctx, hidx, hvec, D)
    w["ohnsw"] = oracle.BlockBasedHnsw(hidx, hvec, D)
    # three users' SPANN
    per_user = {}
    for j, u in enumerate(USERS):
        uv = H.sift_like(500 + 100 * j, D, n_clusters=20, seed=3 + j)
        per_user[u], _, _ = H.build_spann_files(oracle, uv, [1000 * u + i for i in range(len(uv))], 10, seed=j, max_neighbors=8,
                                                max_layers=3, ef_construction=40)
    cat = F.concat_multi_spann(per_user)
    margs = (cat["user_table"], D, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    w["ms"] = MultiSpannIndex(ctx, *margs)
    w["oms"] = oracle.MultiSpannIndex(*margs)
    w["ms_users"] = [USERS[i % 3] for i in range(300)]
    w["ms_bm"] = allow_bitmap(np.arange(0, 700, 2), 700)   # even user-local point ids, shared by the batch
    yield w
    for name in ("flat", "ivf", "hnsw", "ms"):
        w[name].close()


def _dev_result(torch, ids, sc, cn):
    from muopdb_amd.index import SearchResult
    h = ids.cpu().numpy().view(np.uint64)
    return SearchResult(h.shape[0], h.shape[1], h[:, :, 0], h[:, :, 1], sc.cpu().numpy(), cn.cpu().numpy().view(np.uint32))


def _row_bytes(res, b):
    """a result's defined bytes: counts, and every row up to its count"""
    return b"".join([np.asarray(res.counts[:b], np.uint32).tobytes()] +
                    [np.ascontiguousarray(a[i, :int(res.counts[i])]).tobytes() for i in range(b) for a in (res.doc_lo, res.doc_hi, res.scores)])


def _sequence(ctx, oracle, w):
    """every family at every batch size; returns the outputs' bytes in call order"""
    import torch
    from muopdb_amd import lib as L
    from muopdb_amd.index import SearchParams
    dev = torch.device("cuda", torch.cuda.current_device())
    sp, osp = SearchParams(K, 40).with_num_explored_centroids(4), oracle.SearchParams(K, 40, num_explored_centroids=4)
    spc = sp.to_c()
    out = []

    def want(key, make):
        if key not in w["want"]:
            w["want"][key] = make()
        return w["want"][key]

    def outs(b, ids_shape=None, ids_dtype=torch.int64):
        t = (torch.zeros(ids_shape or (b, K, 2), dtype=ids_dtype, device=dev), torch.zeros((b, K), dtype=torch.float32, device=dev),
             torch.zeros(b, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()   # the fills run on torch's stream, the searches on the context's
        return t

    def rows(res, ores, b):
        assert_result_rows(res, ores, b)
        out.append(_row_bytes(res, b))

    for step, b in enumerate(BATCHES):
        q = w["q"][:b]
        qd = torch.from_numpy(q).to(dev)
        # ---- flat: host, device
        oids, odist = want(("flat", b), lambda: oracle.flat_topk(0, w["base"], q, K))
        ids, dist, cnt = w["flat"].search(q, K)
        assert np.array_equal(ids, oids) and np.all(cnt == K)
        assert_scores(dist, odist)
        out.append(ids.tobytes() + dist.tobytes())
        fi, fd_, fc = outs(b, (b, K), torch.int32)
        w["flat"].search_device(qd.data_ptr(), b, K, fi.data_ptr(), fd_.data_ptr(), fc.data_ptr())
        ctx.sync()
        assert np.array_equal(fi.cpu().numpy().view(np.uint32), oids) and np.all(fc.cpu().numpy() == K)
        assert_scores(fd_.cpu().numpy(), odist)
        out.append(fi.cpu().numpy().tobytes() + fd_.cpu().numpy().tobytes())
        # ---- IVF-PQ: host, host + bitmaps, device, device + bitmaps, submit / wait
        bm = w["ivf_bm"][:b]
        plain = want(("ivf", b), lambda: w["oivf"].search(q, K, num_probes=P))

        def filtered():
            with oracle.planner_filter(bm):
                return w["oivf"].search(q, K, num_probes=P)
        filt = want(("ivf_f", b), filtered)
        rows(w["ivf"].search(q, K, P), plain, b)
        rows(w["ivf"].search(q, K, P, planner=bm), filt, b)
        ids, sc, cn = outs(b)
        ctx.check(ctx.lib.mdb_ivf_search(w["ivf"].h, C.c_void_p(qd.data_ptr()), C.c_size_t(b), None, C.c_size_t(P), C.c_size_t(K),
                                         C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(cn.data_ptr())))
        ctx.sync()
        rows(_dev_result(torch, ids, sc, cn), plain, b)
        bmd = torch.from_numpy(bm.view(np.int32)).to(dev)
        ids, sc, cn = outs(b)
        ctx.check(ctx.lib.mdb_ivf_search_filtered(w["ivf"].h, C.c_void_p(qd.data_ptr()), C.c_size_t(b), None, C.c_size_t(P), C.c_size_t(K),
                                                  C.c_int(L.MEM_DEVICE), C.c_void_p(bmd.data_ptr()), C.c_size_t(b), C.c_size_t(bm.shape[1]),
                                                  C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(cn.data_ptr())))
        ctx.sync()
        rows(_dev_result(torch, ids, sc, cn), filt, b)
        if step % 2 == 0:
            rows(w["ivf"].search_submit(q, K, P, planner=bm).wait(), filt, b)
        # ---- HNSW: host, device, submit / wait
        hw = want(("hnsw", b), lambda: w["ohnsw"].ann_search(q, K, EF))
        rows(w["hnsw"].ann_search(q, K, EF), hw, b)
        ids, sc, cn = outs(b)
        w["hnsw"].ann_search_device(qd.data_ptr(), b, K, EF, ids.data_ptr(), sc.data_ptr(), cn.data_ptr())
        ctx.sync()
        rows(_dev_result(torch, ids, sc, cn), hw, b)
        if step % 2 == 1:
            rows(w["hnsw"].ann_search_submit(q, K, EF).wait(), hw, b)
        # ---- multi-user SPANN: host, host + a shared bitmap, device
        users = w["ms_users"][:b]
        mw = want(("ms", b), lambda: w["oms"].search_for_user(users, q, osp))

        def ms_filtered():
            with oracle.planner_filter(w["ms_bm"]):
                return w["oms"].search_for_user(users, q, osp)
        mf = want(("ms_f", b), ms_filtered)
        got = w["ms"].search_for_user(users, q, sp)
        assert np.all(got.found[:b] == 1)
        rows(got, mw, b)
        rows(w["ms"].search_for_user(users, q, sp, planner=w["ms_bm"]), mf, b)
        ids, sc, cn = outs(b)
        fo = torch.zeros(b, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.mdb_multi_spann_search(w["ms"].h, L.u128_array(users), C.c_void_p(qd.data_ptr()), C.c_size_t(b), C.byref(spc),
                                                 C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                                 C.c_void_p(cn.data_ptr()), C.c_void_p(fo.data_ptr())))
        ctx.sync()
        assert np.all(fo.cpu().numpy() == 1)
        rows(_dev_result(torch, ids, sc, cn), mw, b)
    return out


def test_interleaved_calls_growth_then_shrink_and_again(ctx, oracle, world):
    pytest.importorskip("torch")
    first = _sequence(ctx, oracle, world)
    second = _sequence(ctx, oracle, world)
    assert len(first) == len(second) and all(a == b for a, b in zip(first, second)), "the second pass over the same context differs"


@pytest.fixture(scope="module")
def assign_case(oracle):
    n, d, mc, thr = 65536 + 100, 16, 2, 0.1
    v = H.sift_like(n, d, n_clusters=32, seed=11)
    cent = H.kmeans(v[:4000], 64, iters=3, seed=1)
    return v, cent, mc, thr, oracle.ivf_assign(cent, v, mc, thr)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_ivf_assign_second_pass_of_the_loop(ctx, assign_case, mem):
    """65 536 vectors per pass: 65 536 + 100 is the smallest input whose loop rewinds the arena and goes round again"""
    from muopdb_amd import lib as L
    from muopdb_amd.index import ivf_assign
    v, cent, mc, thr, (oids, ocnt) = assign_case
    n, d = v.shape
    if mem == "host":
        ids, cnt = ivf_assign(ctx, cent, v, mc, thr)
    else:
        torch = pytest.importorskip("torch")
        dev = torch.device("cuda", torch.cuda.current_device())
        cd, vd = torch.from_numpy(cent).to(dev), torch.from_numpy(v).to(dev)
        idd = torch.zeros((n, mc), dtype=torch.int32, device=dev)
        cnd = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()   # the uploads and fills run on torch's stream, the call on the context's
        ctx.check(ctx.lib.mdb_ivf_assign(ctx.h, C.c_void_p(cd.data_ptr()), C.c_size_t(cent.shape[0]), C.c_void_p(vd.data_ptr()), C.c_size_t(n),
                                         C.c_size_t(d), C.c_size_t(mc), C.c_float(thr), C.c_int(L.MEM_DEVICE),
                                         C.c_void_p(idd.data_ptr()), C.c_void_p(cnd.data_ptr())))
        ctx.sync()
        ids, cnt = idd.cpu().numpy().view(np.uint32), cnd.cpu().numpy().view(np.uint32)
    assert np.array_equal(cnt, ocnt) and np.array_equal(ids, oids)

"""MDB_MEM_DEVICE calls on a BORROWED stream with the host ahead of the GPU (-m gpu).

Every device-memory entry "returns without a sync, asynchronous on the context's stream", and mdb_set_stream binds that stream to the
caller's.  Here each context runs on a stream S that torch also uses (a side stream, or the NULL stream), and two building blocks make
the contract observable:

* the STALL: a chain of 4096 x 4096 f32 torch.mm on S, followed by an event.  While it runs, everything the test and the library
  enqueue on S waits, so the host really is ahead: every call that is supposed to return ahead is followed by
  `assert not stall_end.query()`, and a stall that is too short fails the test instead of letting it pass vacuously.  A window is
  run twice un-stalled first (that sizes the arena and the pinned buffers, is checked against the oracle too, and its second pass gives
  the window's host time); the stall is then max(20 ms, 10 x that host time), and never more than 200 ms in one test.
* DECOYS: the device query buffer holds decoy queries whose oracle rows differ from the real queries' in EVERY row (asserted on the
  CPU).  The real queries reach the buffer only through a copy_(pinned, non_blocking=True) enqueued on S behind the stall, and the
  buffer is overwritten with decoys again on S right behind the call.  Work that the library puts on any other stream, or that
  reads the buffer late, sees decoys.

Expected values are the oracle's: ids exact, score bits equal, counts equal; counters as the oracle counts them, or as the same call
reports them alone on a fresh context where the oracle has no counterpart.

Figures of one run on an MI355X (every stalled window prints its own; pytest -s shows them): one torch.mm of the chain 1.05 ms; the
host side of a window of one asynchronous call 0.011 - 0.068 ms, of two or three calls (sequences, submit + device call) 0.027 -
0.091 ms, so ten times the host time stays far below the floor and the stall actually used is 20 ms (20 products) in every window.
A window that has to wait — a call that synchronises inside, the fifth call of the staging ring, the arena's consolidation — comes
back after 18.0 - 22.1 ms: the length of the stall as the host sees it.
"""
import ctypes as C
import math
import time

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H

pytestmark = pytest.mark.gpu

K, P, EF = 10, 6, 48
USERS = tuple(range(3, 11))                                     # eight users
NQ = 96                                                         # real / decoy query rows per dimension
SHAPES = {"d32b4": (32, 4), "d20b5": (20, 5), "d32b3": (32, 3)}  # read in place / staged (d % 16) / staged (the padding row)
STALL_MIN_MS, STALL_MAX_MS = 20.0, 200.0
NAN_P = 2                                                       # probes of the index with the planted NaN row


def vp(x):
    return C.c_void_p(x)


def sz(x):
    return C.c_size_t(x)


# =================================================================================== the world: files, oracle twins, queries
def _build_files(oracle, d):
    """the four tiny indexes of tests/test_gpu_scratch.py at dimension d (the IVF-PQ with 8-bit codes: at d = 32 its small batches
    take the fused step, at d = 20 — five code bytes, no whole words — coarse search + scan), as bytes with their oracle twins"""
    from muopdb_amd.index import allow_bitmap
    rng = np.random.default_rng(100 + d)
    f = dict(d=d, alone={})
    pool = H.sift_like(4096, d, n_clusters=20, seed=3)
    f["base"] = pool
    # IVF-PQ 2 048 x d, 16 lists, subvectors of 4, 8 bits
    n = 2048
    v = pool[:n]
    cent = H.kmeans(v, 16, iters=3, seed=4)
    cb = H.train_pq_codebook(v[:1500], 4, 8, iters=2)
    f["cent"], f["pq"] = cent, (d, 4, 8, cb)
    f["opq"] = oracle.ProductQuantizer(d, 4, 8, cb)
    index, vec, pls = H.build_ivf_files(v, [100 + 3 * i for i in range(n)], cent, quantize=f["opq"].quantize)
    f["ivf_index"], f["ivf_vec"], f["ivf_lists"] = index, vec, [len(p) for p in pls]
    f["oivf"] = oracle.BlockBasedIvf(index, vec, oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 4, 8, cb))
    f["ivf_bm"] = np.stack([allow_bitmap(np.sort(rng.choice(n, n // 3, replace=False)), n) for _ in range(8)])
    # HNSW 2 000 x d
    hidx, hvec = H.build_hnsw_files(oracle, pool[:2000], list(range(2000)), max_neighbors=8, max_layers=3, ef_construction=40)
    f["hidx"], f["hvec"] = hidx, hvec
    f["ohnsw"] = oracle.BlockBasedHnsw(hidx, hvec, d)
    # eight users' SPANN, and the first user's files as a single-user SPANN
    per_user, most = {}, 0
    for j, u in enumerate(USERS):
        uv = H.sift_like(300 + 40 * j, d, n_clusters=20, seed=3 + j)
        most = max(most, len(uv))
        per_user[u], _, _ = H.build_spann_files(oracle, uv, [1000 * u + i for i in range(len(uv))], 10, seed=j, max_neighbors=8,
                                                max_layers=3, ef_construction=40)
    cat = F.concat_multi_spann(per_user)
    f["margs"] = (cat["user_table"], d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    f["oms"] = oracle.MultiSpannIndex(*f["margs"])
    f["ms_bm"] = allow_bitmap(np.arange(0, most, 2), most)     # even user-local point ids, shared by the batch
    one = per_user[USERS[0]]
    f["sargs"] = (one["hnsw_index"], one["hnsw_vectors"], one["ivf_index"], one["ivf_vectors"])
    f["ospann"] = oracle.Spann(*f["sargs"])
    f["osp"] = oracle.SearchParams(K, 40, num_explored_centroids=4)
    # real queries, and per row a decoy whose nearest IVF centroid is another one
    f["q"] = (pool[rng.choice(4096, NQ, replace=False)] + rng.normal(0, 3, (NQ, d))).astype(np.float32)
    cand = (pool[rng.choice(4096, 8 * NQ, replace=False)] + rng.normal(0, 3, (8 * NQ, d))).astype(np.float32)
    aq, ac, used, decoy = H.assign(f["q"], cent), H.assign(cand, cent), set(), []
    for i in range(NQ):
        j = next(j for j in range(len(cand)) if j not in used and ac[j] != aq[i])
        used.add(j)
        decoy.append(cand[j])
    f["decoy"] = np.asarray(decoy, np.float32)
    if d == 32:
        # a NaN planted the way tests/test_gpu_nonfinite.py plants it: one f32 row of one posting list — exactly the queries that
        # probe that list raise (the oracle) / flag MDB_ERR_NAN (the library); a status, never a fault
        vn = pool[:1024]
        cn = H.kmeans(vn, 8, iters=3, seed=5)
        nindex, nvec, npls = H.build_ivf_files(vn, [7 + 2 * i for i in range(1024)], cn)
        c_star = 5
        bad = vn.copy()
        bad[int(npls[c_star][0]), 5] = np.nan
        vec_bad = F.write_vector_file(bad)
        onan = oracle.BlockBasedIvf(nindex, vec_bad)
        probes = oracle.BlockBasedIvf(nindex, nvec).find_nearest_centroids(f["q"], NAN_P)
        touches = (probes == c_star).any(axis=1)
        hit, miss = np.flatnonzero(touches)[:4], np.flatnonzero(~touches)[:4]
        assert len(hit) == 4 and len(miss) == 4, "the planted list must be probed by some queries and missed by others"
        with pytest.raises(ValueError):
            onan.search(f["q"][hit], K, num_probes=NAN_P)
        f["nan"] = dict(index=nindex, vec=vec_bad, o=onan, hit=hit, miss=miss)
    return f


@pytest.fixture(scope="module")
def files(oracle):
    return {d: _build_files(oracle, d) for d in (32, 20)}


def _load(ctx, f, T, dev, only=None):
    """GPU handles of the world `f` on `ctx` (all of them, or the names in `only`) and the device-resident constants of the calls"""
    from muopdb_amd.index import BlockBasedHnsw, BlockBasedIvf, FlatIndex, MultiSpannIndex, ProductQuantizer, Spann
    make = dict(flat=lambda: FlatIndex(ctx, f["base"]),
                ivf=lambda: BlockBasedIvf(ctx, f["ivf_index"], f["ivf_vec"], ProductQuantizer(*f["pq"])),
                hnsw=lambda: BlockBasedHnsw(ctx, f["hidx"], f["hvec"], f["d"]),
                spann=lambda: Spann(ctx, *f["sargs"]),
                ms=lambda: MultiSpannIndex(ctx, *f["margs"]))
    if "nan" in f:
        make["nan"] = lambda: BlockBasedIvf(ctx, f["nan"]["index"], f["nan"]["vec"])
    g = dict(handles=[])
    for name, fn in make.items():
        if only is None or name in only:
            g[name] = fn()
            g["handles"].append(g[name])
    g["ivf_bm"] = T.from_numpy(f["ivf_bm"].view(np.int32)).to(dev)
    g["ms_bm"] = T.from_numpy(f["ms_bm"].view(np.int32)).to(dev)
    g["cent"] = T.from_numpy(f["cent"]).to(dev)
    T.cuda.synchronize()
    return g


def _unload(g):
    for h in g["handles"]:
        h.close()


# =================================================================================== the stall and the buffers of a call
class Stall:
    """a chain of torch.mm on a resident 4096 x 4096 pair; run(ms, stream) enqueues about `ms` of it and returns the event behind it"""

    def __init__(self, T, dev):
        self.T = T
        self.a, self.b = T.randn(4096, 4096, device=dev), T.randn(4096, 4096, device=dev)
        self.c = T.empty_like(self.a)
        for _ in range(3):
            T.mm(self.a, self.b, out=self.c)
        e0, e1 = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            T.mm(self.a, self.b, out=self.c)
        e1.record()
        T.cuda.synchronize()
        self.mm_ms = e0.elapsed_time(e1) / 10

    def run(self, ms, stream):
        n = max(1, math.ceil(ms / self.mm_ms))
        for _ in range(n):
            self.T.mm(self.a, self.b, out=self.c)
        end = self.T.cuda.Event()
        end.record(stream)
        return end, n


def _as_torch_dtype(a):
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))


class Bufs:
    """one call's device buffers: inputs that hold DECOYS until produce() copies the real rows in from pinned memory (on the current
    stream), poisoned outputs, and pinned mirrors that collect() fills — clone the outputs, put the decoys back, copy out"""

    def __init__(self, T, dev, real, decoy, outs):
        self.T, self.out_dtype = T, {n: np.dtype(dt) for n, (_, dt) in outs.items()}
        self.pin_real = {n: T.from_numpy(_as_torch_dtype(a)).pin_memory() for n, a in real.items()}
        self.pin_decoy = {n: T.from_numpy(_as_torch_dtype(a)).pin_memory() for n, a in decoy.items()}
        self.dev_in = {n: T.from_numpy(_as_torch_dtype(a)).to(dev) for n, a in decoy.items()}
        self.dev_out = {n: T.from_numpy(_as_torch_dtype(np.zeros(shape, dt))).to(dev) for n, (shape, dt) in outs.items()}
        self.pin_out = {n: T.from_numpy(_as_torch_dtype(np.zeros(shape, dt))).pin_memory() for n, (shape, dt) in outs.items()}
        self.keep = None
        T.cuda.synchronize()

    def ptrs(self):
        p = {n: t.data_ptr() for n, t in self.dev_in.items()}
        p.update({n: t.data_ptr() for n, t in self.dev_out.items()})
        return p

    def poison(self):
        for t in self.dev_out.values():
            t.fill_(255 if t.dtype == self.T.uint8 else -1)

    def produce(self):
        for n, t in self.dev_in.items():
            t.copy_(self.pin_real[n], non_blocking=True)

    def collect(self):
        self.keep = {n: t.clone() for n, t in self.dev_out.items()}
        for n, t in self.dev_in.items():
            t.copy_(self.pin_decoy[n], non_blocking=True)
        for n, t in self.keep.items():
            self.pin_out[n].copy_(t, non_blocking=True)

    def host(self):
        return {n: t.numpy().view(self.out_dtype[n]).copy() for n, t in self.pin_out.items()}


class Step:
    """one library call of a window: `ahead` — it is asynchronous and must return while the stall still runs; after() runs right
    behind the call (the host reusing its arrays)"""

    def __init__(self, bufs, call, ahead=True, after=None):
        self.bufs, self.call, self.ahead, self.after = bufs, call, ahead, after


def run_window(T, stall, stream, steps, stall_ms=0.0, what="", sync=True, before=None):
    """On `stream`: poison the outputs; stall; produce every step's inputs; make the calls (a step that must be ahead asserts that the
    stall has not ended); collect.  No mdb_sync: the stream alone orders everything.  Returns (host ms of the calls, the stall's event)."""
    end = None
    with T.cuda.stream(stream):
        for s in steps:
            s.bufs.poison()
        if before:
            before()
        if stall_ms:
            end, n = stall.run(stall_ms, stream)
        for s in steps:
            s.bufs.produce()
        t0 = time.perf_counter()
        for i, s in enumerate(steps):
            s.call()
            if end is not None and s.ahead:
                assert not end.query(), "%s: call %d came back after the %.0f ms stall had ended — it did not return ahead" % (what, i, stall_ms)
            if s.after:
                s.after()
        host_ms = (time.perf_counter() - t0) * 1e3
        for s in steps:
            s.bufs.collect()
    if sync:
        stream.synchronize()
    if end is not None:
        print("[stall] %s: %.1f ms nominal (%d products of %.2f ms), host side %.3f ms" % (what, stall_ms, n, stall.mm_ms, host_ms))
    return host_ms, end


def stall_for(host_ms):
    """>= 10 x the window's un-stalled host time, from 20 ms; a window whose host side needs more than the cap is an error"""
    assert 10 * host_ms <= STALL_MAX_MS, "the window's host side takes %.2f ms: no stall within %.0f ms covers it tenfold" % (host_ms, STALL_MAX_MS)
    return max(STALL_MIN_MS, 10 * host_ms)


def three_passes(T, stall, stream, steps, check, what, before=None):
    """un-stalled (sizes every buffer), un-stalled again (the host time), stalled; check() after each"""
    run_window(T, stall, stream, steps, what=what, before=before)
    check("first un-stalled pass")
    host_ms, _ = run_window(T, stall, stream, steps, what=what, before=before)
    check("second un-stalled pass")
    run_window(T, stall, stream, steps, stall_for(host_ms), what=what, before=before)
    check("stalled pass")


class Rig:
    """a context bound to a stream that torch uses too, with the worlds of both dimensions loaded on it"""

    def __init__(self, T, kind, files, stall):
        from muopdb_amd import lib as L
        self.T, self.kind, self.stall = T, kind, stall
        self.dev = T.device("cuda", T.cuda.current_device())
        self.stream = T.cuda.Stream() if kind == "side" else T.cuda.default_stream()   # kept alive until close()
        self.ctx = L.Context(0)
        self.bind(self.ctx)
        self.g = {d: _load(self.ctx, f, T, self.dev) for d, f in files.items()}

    def bind(self, ctx):
        if self.kind == "null":
            assert self.stream.cuda_stream == 0, "torch's default stream is not the NULL stream here"
            ctx.set_stream(0)
        else:
            ctx.set_stream(self.stream.cuda_stream)

    def bufs(self, real, decoy, outs):
        return Bufs(self.T, self.dev, real, decoy, outs)

    def passes(self, steps, check, what, before=None):
        three_passes(self.T, self.stall, self.stream, steps, check, "%s/%s" % (self.kind, what), before)

    def window(self, steps, stall_ms=0.0, what="", **kw):
        return run_window(self.T, self.stall, self.stream, steps, stall_ms, "%s/%s" % (self.kind, what), **kw)

    def close(self):
        self.T.cuda.synchronize()
        for g in self.g.values():
            _unload(g)
        self.ctx.close()
        self.stream = None


@pytest.fixture(scope="module")
def torch_mod():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def stall(torch_mod):
    T = torch_mod
    return Stall(T, T.device("cuda", T.cuda.current_device()))


@pytest.fixture(scope="module", params=["side", "null"])
def rig(request, torch_mod, files, stall):
    r = Rig(torch_mod, request.param, files, stall)
    yield r
    r.close()


# =================================================================================== rows: what is compared
def search_rows(res, b, found=None):
    """per row: (count, doc ids up to the count, the scores' bytes up to the count[, found])"""
    rows = []
    for i in range(b):
        c = int(res.counts[i])
        row = (c, tuple(res.doc_ids(i)), np.ascontiguousarray(res.scores[i, :c], np.float32).tobytes())
        rows.append(row + ((int(found[i]),) if found is not None else ()))
    return rows


def got_search_rows(out, b, with_found=False):
    from muopdb_amd.index import SearchResult
    h = out["ids"].view(np.uint64)
    res = SearchResult(h.shape[0], h.shape[1], h[:, :, 0], h[:, :, 1], out["sc"], out["cn"].view(np.uint32))
    return search_rows(res, b, out["fo"] if with_found else None)


def assert_rows(got, want, what):
    assert len(got) == len(want), what
    for i, (a, e) in enumerate(zip(got, want)):
        assert a == e, "%s: row %d differs from the oracle's\n got  %r\n want %r" % (what, i, a[:2], e[:2])


def assert_decoys_differ(want, wdecoy, rowwise, what):
    """the precondition of every window: with the decoys in place of the real rows the oracle's result differs in EVERY row"""
    if rowwise:
        same = [i for i, (a, e) in enumerate(zip(want, wdecoy)) if a[:2] == e[:2]]
        assert not same, "%s: decoy rows %s give the real rows' result" % (what, same)
    else:
        assert want != wdecoy, what


def search_outs(b, found=False):
    o = {"ids": ((b, K, 2), np.uint64), "sc": ((b, K), np.float32), "cn": ((b,), np.uint32)}
    if found:
        o["fo"] = ((b,), np.uint8)
    return o


def users_of(b, shift=0):
    return [USERS[(3 * i + shift) % len(USERS)] for i in range(b)]


def spc():
    from muopdb_amd.index import SearchParams
    return SearchParams(K, 40).with_num_explored_centroids(4).to_c()


# =================================================================================== the families of case 1
class Family:
    asynchronous, rowwise, found = True, True, False

    def inputs(self, f, b, which, off=0):
        return {"q": f["q" if which == "real" else "decoy"][np.arange(off, off + b) % NQ]}   # (a batch beyond the pool repeats its rows)

    def outputs(self, f, b):
        return search_outs(b, self.found)

    def got(self, f, out, b):
        return got_search_rows(out, b, self.found)


class Flat(Family):
    def outputs(self, f, b):
        return {"ids": ((b, K), np.uint32), "sc": ((b, K), np.float32), "cn": ((b,), np.uint32)}

    def invoke(self, ctx, g, f, p, b):
        g["flat"].search_device(p["q"], b, K, p["ids"], p["sc"], p["cn"])

    def want(self, orc, f, inp, b):
        ids, dist = orc.flat_topk(0, f["base"], inp["q"], K)
        return [(K, tuple(int(x) for x in ids[i]), dist[i].tobytes()) for i in range(b)]

    def got(self, f, out, b):
        return [(int(out["cn"][i]), tuple(int(x) for x in out["ids"][i]), out["sc"][i].tobytes()) for i in range(b)]


class Ivf(Family):
    """probes = NULL: the fused step at d = 32, coarse search + scan at d = 20"""

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        ctx.check(ctx.lib.mdb_ivf_search(g["ivf"].h, vp(p["q"]), sz(b), None, sz(P), sz(K), C.c_int(L.MEM_DEVICE), vp(p["ids"]), vp(p["sc"]),
                                         vp(p["cn"])))

    def want(self, orc, f, inp, b):
        return search_rows(f["oivf"].search(inp["q"], K, num_probes=P), b)


class IvfProbes(Family):
    """explicit probes, device-resident and produced on the stream like the queries"""

    def inputs(self, f, b, which, off=0):
        q = Family.inputs(self, f, b, which, off)["q"]
        return {"q": q, "probes": f["oivf"].find_nearest_centroids(q, P)}

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        ctx.check(ctx.lib.mdb_ivf_search(g["ivf"].h, vp(p["q"]), sz(b), vp(p["probes"]), sz(P), sz(K), C.c_int(L.MEM_DEVICE), vp(p["ids"]),
                                         vp(p["sc"]), vp(p["cn"])))

    def want(self, orc, f, inp, b):
        return search_rows(f["oivf"].search(inp["q"], K, probes=inp["probes"]), b)


class IvfFiltered(Family):
    """one device bitmap per query"""

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        ctx.check(ctx.lib.mdb_ivf_search_filtered(g["ivf"].h, vp(p["q"]), sz(b), None, sz(P), sz(K), C.c_int(L.MEM_DEVICE), vp(g["ivf_bm"].data_ptr()),
                                                  sz(b), sz(f["ivf_bm"].shape[1]), vp(p["ids"]), vp(p["sc"]), vp(p["cn"])))

    def want(self, orc, f, inp, b):
        with orc.planner_filter(f["ivf_bm"][:b]):
            return search_rows(f["oivf"].search(inp["q"], K, num_probes=P), b)


class Hnsw(Family):
    def invoke(self, ctx, g, f, p, b):
        g["hnsw"].ann_search_device(p["q"], b, K, EF, p["ids"], p["sc"], p["cn"])

    def want(self, orc, f, inp, b):
        return search_rows(f["ohnsw"].ann_search(inp["q"], K, EF), b)


class SpannOne(Family):
    found = True

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        c = spc()
        ctx.check(ctx.lib.mdb_spann_search(g["spann"].h, vp(p["q"]), sz(b), C.byref(c), C.c_int(L.MEM_DEVICE), vp(p["ids"]), vp(p["sc"]), vp(p["cn"]),
                                           vp(p["fo"])))

    def want(self, orc, f, inp, b):
        r = f["ospann"].search(inp["q"], f["osp"])
        return search_rows(r, b, r.found)


class MultiSpann(Family):
    found = True

    def __init__(self, shift=0, filtered=False):
        self.shift, self.filtered = shift, filtered

    def invoke(self, ctx, g, f, p, b, user_array=None):
        from muopdb_amd import lib as L
        c = spc()
        ua = user_array if user_array is not None else L.u128_array(users_of(b, self.shift))
        if self.filtered:
            ctx.check(ctx.lib.mdb_multi_spann_search_filtered(g["ms"].h, ua, vp(p["q"]), sz(b), C.byref(c), C.c_int(L.MEM_DEVICE),
                                                              vp(g["ms_bm"].data_ptr()), sz(1), sz(f["ms_bm"].shape[0]), vp(p["ids"]), vp(p["sc"]),
                                                              vp(p["cn"]), vp(p["fo"])))
        else:
            ctx.check(ctx.lib.mdb_multi_spann_search(g["ms"].h, ua, vp(p["q"]), sz(b), C.byref(c), C.c_int(L.MEM_DEVICE), vp(p["ids"]), vp(p["sc"]),
                                                     vp(p["cn"]), vp(p["fo"])))

    def want(self, orc, f, inp, b):
        if self.filtered:
            with orc.planner_filter(f["ms_bm"]):
                r = f["oms"].search_for_user(users_of(b, self.shift), inp["q"], f["osp"])
        else:
            r = f["oms"].search_for_user(users_of(b, self.shift), inp["q"], f["osp"])
        return search_rows(r, b, r.found)


class Centroids(Family):
    def outputs(self, f, b):
        return {"probes": ((b, P), np.uint32)}

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        ctx.check(ctx.lib.mdb_ivf_find_nearest_centroids(g["ivf"].h, vp(p["q"]), sz(b), sz(P), C.c_int(L.MEM_DEVICE), vp(p["probes"])))

    def want(self, orc, f, inp, b):
        pr = f["oivf"].find_nearest_centroids(inp["q"], P)
        return [(P, tuple(int(x) for x in pr[i])) for i in range(b)]

    def got(self, f, out, b):
        return [(P, tuple(int(x) for x in out["probes"][i])) for i in range(b)]


class Quantize(Family):
    """synchronises inside (the uploaded codebook dies with the call): ordering only"""
    asynchronous = False

    def outputs(self, f, b):
        return {"codes": ((b, f["d"] // 4), np.uint8)}

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd.index import ProductQuantizer
        ProductQuantizer(*f["pq"]).quantize_device(ctx, p["q"], b, p["codes"])

    def want(self, orc, f, inp, b):
        codes = f["opq"].quantize(inp["q"])
        return [(codes.shape[1], tuple(int(x) for x in codes[i])) for i in range(b)]

    def got(self, f, out, b):
        return [(out["codes"].shape[1], tuple(int(x) for x in out["codes"][i])) for i in range(b)]


class Assign(Family):
    """mdb_ivf_assign with device data; synchronises inside: ordering only"""
    asynchronous = False

    def outputs(self, f, b):
        return {"ids": ((b, 2), np.uint32), "cn": ((b,), np.uint32)}

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        ctx.check(ctx.lib.mdb_ivf_assign(ctx.h, vp(g["cent"].data_ptr()), sz(f["cent"].shape[0]), vp(p["q"]), sz(b), sz(f["d"]), sz(2), C.c_float(0.1),
                                         C.c_int(L.MEM_DEVICE), vp(p["ids"]), vp(p["cn"])))

    def want(self, orc, f, inp, b):
        ids, cnt = orc.ivf_assign(f["cent"], inp["q"], 2, 0.1)
        return [(int(cnt[i]), tuple(int(x) for x in ids[i])) for i in range(b)]

    def got(self, f, out, b):
        return [(int(out["cn"][i]), tuple(int(x) for x in out["ids"][i])) for i in range(b)]


class Kmeans(Family):
    """mdb_kmeans_fit with device data (32 + b rows, four clusters); synchronises inside: ordering only"""
    asynchronous, rowwise = False, False
    INIT = np.array([0, 5, 11, 17], np.uint64)

    def inputs(self, f, b, which, off=0):
        return {"q": f["q" if which == "real" else "decoy"][off:off + 32 + b]}

    def outputs(self, f, b):
        return {"cent": ((4, f["d"]), np.float32), "lab": ((32 + b,), np.uint32)}

    def invoke(self, ctx, g, f, p, b):
        from muopdb_amd import lib as L
        err, it = C.c_float(), C.c_uint32()
        ctx.check(ctx.lib.mdb_kmeans_fit(ctx.h, vp(p["q"]), sz(32 + b), sz(f["d"]), sz(4), sz(5), C.c_float(0.0), L.ptr(self.INIT, C.c_uint64), sz(4),
                                         C.c_int(L.MEM_DEVICE), vp(p["cent"]), vp(p["lab"]), C.byref(err), C.byref(it)))

    def want(self, orc, f, inp, b):
        cent, lab, _, _ = orc.kmeans_fit(inp["q"], 4, 5, 0.0, self.INIT)
        return [cent.tobytes(), lab.tobytes()]

    def got(self, f, out, b):
        return [out["cent"].tobytes(), out["lab"].tobytes()]


FAMS = dict(flat=Flat(), ivf=Ivf(), ivf_probes=IvfProbes(), ivf_filtered=IvfFiltered(), hnsw=Hnsw(), spann=SpannOne(), multi_spann=MultiSpann(),
            centroids=Centroids(), quantize=Quantize(), assign=Assign(), kmeans=Kmeans())


def make_step(rig, oracle, f, g, fam, b, off=0, what="", ahead=None, ctx=None):
    """buffers, oracle rows and the Step of one call of `fam` on rows [off, off + b) — the decoy precondition is asserted here"""
    real, decoy = fam.inputs(f, b, "real", off), fam.inputs(f, b, "decoy", off)
    want, wdecoy = fam.want(oracle, f, real, b), fam.want(oracle, f, decoy, b)
    assert_decoys_differ(want, wdecoy, fam.rowwise, what)
    bufs = rig.bufs(real, decoy, fam.outputs(f, b))
    ptrs = bufs.ptrs()
    c = ctx or rig.ctx
    step = Step(bufs, lambda: fam.invoke(c, g, f, ptrs, b), fam.asynchronous if ahead is None else ahead)
    step.want, step.got = want, (lambda: fam.got(f, bufs.host(), b))
    return step


# =================================================================================== 1. ordering on the borrowed stream
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("fam", list(FAMS))
def test_call_is_ordered_on_the_borrowed_stream(rig, files, oracle, fam, shape):
    """stall; real queries produced on S; the call (ahead of the stall where the entry is asynchronous); on S the outputs are cloned
    and the query buffer overwritten with decoys again; D2H; S.synchronize() — no mdb_sync anywhere; rows equal the oracle's"""
    d, b = SHAPES[shape]
    f, g = files[d], rig.g[d]
    what = "%s %s" % (fam, shape)
    step = make_step(rig, oracle, f, g, FAMS[fam], b, what=what)
    rig.passes([step], lambda when: assert_rows(step.got(), step.want, "%s, %s" % (what, when)), what)


# =================================================================================== 2. the staging ring under run-ahead
def _multi_spann_sequence(rig, oracle, f, g, batches, ahead, ctx=None):
    """consecutive mdb_multi_spann_search device calls that share ONE host user-id array: every call names other users, and the array
    is overwritten with the next call's users (other valid ones) the moment a call returns.  Call 2 is filtered."""
    from muopdb_amd import lib as L
    bmax = max(batches)
    ua = L.u128_array([USERS[0]] * bmax)

    def put(users):
        for i, u in enumerate(users):
            ua[i].lo, ua[i].hi = u & 0xFFFFFFFFFFFFFFFF, u >> 64

    steps, off = [], 0
    fams = [MultiSpann(shift=j + 1, filtered=(j == 2)) for j in range(len(batches))]
    for j, b in enumerate(batches):
        if off + b > NQ:
            off = 0
        st = make_step(rig, oracle, f, g, fams[j], b, off=off, what="multi-spann call %d" % j, ahead=ahead[j], ctx=ctx)
        ptrs, fam, c = st.bufs.ptrs(), fams[j], ctx or rig.ctx
        st.call = (lambda fam=fam, ptrs=ptrs, b=b: fam.invoke(c, g, f, ptrs, b, user_array=ua))
        nxt = users_of(bmax, fams[(j + 1) % len(batches)].shift)
        st.after = (lambda nxt=nxt: put(nxt))
        steps.append(st)
        off += b
    return steps, (lambda: put(users_of(bmax, fams[0].shift)))


def _check_all(steps, what):
    def check(when):
        for j, st in enumerate(steps):
            assert_rows(st.got(), st.want, "%s, call %d, %s" % (what, j, when))
    return check


def test_staging_ring_six_calls_behind_one_stall(rig, files, oracle):
    """Six mdb_multi_spann_search device calls (b = 4, call 2 filtered) behind one stall.  mdb_stage_small keeps FOUR pinned slots, each
    guarded by the event recorded behind its copy, and a device call stages exactly once (its user slots; a device bitmap is taken in
    place), so calls 0 - 3 return ahead — asserted — and call 4, the fifth staging, waits in hipEventSynchronize for call 0's copy,
    i.e. for the stall to end; call 5 follows at once.  Without that wait call 4 would overwrite slot 0 while call 0's copy is still
    queued, and call 0 would search call 4's users."""
    f, g = files[32], rig.g[32]
    steps, before = _multi_spann_sequence(rig, oracle, f, g, [4] * 6, ahead=[True] * 4 + [False] * 2)
    rig.passes(steps, _check_all(steps, "ring"), "ring x6", before=before)


@pytest.mark.parametrize("big", [64, 4100])
def test_arena_grows_mid_sequence_behind_the_stall(rig, files, oracle, big):
    """b = 4, 4, big, 4, 4, 4 on a context that has only ever served b = 4: the third call spills into a second arena chunk while the
    kernels of the first two are still queued, the fourth call's begin() consolidates (release_cb waits for the stream before it frees
    a chunk).  Calls 0 and 1 return ahead; from the growth on a call may block.  mdb_pinned serves host-memory calls only — every one
    of them ends with a stream sync, and none is accepted while a submit is pending — so no device call reaches its regrowth; the
    pinned buffers a device call does use are the ring's slots, 16 KB = 4 096 user slots each: big = 4 100 makes the third call free
    its slot and take a larger one, behind the slot's event, while the other slots' copies are still queued."""
    from muopdb_amd import lib as L
    f = files[32]
    ctx = L.Context(0)
    rig.bind(ctx)
    g = _load(ctx, f, rig.T, rig.dev, only=("ms",))
    try:
        warm, before = _multi_spann_sequence(rig, oracle, f, g, [4] * 3, ahead=[True] * 3, ctx=ctx)
        for when in ("first un-stalled pass", "second un-stalled pass"):
            host_ms, _ = rig.window(warm, what="grow warm-up", before=before)
            _check_all(warm, "grow warm-up")(when)
        steps, before = _multi_spann_sequence(rig, oracle, f, g, [4, 4, big, 4, 4, 4], ahead=[True, True] + [False] * 4, ctx=ctx)
        rig.window(steps, stall_for(2 * host_ms), what="grow 4-4-%d-4-4-4" % big, before=before)
        _check_all(steps, "grow")("stalled pass")
        rig.window(steps, what="grow again", before=before)      # the consolidated arena serves the same sequence again
        _check_all(steps, "grow")("un-stalled pass behind it")
    finally:
        rig.T.cuda.synchronize()
        _unload(g)
        ctx.close()


# =================================================================================== 3. counters after device-call sequences
SEQUENCES = {
    "spann>hnsw": [("spann", 4, {}), ("hnsw", 4, {})],
    "spann>spann": [("multi_spann", 4, {}), ("multi_spann", 5, {})],
    "spann(merge and remap apart)>spann": [("multi_spann", 4, {"MDB_SCAN_NO_FUSED_REMAP": 1}), ("multi_spann", 5, {})],
    "spann>spann(merge and remap apart)": [("multi_spann", 4, {}), ("multi_spann", 5, {"MDB_SCAN_NO_FUSED_REMAP": 1})],
    "fused x3": [("ivf", 4, {}), ("ivf", 7, {}), ("ivf", 3, {})],
    "fused>spann>fused": [("ivf", 4, {}), ("multi_spann", 4, {}), ("ivf", 5, {})],
    "hnsw>flat": [("hnsw", 4, {}), ("flat", 4, {})],
}
INDEX_OF = dict(spann="spann", multi_spann="ms", ivf="ivf", hnsw="hnsw", flat="flat")


def _with_options(ctx, opts, call):
    def wrapped():
        import contextlib
        with contextlib.ExitStack() as st:
            for name, val in opts.items():
                st.enter_context(ctx.option(name, val))
            call()
    return wrapped


def _stats_alone(rig, oracle, f, fam, b, off, opts):
    """mdb_get_stats of the same call made alone on a fresh context (on its own stream; torch's work is finished before and the
    context is synchronised behind)"""
    from muopdb_amd import lib as L
    key = (fam, b, off, tuple(sorted(opts.items())))
    if key not in f["alone"]:
        ctx = L.Context(0)
        g = _load(ctx, f, rig.T, rig.dev, only=(INDEX_OF[fam],))
        try:
            st = make_step(rig, oracle, f, g, FAMS[fam], b, off=off, what="alone", ctx=ctx)
            st.bufs.produce()
            rig.T.cuda.synchronize()
            _with_options(ctx, opts, st.call)()
            ctx.sync()
            f["alone"][key] = ctx.stats()
            st.bufs.collect()
            rig.T.cuda.synchronize()
            assert_rows(st.got(), st.want, "alone %s" % (key,))
        finally:
            _unload(g)
            ctx.close()
    return f["alone"][key]


def _oracle_counters(oracle, f, fam, b, off):
    """what the oracle itself counts for the call: HNSW (distance evaluations, expanded nodes); IVF the posting-list entries of the
    probed lists (nothing is tombstoned or filtered: every entry is scored); flat n x b"""
    q = f["q"][off:off + b]
    if fam == "hnsw":
        f["ohnsw"].stats()
        f["ohnsw"].ann_search(q, K, EF)
        evals, expanded = f["ohnsw"].stats()
        return dict(distance_evals=evals, expanded_nodes=expanded, scored_vectors=0)
    if fam == "ivf":
        probes = f["oivf"].find_nearest_centroids(q, P)
        return dict(scored_vectors=int(sum(f["ivf_lists"][int(c)] for row in probes for c in row)), distance_evals=0, expanded_nodes=0)
    if fam == "flat":
        return dict(scored_vectors=len(f["base"]) * b, distance_evals=0, expanded_nodes=0)
    return {}


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_stats_are_the_last_calls_after_a_sequence(rig, files, oracle, seq):
    """mdb_get_stats behind a sequence of device calls, un-stalled and stalled, reports the LAST call: the oracle's counters where it
    has them, and in every field what the same call reports alone on a fresh context.  The sequences walk the bookkeeping that saves
    memset launches: counters_clean / counter_base = 24 behind a SPANN device call whose merge launch saved the counters (and NOT behind
    one that merged and remapped in two launches), the fused step's two alternating sets, dev_counters = false behind a flat scan."""
    f, g = files[32], rig.g[32]
    steps, off = [], 0
    for fam, b, opts in SEQUENCES[seq]:
        st = make_step(rig, oracle, f, g, FAMS[fam], b, off=off, what="%s: %s" % (seq, fam))
        st.call = _with_options(rig.ctx, opts, st.call)
        steps.append(st)
        last = (fam, b, off, opts)
        off += 8
    alone = _stats_alone(rig, oracle, f, *last)
    counted = _oracle_counters(oracle, f, *last[:3])
    assert all(alone[k] == v for k, v in counted.items()), (seq, alone, counted)
    if last[0] in ("spann", "multi_spann"):
        assert alone["distance_evals"] > 0 and alone["scored_vectors"] > 0, alone

    def check(when):
        st = rig.ctx.stats()
        assert st == alone, "%s, %s: mdb_get_stats gives %r, the last call alone %r" % (seq, when, st, alone)
        _check_all(steps, seq)(when)
    rig.passes(steps, check, seq)


# =================================================================================== 4. submit / poll / wait
def _submitters(f, g, b, off=0):
    from muopdb_amd.index import SearchParams
    sp = SearchParams(K, 40).with_num_explored_centroids(4)
    q = f["q"][off:off + b]
    return dict(
        ivf=(lambda: g["ivf"].search_submit(q, K, P), lambda: search_rows(f["oivf"].search(q, K, num_probes=P), b)),
        hnsw=(lambda: g["hnsw"].ann_search_submit(q, K, EF), lambda: search_rows(f["ohnsw"].ann_search(q, K, EF), b)),
        spann=(lambda: g["spann"].search_submit(q, sp), lambda: search_rows(f["ospann"].search(q, f["osp"]), b)),
        multi_spann=(lambda: g["ms"].search_for_user_submit(users_of(b), q, sp),
                     lambda: search_rows(f["oms"].search_for_user(users_of(b), q, f["osp"]), b)))


@pytest.mark.parametrize("fam", ["ivf", "hnsw", "spann", "multi_spann"])
def test_submit_poll_wait_on_the_borrowed_stream(rig, files, oracle, fam):
    """behind a stall a submitted call is pending: mdb_poll says no, a host-memory call is refused (and neither blocks), the refusal
    leaves the pending call alone; S.synchronize() — mdb_poll says yes — mdb_wait hands over the oracle's rows"""
    from muopdb_amd import lib as L
    T, f, g, b = rig.T, files[32], rig.g[32], 4
    submit, want = _submitters(f, g, b)[fam]
    want = want()
    host_ms = 0.0
    for stalled in (False, False, True):
        with T.cuda.stream(rig.stream):
            end = rig.stall.run(stall_for(host_ms), rig.stream)[0] if stalled else None
            t0 = time.perf_counter()
            pend = submit()
            host_ms = (time.perf_counter() - t0) * 1e3
            if stalled:
                assert not end.query(), "the submit did not return ahead"
                assert pend.done() is False
                with pytest.raises(L.MuopdbError) as e:
                    g["flat"].search(f["q"][:b], K)
                assert e.value.status == L.MDB_ERR_INVALID_ARG and "pending" in str(e.value)
                assert not end.query(), "mdb_poll or the refused host call waited for the stream"
        rig.stream.synchronize()
        assert pend.done() is True
        assert_rows(search_rows(pend.wait(), b), want, "%s submit, stalled=%s" % (fam, stalled))
        rig.ctx.sync()


@pytest.mark.parametrize("fam", ["ivf", "hnsw", "spann", "multi_spann"])
def test_device_call_between_submit_and_wait(rig, files, oracle, fam):
    """a device-memory call of the same family on the same context between *_submit and mdb_wait, behind a stall: both results right"""
    f, g, b = files[32], rig.g[32], 4
    submit, want = _submitters(f, g, b)[fam]
    want = want()
    step = make_step(rig, oracle, f, g, FAMS[fam], b, off=16, what="%s device call" % fam)
    pend = [None]
    inner = step.call

    def both():
        pend[0] = submit()
        inner()
    step.call = both

    def check(when):
        assert_rows(search_rows(pend[0].wait(), b), want, "%s submit, %s" % (fam, when))
        rig.ctx.sync()
        assert_rows(step.got(), step.want, "%s device call, %s" % (fam, when))
    rig.passes([step], check, "%s submit + device" % fam)


def _assert_nan_decoys_differ(nan, f, want, b):
    """the decoys under the clean rows give other rows (or meet the NaN: another status)"""
    try:
        wdecoy = search_rows(nan["o"].search(f["decoy"][nan["miss"]], K, num_probes=NAN_P), b)
    except ValueError:
        return
    assert_decoys_differ(want, wdecoy, True, "index with the planted NaN")


@pytest.mark.parametrize("first", ["wait", "sync"])
@pytest.mark.parametrize("planted", ["submit", "device"])
def test_submit_and_device_call_keep_their_own_errors(rig, files, oracle, planted, first):
    """A submitted call and a device-memory call behind it on ONE context, one of the two meeting the planted NaN: mdb_wait reports
    the submitted call's status and mdb_sync the device call's — whichever of the two is called first — and the clean one's rows are
    the oracle's.  (Both used to travel through one host flag word: mdb_sync in front of mdb_wait handed the device call's status to
    mdb_wait as well and dropped the submitted call's.)"""
    from muopdb_amd import lib as L
    f, nan = files[32], files[32]["nan"]
    g = rig.g[32]["nan"]
    sub_rows, dev_rows = (nan["hit"], nan["miss"]) if planted == "submit" else (nan["miss"], nan["hit"])
    b = 4
    want = search_rows(nan["o"].search(f["q"][nan["miss"]], K, num_probes=NAN_P), b)
    _assert_nan_decoys_differ(nan, f, want, b)

    class NanIvf(Ivf):
        def inputs(self, f_, b_, which, off=0):
            return {"q": (f_["q"] if which == "real" else f_["decoy"])[dev_rows]}

        def invoke(self, ctx, g_, f_, p, b_):
            ctx.check(ctx.lib.mdb_ivf_search(g.h, vp(p["q"]), sz(b_), None, sz(NAN_P), sz(K), C.c_int(L.MEM_DEVICE), vp(p["ids"]), vp(p["sc"]),
                                             vp(p["cn"])))          # MDB_OK here, whatever the rows meet

    bufs = rig.bufs(NanIvf().inputs(f, b, "real"), NanIvf().inputs(f, b, "decoy"), search_outs(b))
    ptrs = bufs.ptrs()
    pend = [None]

    def both():
        pend[0] = g.search_submit(f["q"][sub_rows], K, NAN_P)
        NanIvf().invoke(rig.ctx, None, f, ptrs, b)
    step = Step(bufs, both, ahead=True)

    def status(call):
        try:
            call()
            return L.MDB_OK
        except L.MuopdbError as e:
            return e.status

    def check(when):
        res = [None]

        def wait():
            res[0] = pend[0].wait()
        order = [("wait", wait), ("sync", rig.ctx.sync)]
        got = {name: status(call) for name, call in (order if first == "wait" else order[::-1])}
        expect = {"wait": 5 if planted == "submit" else 0, "sync": 5 if planted == "device" else 0}
        assert got == expect, "%s, NaN planted in the %s call, %s first: statuses %r, expected %r (5 = MDB_ERR_NAN)" % (when, planted, first, got, expect)
        assert status(rig.ctx.sync) == L.MDB_OK and status(lambda: rig.ctx.check(rig.ctx.lib.mdb_wait(rig.ctx.h))) == L.MDB_OK
        if planted == "device":
            assert_rows(search_rows(res[0], b), want, "the clean submitted call, %s" % when)
        else:
            assert_rows(got_search_rows(bufs.host(), b), want, "the clean device call, %s" % when)
    rig.passes([step], check, "NaN in %s, %s first" % (planted, first))


# =================================================================================== 5. deferred errors on a borrowed stream
def test_deferred_nan_on_the_borrowed_stream(rig, files, oracle):
    """a device call that meets the planted NaN returns MDB_OK, and so does a clean one issued behind it before any sync (both ahead
    of the stall); then mdb_sync returns MDB_ERR_NAN once and MDB_OK after that, and the clean call's rows are the oracle's"""
    from muopdb_amd import lib as L
    f, nan = files[32], files[32]["nan"]
    g, b = rig.g[32]["nan"], 4
    want = search_rows(nan["o"].search(f["q"][nan["miss"]], K, num_probes=NAN_P), b)
    _assert_nan_decoys_differ(nan, f, want, b)
    steps = []
    for rows in (nan["hit"], nan["miss"]):
        bufs = rig.bufs({"q": f["q"][rows]}, {"q": f["decoy"][rows]}, search_outs(b))
        p = bufs.ptrs()
        steps.append(Step(bufs, lambda p=p: rig.ctx.check(rig.ctx.lib.mdb_ivf_search(g.h, vp(p["q"]), sz(b), None, sz(NAN_P), sz(K), C.c_int(L.MEM_DEVICE),
                                                                                  vp(p["ids"]), vp(p["sc"]), vp(p["cn"])))))

    def check(when):
        with pytest.raises(L.MuopdbError) as e:
            rig.ctx.sync()
        assert e.value.status == 5, (when, e.value)
        rig.ctx.sync()
        assert_rows(got_search_rows(steps[1].bufs.host(), b), want, "the clean call behind the NaN call, %s" % when)
    rig.passes(steps, check, "deferred NaN")


# =================================================================================== 6. switching streams
def test_switching_streams_and_a_second_context_on_an_attached_handle(torch_mod, files, oracle, stall):
    """one context: its own stream -> S1 -> S2 -> NULL, an HNSW and an IVF-PQ device search on each.  On its own stream the context is
    NOT ordered with torch: the test synchronises torch before the call and the context behind it.  On a borrowed stream the window
    runs behind a stall and is NOT synchronised: the next mdb_set_stream must drain the old stream (the stall's event and the stream
    report done when it returns).  A second context on a third borrowed stream searches the same resident indexes through attached
    handles between the first context's calls; every result equals the oracle's."""
    from muopdb_amd import lib as L
    T = torch_mod
    dev = T.device("cuda", T.cuda.current_device())
    f = files[32]

    class Plain:  # what make_step needs of a rig
        def __init__(self, ctx):
            self.ctx = ctx

        def bufs(self, real, decoy, outs):
            return Bufs(T, dev, real, decoy, outs)

    ctx1, ctx2 = L.Context(0), L.Context(0)
    s1, s2, s3, null = T.cuda.Stream(), T.cuda.Stream(), T.cuda.Stream(), T.cuda.default_stream()
    g1 = _load(ctx1, f, T, dev, only=("hnsw", "ivf"))
    ctx2.set_stream(s3.cuda_stream)
    g2 = dict(handles=[], hnsw=g1["hnsw"].attach(ctx2), ivf=g1["ivf"].attach(ctx2), ivf_bm=g1["ivf_bm"], ms_bm=g1["ms_bm"], cent=g1["cent"])
    g2["handles"] = [g2["hnsw"], g2["ivf"]]
    try:
        def steps_of(ctx, g, off):
            return [make_step(Plain(ctx), oracle, f, g, FAMS[fam], 4, off=off + 4 * i, what="switch %s" % fam, ctx=ctx) for i, fam in enumerate(("hnsw", "ivf"))]

        other = steps_of(ctx2, g2, 80)
        run_window(T, stall, s3, other, what="attached handles, first un-stalled pass")
        _check_all(other, "second context")("first un-stalled pass")
        other_ms, _ = run_window(T, stall, s3, other, what="attached handles, second un-stalled pass")
        _check_all(other, "second context")("second un-stalled pass")

        def other_context(when):
            run_window(T, stall, s3, other, stall_for(other_ms), what="attached handles on a third stream, " + when)
            _check_all(other, "second context")(when)

        # ---- its own (non-blocking) stream
        own = steps_of(ctx1, g1, 0)
        for s in own:
            s.bufs.produce()
        T.cuda.synchronize()
        for s in own:
            s.call()
        ctx1.sync()
        for s in own:
            s.bufs.collect()
        T.cuda.synchronize()
        _check_all(own, "own stream")("")
        other_context("behind the own-stream calls")
        # ---- S1 -> S2 -> NULL (-> S1): each switch drains the stream before.  The stalled window is left un-synchronised: the host is
        # ahead when it asks for the switch, and reads the window's pinned results the moment the switch returns
        pending = None
        for off, (name, stream) in enumerate((("S1", s1), ("S2", s2), ("NULL", null), ("S1 again", s1))):
            ctx1.set_stream(stream.cuda_stream)
            if pending:
                pname, pstream, psteps, pend = pending
                assert pend.query() and pstream.query(), "mdb_set_stream returned before %s had drained" % pname
                _check_all(psteps, "on " + pname)("stalled, read behind the switch with no synchronize")
            if off < 3:   # (eight stalled windows of 20 ms in this test: 160 ms)
                other_context("behind the switch to " + name)
            st = steps_of(ctx1, g1, 8 + 8 * off)
            run_window(T, stall, stream, st, what="warm-up on " + name)
            _check_all(st, "on " + name)("first un-stalled pass")
            host_ms, _ = run_window(T, stall, stream, st, what="warm-up on " + name)
            _check_all(st, "on " + name)("second un-stalled pass")
            _, end = run_window(T, stall, stream, st, stall_for(host_ms), what="on " + name, sync=False)
            assert not end.query(), "the host is not ahead of %s when it asks for the switch" % name
            pending = (name, stream, st, end)
        pending[1].synchronize()
        _check_all(pending[2], "on " + pending[0])("stalled")
    finally:
        T.cuda.synchronize()
        _unload(g2)
        _unload(g1)
        ctx2.close()
        ctx1.close()

"""mdb_get_stats: the four fields of mdb_stats after every search form, every way to call, under tombstones and filters, after the
shard entries, after sequences of calls on one context and after calls that do no search; and mdb_set_profiling / mdb_get_profile
(-m gpu).

The expected numbers come from tests/stats_model.py — a host model that restates the contract of include/muopdb_hip.h ("mdb_stats:
the contract") from the posting lists, the probe rows, the tombstones, the allow bitmaps and the oracle's graph counters;
tests/test_stats_model.py holds that model to the oracle's own counts.  Every comparison of stats is exact equality of all four
fields, and the rows of the same call are compared with the oracle's, so a form that counts right and answers wrong does not pass.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from muopdb_amd import formats as F
from tests import helpers as H
from tests import stats_model as M
from tests.test_gpu_hnsw_route import GRAPHS
from tests.test_gpu_parity import assert_result_rows, assert_scores

pytestmark = pytest.mark.gpu

K, P, EF = 10, 5, 64
NEXP, EFC, RATIO = 4, 40, 0.1
USERS = (5, 9, 12)
UNKNOWN = 77
INVALID_ARG, ERR_NAN, UNSUPPORTED, OUT_OF_RANGE = 1, 5, 7, 8


@contextlib.contextmanager
def options(ctx, **opts):
    with contextlib.ExitStack() as st:
        for name, val in opts.items():
            st.enter_context(ctx.option(name, val))
        yield


@pytest.fixture(scope="module")
def ctx():
    from muopdb_amd import lib as L
    c = L.Context(0)
    yield c
    c.close()


def vp(x):
    return C.c_void_p(x)


def sz(x):
    return C.c_size_t(x)


# =================================================================================== the world: files, oracle twins, queries (no GPU)
def _near(v, b, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    return (v[rng.integers(0, len(v), b)] + rng.normal(0, sigma, (b, v.shape[1]))).astype(np.float32)


def _ivf_world(oracle, pq, lists=20):
    """3 000 points in 20 lists: f32 rows of dimension 32, or 8-bit PQ codes of 16 subvectors of 4 (dimension 64).  lists = 1024: rows
    around given centroids, as tests/test_gpu_instantiations.py builds the coarse quantizer that the matrix-core coarse search serves
    (cm_build: 1 024 .. 16 384 centroids of dimension 64 / 96 / 128 / 192 / 256)"""
    n, d = 3000, 64 if pq else 32
    if lists <= 64:
        v = H.sift_like(n, d, n_clusters=20, seed=11 + pq)
        cent = H.kmeans(v, lists, iters=3, seed=4)
    else:
        rng = np.random.default_rng(lists)
        cent = H.sift_like(lists, d, n_clusters=32, seed=13)
        v = (cent[rng.integers(0, lists, n)] + rng.normal(0, 3.0, (n, d))).astype(np.float32)
    docs = [100 + 3 * i for i in range(n)]
    w = dict(n=n, d=d, pq=pq, docs=docs, v=v, q=_near(v, 8, 5))
    if pq:
        w["cb"] = H.train_pq_codebook(v[:1500], 4, 8, iters=2)
        w["index"], w["vec"], w["pls"] = H.build_ivf_files(v, docs, cent, quantize=oracle.ProductQuantizer(d, 4, 8, w["cb"]).quantize)
        w["row"] = dict(m=d // 4)
    else:
        w["index"], w["vec"], w["pls"] = H.build_ivf_files(v, docs, cent)
        w["row"] = dict(d=d)
    w["o"] = _ivf_oracle(oracle, w)
    w["nearest"] = w["o"].find_nearest_centroids(w["q"], P)
    # the longest list that query 0 probes, named three times in every row
    w["longest"] = max((int(c) for c in w["nearest"][0]), key=lambda c: len(w["pls"][c]))
    thrice = np.concatenate([w["nearest"], np.full((8, 2), w["longest"], np.uint32)], 1)
    thrice[:, 0] = w["longest"]
    w["thrice"] = np.ascontiguousarray(thrice[:, [0, 5, 1, 2, 6, 3, 4]])
    # its nearest point per query: tombstoned in the `dead` twins
    one = np.full((8, 1), w["longest"], np.uint32)
    first = w["o"].search(w["q"], 1, probes=one)
    w["dead_docs"] = sorted({first.doc_ids(i)[0] for i in range(8)})
    w["dead"] = [docs.index(doc) for doc in w["dead_docs"]]
    w["o_dead"] = _ivf_oracle(oracle, w)
    for doc in w["dead_docs"]:
        assert w["o_dead"].invalidate(doc)
    rng = np.random.default_rng(6)
    from muopdb_amd.index import allow_bitmap
    w["bm_shared"] = allow_bitmap(np.arange(0, n, 2), n)
    w["bm_each"] = np.stack([allow_bitmap(np.sort(rng.choice(n, n // 2, replace=False)), n) for _ in range(8)])
    w["bm_wide"] = np.concatenate([w["bm_each"], np.zeros((8, 3), np.uint32)], 1)
    return w


def _ivf_oracle(oracle, w):
    quant = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 4, 8, w["cb"]) if w["pq"] else oracle.Quant()
    return oracle.BlockBasedIvf(w["index"], w["vec"], quant)


def _ivf_gpu(ctx, w, dead=False, **kw):
    from muopdb_amd.index import BlockBasedIvf, ProductQuantizer
    g = BlockBasedIvf(ctx, w["index"], w["vec"], ProductQuantizer(w["d"], 4, 8, w["cb"]) if w["pq"] else None, **kw)
    if dead:
        for doc in w["dead_docs"]:
            assert g.invalidate(doc)
    return g


def ring_graph(n, d, upper, seed):
    """a graph of the shapes of tests/test_gpu_hnsw_route.py's GRAPHS: layer 0 a ring with four random long links over n points,
    layer i >= 1 a ring with four random members over the first upper[i - 1] points"""
    rng = np.random.default_rng(seed)
    v = rng.random((n, d), dtype=np.float32)
    ar = np.arange(n)
    nb = np.stack([(ar + 1) % n, (ar - 1) % n] + [rng.integers(0, n, n) for _ in range(4)], 1)
    layers = [(None, np.arange(n + 1, dtype=np.uint64) * 6, nb.reshape(-1).astype(np.uint32))]
    for m in upper:
        pts = np.arange(m)
        unb = np.stack([np.roll(pts, -1), np.roll(pts, 1)] + [pts[rng.integers(0, m, m)] for _ in range(4)], 1)
        layers.append({int(p): [int(x) for x in row] for p, row in zip(pts, unb)})
    q = (v[rng.integers(0, n, 8)] + rng.normal(0, 0.02, (8, d))).astype(np.float32)
    return v, layers, q


def _hnsw_world(oracle, name, integer=False):
    _, n, d, upper, _ = GRAPHS[name]
    v, layers, q = ring_graph(n, d, upper, seed=len(name))
    if integer:    # rows and queries in 0..3: exact distance ties at the frontier form's stop test
        rng = np.random.default_rng(2)
        v, q = rng.integers(0, 4, v.shape).astype(np.float32), rng.integers(0, 4, q.shape).astype(np.float32)
    w = dict(d=d, q=q[:8], pq=name == "pq")
    if w["pq"]:
        w["cb"] = H.train_pq_codebook(v[:1000], 8, 8, iters=2)
        codes = oracle.ProductQuantizer(d, 8, 8, w["cb"], 0).quantize(v)
        w["index"], w["vec"] = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d // 8), F.write_vector_file(codes)
        w["o"] = oracle.BlockBasedHnsw(w["index"], w["vec"], d, oracle.Quant(oracle.QUANT_PQ, 0, 8, 8, w["cb"]))
        w["row"] = dict(m=d // 8)
    else:
        w["index"], w["vec"] = F.write_hnsw_index(layers, np.arange(n, dtype=np.uint64), d), F.write_vector_file(v)
        w["o"] = oracle.BlockBasedHnsw(w["index"], w["vec"], d)
        w["row"] = dict(d=d)
    w["want"] = {}
    return w


def _hnsw_gpu(ctx, w):
    from muopdb_amd.index import BlockBasedHnsw, ProductQuantizer
    return BlockBasedHnsw(ctx, w["index"], w["vec"], w["d"], ProductQuantizer(w["d"], 8, 8, w["cb"], 0) if w["pq"] else None)


def _hnsw_want(w, b, ef):
    """the oracle's rows and the model's stats of ann_search(q[:b], K, ef): computed once, shared, never changed"""
    if (b, ef) not in w["want"]:
        w["o"].stats()
        rows = w["o"].ann_search(w["q"][:b], K, ef)
        w["want"][b, ef] = (rows, M.hnsw(*w["o"].stats(), **w["row"]))
    return w["want"][b, ef]


def _spann_world(oracle, pq):
    """the three users of tests/test_gpu_scratch.py (500, 600, 700 points of dimension 32 in 10 lists each), f32 or 6-bit PQ lists"""
    from muopdb_amd.index import allow_bitmap
    d = 32
    w = dict(d=d, pq=pq, per_user={}, pls={}, graph={}, row=dict(m=8) if pq else dict(d=d))
    pool = H.sift_like(1500, d, n_clusters=20, seed=3)
    quantize = None
    if pq:
        w["cb"] = H.train_pq_codebook(pool, 4, 6, iters=2)
        quantize = oracle.ProductQuantizer(d, 4, 6, w["cb"]).quantize
        w["oquant"] = oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, 4, 6, w["cb"])
    else:
        w["oquant"] = None
    qs = []
    for j, u in enumerate(USERS):
        uv = H.sift_like(500 + 100 * j, d, n_clusters=20, seed=3 + j)
        w["per_user"][u], _, w["pls"][u] = H.build_spann_files(oracle, uv, [1000 * u + i for i in range(len(uv))], 10, quantize=quantize, seed=j,
                                                               max_neighbors=8, max_layers=3, ef_construction=40)
        w["graph"][u] = oracle.BlockBasedHnsw(w["per_user"][u]["hnsw_index"], w["per_user"][u]["hnsw_vectors"], d)
        qs.append(_near(uv, 3, 20 + j, 3.0))
    cat = F.concat_multi_spann(w["per_user"])
    w["margs"] = (cat["user_table"], d, cat["hnsw_index"], cat["hnsw_vectors"], cat["ivf_index"], cat["ivf_vectors"])
    w["oms"] = oracle.MultiSpannIndex(*w["margs"], w["oquant"])
    # a batch that mixes the users and holds one unknown user
    w["users"] = [USERS[0], USERS[1], UNKNOWN, USERS[2], USERS[1], USERS[0], USERS[2]]
    w["q"] = np.stack([qs[0][0], qs[1][0], qs[1][1], qs[2][0], qs[1][2], qs[0][1], qs[2][1]])
    w["bm"] = allow_bitmap(np.arange(0, 700, 2), 700)     # even user-local point ids, shared by the batch
    one = w["per_user"][USERS[0]]
    w["sargs"] = (one["hnsw_index"], one["hnsw_vectors"], one["ivf_index"], one["ivf_vectors"])
    w["ospann"] = oracle.Spann(*w["sargs"], w["oquant"])
    w["osp"] = oracle.SearchParams(K, EFC, num_explored_centroids=NEXP, centroid_distance_ratio=RATIO)
    return w


def _spann_model(w, users, q, allow=None, owned=None, dead=None, part="both"):
    """the centroid graphs' counters of every known user's query + the scan of the lists the ratio filter kept.  dead: user -> its
    tombstoned point ids; part: "graph" (the probes-only call) or "scan" (the call that is handed the probes) count one half"""
    m = {"m": w["row"]["m"]} if w["pq"] else {}
    total = M.spann(0, 0, 0, w["d"], **m)
    for i, u in enumerate(users):
        if u not in w["graph"]:
            continue
        g = w["graph"][u]
        g.stats()
        rows = g.ann_search(q[i:i + 1], NEXP, EFC)
        evals, expanded = g.stats()
        kept = M.ratio_filter(rows.doc_ids(0), rows.scores[0, :int(rows.counts[0])], RATIO)
        scored = M.ivf_scored(w["pls"][u], [kept], (dead or {}).get(u, ()), allow, owned)
        if part == "graph":
            scored = 0
        if part == "scan":
            evals = expanded = 0
        total = M.add(total, M.spann(evals, expanded, scored, w["d"], **m))
    return total


def _spann_params():
    from muopdb_amd.index import SearchParams
    return SearchParams(K, EFC).with_num_explored_centroids(NEXP).with_centroid_distance_ratio(RATIO)


def _spann_gpu(ctx, w, **kw):
    from muopdb_amd.index import MultiSpannIndex, ProductQuantizer
    return MultiSpannIndex(ctx, *w["margs"], ProductQuantizer(w["d"], 4, 6, w["cb"]) if w["pq"] else None, **kw)


FLAT_SHAPES = {"small": (777, 30, 5, 3), "one-query": (4100, 96, 1, 1), "batched": (65536, 16, 8, 3)}   # 65 536 = 1 024 tiles: the least the batched path takes


@pytest.fixture(scope="module")
def world(oracle):
    w = dict(flat={}, ivf={False: _ivf_world(oracle, False), True: _ivf_world(oracle, True), "cm": _ivf_world(oracle, True, lists=1024)},
             hnsw={name: _hnsw_world(oracle, name) for name in GRAPHS}, spann={False: _spann_world(oracle, False), True: _spann_world(oracle, True)})
    w["hnsw"]["integer"] = _hnsw_world(oracle, "three-layers", integer=True)
    for name, (n, d, b, k) in FLAT_SHAPES.items():
        base = H.sift_like(n, d, n_clusters=20, seed=n)
        q = _near(base, b, 9, 5.0)
        w["flat"][name] = dict(base=base, q=q, k=k, want=oracle.flat_topk(0, base, q, k), model=M.flat(n, d, b, k))
    return w


@pytest.fixture(scope="module")
def loaded(ctx, world):
    """the world's GPU handles on the module's context"""
    from muopdb_amd.index import FlatIndex
    g = dict(flat={name: FlatIndex(ctx, f["base"]) for name, f in world["flat"].items()},
             ivf={pq: _ivf_gpu(ctx, w) for pq, w in world["ivf"].items()}, ivf_dead={pq: _ivf_gpu(ctx, w, dead=True) for pq, w in world["ivf"].items()},
             hnsw={name: _hnsw_gpu(ctx, w) for name, w in world["hnsw"].items()}, spann={pq: _spann_gpu(ctx, w) for pq, w in world["spann"].items()})
    yield g
    for fam in g.values():
        for h in fam.values():
            h.close()


def assert_flat_rows(got, want):
    ids, dist, _ = got
    assert np.array_equal(ids, want[0])
    assert_scores(dist, want[1])


def assert_stats(ctx, model, what=""):
    st = ctx.stats()
    assert st == model, "%s: mdb_get_stats gives %r, the model %r" % (what, st, model)
    assert ctx.stats() == st, "%s: a second read differs" % what


# =================================================================================== a. every form
@pytest.mark.parametrize("shape", list(FLAT_SHAPES))
def test_flat_forms(ctx, world, loaded, shape):
    """`batched`: 65 536 rows are the fewest for which flat_build_aux builds the sample, and b = 8, k = 3 pass every other condition of
    flat_mfma_applicable — but for its cooldown: after a batch whose candidate lists overflowed it sends MDB_MF_COOLDOWN calls to the
    exact kernels.  With the option at 0 it never does, so every MDB_FLAT_NO_MFMA = 0 call here takes the batched path."""
    f, g = world["flat"][shape], loaded["flat"][shape]
    for no_mfma in (0, 1):
        for no_small in (0, 1, 2, 4):
            with options(ctx, MDB_FLAT_NO_MFMA=no_mfma, MDB_FLAT_NO_SMALL=no_small, MDB_MF_COOLDOWN=0):
                assert_flat_rows(g.search(f["q"], f["k"]), f["want"])
                assert_stats(ctx, f["model"], "%s no_mfma=%d no_small=%d" % (shape, no_mfma, no_small))


F32_FORMS = [dict(MDB_SCAN_F32_BLK=blk, MDB_SCAN_F32_NSPLIT=ns, MDB_SCAN_MASKS_ALWAYS=ma) for blk in (64, 128, 0) for ns in (0, 2) for ma in (0, 1)]
PQ3 = dict(MDB_PQ_NO_FUSED=1, MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1)
# name -> (options, batch): IvfSet::fused_ok takes batches below MDB_PQ_TWO_PHASE_MIN_B (512) with k and probes up to 64 — 4 queries here;
# the others run the six-launch step (coarse search, query codes, scan, merge, remap) around the scan the options select
PQ_FORMS = {
    "fused": (dict(), 4),
    "six-launch-pq2-bound-filter": (dict(MDB_PQ_NO_FUSED=1), 8), "pq2-no-bound-filter": (dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FILTER=1), 8),
    "pq2-no-full": (dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FULL=1), 8), "lut-scan": (dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FAST=1), 8),
    "two-phase": (PQ3, 8), "two-phase-no-full": (dict(PQ3, MDB_PQ_NO_FULL=1), 8), "two-phase-switched-off": (dict(PQ3, MDB_PQ_NO_TWO_PHASE=1), 8),
}
# The fused step's coarse search on the matrix cores (coarse_mode 2 in IvfSet::search_fused) needs cm_usable(): an index of 1 024 ..
# 16 384 lists (the "cm" world) and a batch of at least MDB_IVF_COARSE_MFMA_MIN_B (32: lowered to 1, as tests/test_gpu_instantiations.py
# does).  MDB_CM_SPLIT is read in that mode only; MDB_IVF_COARSE_MFMA = 0 sends the same index through ivf_prep_kernel's exact distances.
CM_FORMS = {"fused-coarse-mfma": dict(MDB_IVF_COARSE_MFMA_MIN_B=1), "fused-coarse-mfma-cm-split": dict(MDB_IVF_COARSE_MFMA_MIN_B=1, MDB_CM_SPLIT=1),
            "fused-coarse-exact": dict(MDB_IVF_COARSE_MFMA_MIN_B=1, MDB_IVF_COARSE_MFMA=0)}
IVF_FORMS = [("f32-" + "-".join("%s%d" % (k.split("_")[-1].lower(), v) for k, v in o.items()), False, o, 8) for o in F32_FORMS] + \
            [("pq-" + name, True, o, b) for name, (o, b) in PQ_FORMS.items()] + \
            [("pq-1024-lists-" + name, "cm", o, 8) for name, o in CM_FORMS.items()]


def _ivf_cases(w, b):
    """(name, probe table or None, tombstones, allow bitmaps): plain, then the three of section c, separately and combined"""
    return [("plain", None, False, None), ("tombstones", None, True, None), ("shared-bitmap", None, False, w["bm_shared"]),
            ("bitmap-per-query", None, False, w["bm_each"][:b]), ("list-named-thrice", w["thrice"][:b], False, None),
            ("all-three", w["thrice"][:b], True, w["bm_each"][:b])]


def _ivf_expect(oracle, w, b, k, probes, dead, allow):
    o = w["o_dead"] if dead else w["o"]
    p = w["nearest"][:b] if probes is None else probes
    with oracle.planner_filter(allow) if allow is not None else contextlib.nullcontext():
        rows = o.search(w["q"][:b], k, probes=p)
    return rows, M.ivf(w["pls"], p, dead=w["dead"] if dead else (), allow=allow, **w["row"])


@pytest.mark.parametrize("name,pq,opts,b", IVF_FORMS, ids=[f[0] for f in IVF_FORMS])
def test_ivf_forms_tombstones_filters_and_repeated_lists(ctx, oracle, world, loaded, name, pq, opts, b):
    w = world["ivf"][pq]
    q = w["q"][:b]
    plain = None
    with options(ctx, **opts):
        for case, probes, dead, allow in _ivf_cases(w, b):
            g = loaded["ivf_dead" if dead else "ivf"][pq]
            rows, model = _ivf_expect(oracle, w, b, K, probes, dead, allow)
            got = g.search(q, K, P, planner=allow) if probes is None else g.search_with_centroids_and_remap(q, probes, K, planner=allow)
            assert_stats(ctx, model, "%s, %s" % (name, case))
            assert_result_rows(got, rows, b)
            plain = plain or model
            # each case must move the count, or it checks nothing
            assert (model["scored_vectors"] < plain["scored_vectors"]) if case in ("tombstones", "shared-bitmap", "bitmap-per-query") else True, case
            assert (model["scored_vectors"] > plain["scored_vectors"]) if case == "list-named-thrice" else True, case


HNSW_SWITCHES = ("MDB_HNSW_NO_BEAM", "MDB_HNSW_NO_TABLE", "MDB_HNSW_NO_WIDE", "MDB_HNSW_NO_CLOSURE", "MDB_HNSW_CLOSURE")


@pytest.mark.parametrize("name", list(GRAPHS) + ["integer"])
def test_hnsw_forms(ctx, world, loaded, name):
    w, g = world["hnsw"][name], loaded["hnsw"][name]
    fallbacks, routes = 0, set()
    for ef in (64, 300, 600):
        for b in (1, 8):
            rows, model = _hnsw_want(w, b, ef)
            for switch in (None,) + HNSW_SWITCHES:
                for val in ((None,) if switch is None else (0, 1)):
                    with options(ctx, **({switch: val} if switch else {})):
                        routes.add(tuple(role for role, *_ in g.describe_search(b, K, ef)[1]))
                        got = g.ann_search(w["q"][:b], K, ef)
                        assert_stats(ctx, model, "%s ef=%d b=%d %s=%s" % (name, ef, b, switch, val))
                        fallbacks += ctx.closure_fallbacks()
                        assert_result_rows(got, rows, b)
    assert len(routes) > 1 or name in ("pq", "no-larger-than-ef"), routes
    if name == "integer":
        assert fallbacks > 0, "no query took the frontier form's tie fallback: the case no longer shows that mdb_stats does not depend on it"


def _spann_search(g, w, planner=None):
    return g.search_for_user(w["users"], w["q"], _spann_params(), planner=planner)


def _spann_want(oracle, w, allow=None):
    with oracle.planner_filter(allow) if allow is not None else contextlib.nullcontext():
        return w["oms"].search_for_user(w["users"], w["q"], w["osp"])


class Dev:
    """device buffers of one call; torch fills them on its own stream, so everything is finished before the context's call"""

    def __init__(self, q, k, flat=False):
        import torch
        self.b, self.k, self.flat = len(q), k, flat
        dev = torch.device("cuda", torch.cuda.current_device())
        self.q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
        self.ids = torch.zeros((self.b, k) if flat else (self.b, k, 2), dtype=torch.int32 if flat else torch.int64, device=dev)
        self.sc = torch.zeros((self.b, k), dtype=torch.float32, device=dev)
        self.cn = torch.zeros(self.b, dtype=torch.int32, device=dev)
        self.fo = torch.zeros(self.b, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def outs(self):
        return [vp(self.ids.data_ptr()), vp(self.sc.data_ptr()), vp(self.cn.data_ptr())]

    def result(self):
        """after mdb_sync"""
        from muopdb_amd.index import SearchResult
        if self.flat:
            return self.ids.cpu().numpy().view(np.uint32), self.sc.cpu().numpy(), self.cn.cpu().numpy()
        h = self.ids.cpu().numpy().view(np.uint64)
        return SearchResult(self.b, self.k, h[:, :, 0], h[:, :, 1], self.sc.cpu().numpy(), self.cn.cpu().numpy().view(np.uint32), self.fo.cpu().numpy())


def _ms_device(ctx, g, users, d):
    """mdb_multi_spann_search in device memory on the buffers `d`; returns at once"""
    from muopdb_amd import lib as L
    pc = _spann_params().to_c()
    ctx.check(ctx.lib.mdb_multi_spann_search(g.h, L.u128_array(list(users)), vp(d.q.data_ptr()), sz(d.b), C.byref(pc), C.c_int(L.MEM_DEVICE), *d.outs(),
                                             vp(d.fo.data_ptr())))


def _spann_device(ctx, g, d):
    from muopdb_amd import lib as L
    pc = _spann_params().to_c()
    ctx.check(ctx.lib.mdb_spann_search(g.h, vp(d.q.data_ptr()), sz(d.b), C.byref(pc), C.c_int(L.MEM_DEVICE), *d.outs(), vp(d.fo.data_ptr())))


@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq"])
def test_multi_spann_forms(ctx, oracle, world, loaded, pq):
    """host calls with and without a shared bitmap, the ratio filter inside the closure kernel and as a launch of its own; device
    calls, where MDB_SCAN_NO_FUSED_REMAP decides between the merge launch that remaps and saves the counters to words 24..27
    (counter_base 24, counters_clean) and a merge followed by a remap launch (counter_base 0) — a host call never reads that switch"""
    w, g = world["spann"][pq], loaded["spann"][pq]
    unknown = w["users"].index(UNKNOWN)
    for allow in (None, w["bm"]):
        rows, model = _spann_want(oracle, w, allow), _spann_model(w, w["users"], w["q"], allow)
        assert model["distance_evals"] > 0 and model["scored_vectors"] > 0 and not rows.found[unknown]
        for no_filter in (0, 1):
            with options(ctx, MDB_CLOSURE_NO_FILTER=no_filter):
                got = _spann_search(g, w, allow)
                assert_stats(ctx, model, "multi-spann pq=%s filter=%s no_filter=%d" % (pq, allow is not None, no_filter))
                assert list(got.found) == list(rows.found)
                assert_result_rows(got, rows, len(w["q"]))
    rows, model = _spann_want(oracle, w), _spann_model(w, w["users"], w["q"])
    for no_filter in (0, 1):
        for no_remap in (0, 1, 0):      # (the third call follows one that left the counters un-saved)
            with options(ctx, MDB_CLOSURE_NO_FILTER=no_filter, MDB_SCAN_NO_FUSED_REMAP=no_remap):
                d = Dev(w["q"], K)
                _ms_device(ctx, g, w["users"], d)
                assert_stats(ctx, model, "multi-spann device pq=%s no_filter=%d no_remap=%d" % (pq, no_filter, no_remap))
                ctx.sync()
                got = d.result()
                assert list(got.found) == list(rows.found)
                assert_result_rows(got, rows, len(w["q"]))
    # the unknown user contributes nothing: the batch without it counts the same
    keep = [i for i in range(len(w["users"])) if i != unknown]
    assert _spann_model(w, [w["users"][i] for i in keep], w["q"][keep]) == _spann_model(w, w["users"], w["q"])


def test_single_user_spann(ctx, oracle, world):
    """mdb_spann_search in host and device memory (both values of MDB_SCAN_NO_FUSED_REMAP), and mdb_spann_search_shard, which reports
    the same: a single-user handle holds every list"""
    from muopdb_amd.index import ProductQuantizer, Spann
    for pq, w in world["spann"].items():
        g = Spann(ctx, *w["sargs"], ProductQuantizer(w["d"], 4, 6, w["cb"]) if pq else None)
        users, q = [USERS[0]] * 3, w["q"][[0, 5, 1]]
        rows, model = w["ospann"].search(q, w["osp"]), _spann_model(w, users, q)
        got = g.search(q, _spann_params())
        assert_stats(ctx, model, "spann pq=%s" % pq)
        assert_result_rows(got, rows, 3)
        for no_remap in (0, 1, 0):
            with options(ctx, MDB_SCAN_NO_FUSED_REMAP=no_remap):
                d = Dev(q, K)
                _spann_device(ctx, g, d)
                assert_stats(ctx, model, "spann device pq=%s no_remap=%d" % (pq, no_remap))
                ctx.sync()
                assert_result_rows(d.result(), rows, 3)
        g.search_shard(q, _spann_params())
        assert_stats(ctx, model, "spann search_shard pq=%s" % pq)
        g.close()


@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq"])
def test_multi_spann_tombstones(ctx, oracle, world, pq):
    """the nearest point of every known user's query, invalidated on both sides: a tombstoned entry is not scored"""
    w = world["spann"][pq]
    g, o = _spann_gpu(ctx, w), oracle.MultiSpannIndex(*w["margs"], w["oquant"])
    first = o.search_for_user(w["users"], w["q"], w["osp"])
    dead = {}
    for i, u in enumerate(w["users"]):
        if first.found[i]:
            doc = first.doc_ids(i)[0]
            if doc - 1000 * u not in dead.setdefault(u, set()):
                assert g.invalidate(u, doc) and o.invalidate(u, doc)
                dead[u].add(doc - 1000 * u)        # doc id = 1000 * user + point id
    rows = o.search_for_user(w["users"], w["q"], w["osp"])
    model = _spann_model(w, w["users"], w["q"], dead=dead)
    assert model["scored_vectors"] < _spann_model(w, w["users"], w["q"])["scored_vectors"]
    got = _spann_search(g, w)
    assert_stats(ctx, model, "multi-spann with tombstones pq=%s" % pq)
    assert_result_rows(got, rows, len(w["q"]))
    d = Dev(w["q"], K)
    _ms_device(ctx, g, w["users"], d)
    assert_stats(ctx, model, "multi-spann device with tombstones pq=%s" % pq)
    ctx.sync()
    assert_result_rows(d.result(), rows, len(w["q"]))
    g.close()


@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq"])
def test_multi_spann_probe_halves(ctx, oracle, world, loaded, pq):
    """mdb_multi_spann_probes is the centroid stage alone: the graph counters, nothing scored; mdb_multi_spann_search_shard_probes is
    handed those rows and scans: the scored entries, no graph counters.  The two add up to the whole call."""
    w, g = world["spann"][pq], loaded["spann"][pq]
    graph, scan = _spann_model(w, w["users"], w["q"], part="graph"), _spann_model(w, w["users"], w["q"], part="scan")
    assert M.add(graph, scan) == _spann_model(w, w["users"], w["q"]) and graph["scored_vectors"] == 0 == scan["distance_evals"]
    rows = g.probes(w["users"], w["q"], _spann_params())
    assert_stats(ctx, graph, "mdb_multi_spann_probes pq=%s" % pq)
    blk = g.search_shard_probes(w["users"], w["q"], _spann_params(), rows)
    assert_stats(ctx, scan, "mdb_multi_spann_search_shard_probes pq=%s" % pq)
    assert np.array_equal(blk, g.search_shard(w["users"], w["q"], _spann_params()))


# =================================================================================== b. every way to call
class Call:
    """one search call of a family, made in host memory, in device memory or through submit + wait, with the oracle's rows and the
    model's stats.  load(ctx) gives the handle on any context."""

    def __init__(self, name, load, host, device, submit, check, model, k=K, flat=False):
        self.name, self.load, self.host, self.device, self.submit, self.check, self.model, self.k, self.flat = \
            name, load, host, device, submit, check, model, k, flat


def _calls(oracle, world):
    from muopdb_amd import lib as L
    from muopdb_amd.index import FlatIndex, ProductQuantizer, Spann
    calls = {}
    # ---- flat
    f = world["flat"]["small"]
    calls["flat"] = Call("flat", lambda c: FlatIndex(c, f["base"]), lambda g: g.search(f["q"], f["k"]),
                         lambda c, g, d: g.search_device(d.q.data_ptr(), d.b, f["k"], d.ids.data_ptr(), d.sc.data_ptr(), d.cn.data_ptr()),
                         None, lambda r: assert_flat_rows(r, f["want"]), f["model"], k=f["k"], flat=True)
    calls["flat"].q = f["q"]
    # ---- IVF f32 (coarse search + scan) and IVF-PQ (the fused step at batch 4)
    for name, pq, b in (("ivf-f32", False, 8), ("ivf-pq-fused", True, 4)):
        w = world["ivf"][pq]
        rows, model = _ivf_expect(oracle, w, b, K, None, False, None)

        def device(c, g, d, b=b):
            c.check(c.lib.mdb_ivf_search(g.h, vp(d.q.data_ptr()), sz(b), None, sz(P), sz(K), C.c_int(L.MEM_DEVICE), *d.outs()))
        calls[name] = Call(name, lambda c, w=w: _ivf_gpu(c, w), lambda g, w=w, b=b: g.search(w["q"][:b], K, P), device,
                           lambda g, w=w, b=b: g.search_submit(w["q"][:b], K, P).wait(), lambda r, rows=rows, b=b: assert_result_rows(r, rows, b), model)
        calls[name].q = w["q"][:b]
    # ---- HNSW over f32 rows and over PQ codes
    for name, graph in (("hnsw-f32", "three-layers"), ("hnsw-pq", "pq")):
        w = world["hnsw"][graph]
        rows, model = _hnsw_want(w, 8, EF)
        calls[name] = Call(name, lambda c, w=w: _hnsw_gpu(c, w), lambda g, w=w: g.ann_search(w["q"], K, EF),
                           lambda c, g, d: g.ann_search_device(d.q.data_ptr(), d.b, K, EF, d.ids.data_ptr(), d.sc.data_ptr(), d.cn.data_ptr()),
                           lambda g, w=w: g.ann_search_submit(w["q"], K, EF).wait(), lambda r, rows=rows: assert_result_rows(r, rows, 8), model)
        calls[name].q = w["q"]
    # ---- SPANN (one user) and multi-user SPANN
    w = world["spann"][False]
    sq = w["q"][[0, 5, 1, 4]]
    srows, smodel = w["ospann"].search(sq, w["osp"]), _spann_model(w, [USERS[0]] * 4, sq)
    calls["spann"] = Call("spann", lambda c: Spann(c, *w["sargs"]), lambda g: g.search(sq, _spann_params()), _spann_device,
                          lambda g: g.search_submit(sq, _spann_params()).wait(), lambda r: assert_result_rows(r, srows, 4), smodel)
    calls["spann"].q = sq
    mrows, mmodel = _spann_want(oracle, w), _spann_model(w, w["users"], w["q"])
    calls["multi-spann"] = Call("multi-spann", lambda c: _spann_gpu(c, w), lambda g: _spann_search(g, w), lambda c, g, d: _ms_device(c, g, w["users"], d),
                                lambda g: g.search_for_user_submit(w["users"], w["q"], _spann_params()).wait(),
                                lambda r: assert_result_rows(r, mrows, len(w["q"])), mmodel)
    calls["multi-spann"].q = w["q"]
    return calls


@pytest.fixture(scope="module")
def calls(oracle, world):
    return _calls(oracle, world)


def run_device(ctx, call, g, sync_first=False):
    """the call in device memory; stats read before mdb_sync (mdb_get_stats waits itself) or behind it; -> (stats, result)"""
    d = Dev(call.q, call.k, call.flat)
    call.device(ctx, g, d)
    if sync_first:
        ctx.sync()
    st = ctx.stats()
    ctx.sync()
    return st, d.result()


@pytest.mark.parametrize("name", ["flat", "ivf-f32", "ivf-pq-fused", "hnsw-f32", "hnsw-pq", "spann", "multi-spann"])
def test_every_way_to_call_reports_the_same(ctx, calls, name):
    call = calls[name]
    g = call.load(ctx)
    try:
        call.check(call.host(g))
        assert_stats(ctx, call.model, name + " host")
        for sync_first in (False, True):
            st, res = run_device(ctx, call, g, sync_first)
            assert st == call.model, "%s device, stats %s mdb_sync: %r, the model %r" % (name, "behind" if sync_first else "before", st, call.model)
            assert ctx.stats() == st
            call.check(res)
        if call.submit:
            call.check(call.submit(g))
            assert_stats(ctx, call.model, name + " submit + wait")
    finally:
        g.close()


@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq-fused"])
def test_ivf_entry_points(ctx, oracle, world, loaded, pq):
    """mdb_ivf_search, _search_points and _search_filtered (one shared bitmap, one per query, words_per_bitmap larger than needed),
    with the coarse search inside and with the probes given"""
    w, g, b = world["ivf"][pq], loaded["ivf"][pq], 4
    q = w["q"][:b]
    for probes in (None, w["thrice"][:b]):
        rows, model = _ivf_expect(oracle, w, b, K, probes, False, None)
        ids, sc, cn = g.search_points(q, K, P, probes=probes)
        assert_stats(ctx, model, "search_points")
        assert [int(c) for c in cn] == [int(c) for c in rows.counts[:b]]
        for i in range(b):    # (ordered by point id among equal distances, the remapped rows by doc id: compared as sets of score bits)
            assert sorted(np.asarray(sc[i, :int(cn[i])], np.float32).view(np.uint32)) == sorted(np.asarray(rows.scores[i, :int(cn[i])], np.float32).view(np.uint32))
        for allow in (w["bm_shared"], w["bm_each"][:b], w["bm_wide"][:b]):
            rows, model = _ivf_expect(oracle, w, b, K, probes, False, allow if allow.ndim == 1 else allow[:, :w["bm_each"].shape[1]])
            got = g.search(q, K, P, planner=allow) if probes is None else g.search_with_centroids_and_remap(q, probes, K, planner=allow)
            assert_stats(ctx, model, "search_filtered %r" % (allow.shape,))
            assert_result_rows(got, rows, b)
    # mdb_ivf_find_nearest_centroids is no search call: the stats stay
    before = ctx.stats()
    assert np.array_equal(g.find_nearest_centroids(q, P), w["nearest"][:b])
    assert ctx.stats() == before


# =================================================================================== d. shards
@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq"])
def test_ivf_shards_add_up(ctx, oracle, world, loaded, pq):
    pytest.importorskip("torch")
    w, b = world["ivf"][pq], 4
    q = w["q"][:b]
    for probes in (None, w["thrice"][:b]):
        rows, whole = _ivf_expect(oracle, w, b, K, probes, False, None)
        p = w["nearest"][:b] if probes is None else probes
        for shard_world in (1, 2, 3):
            shards = [_ivf_gpu(ctx, w, shard_rank=r, shard_world=shard_world) for r in range(shard_world)]
            owner = M.balanced_owner([len(pl) for pl in w["pls"]], shard_world)       # one index: size-balanced ownership
            blocks, scored = [], 0
            for r, s in enumerate(shards):
                blocks.append(s.search_shard(q, K, probes=p))
                # this rank's share: the entries of the lists it holds, and nothing counted on the wrong rank
                assert_stats(ctx, M.ivf(w["pls"], p, owned={c for c, o_ in enumerate(owner) if o_ == r}, **w["row"]), "rank %d of %d" % (r, shard_world))
                scored += ctx.stats()["scored_vectors"]
            assert scored == whole["scored_vectors"], (shard_world, scored, whole)
            last = ctx.stats()
            merged = shards[0].merge_shards(blocks, b, K)
            assert ctx.stats() == last, "mdb_ivf_merge_shards changed the stats"
            assert_result_rows(merged, rows, b)
            for s in shards:
                s.close()


@pytest.mark.parametrize("pq", [False, True], ids=["f32", "pq"])
def test_multi_spann_shards_add_up(ctx, oracle, world, pq):
    pytest.importorskip("torch")
    w = world["spann"][pq]
    rows, whole = _spann_want(oracle, w), _spann_model(w, w["users"], w["q"])
    for shard_world in (1, 2, 3):
        shards = [_spann_gpu(ctx, w, shard_rank=r, shard_world=shard_world) for r in range(shard_world)]
        blocks, scored = [], 0
        for r, s in enumerate(shards):
            blocks.append(s.search_shard(w["users"], w["q"], _spann_params()))
            # the centroid graphs are replicated: every rank traverses all of them, and scans list c of every user where c % world == rank
            mine = _spann_model(w, w["users"], w["q"], owned={c for c in range(10) if M.modulo_owner(10, shard_world)[c] == r})
            assert (mine["distance_evals"], mine["expanded_nodes"]) == (whole["distance_evals"], whole["expanded_nodes"])
            assert_stats(ctx, mine, "rank %d of %d" % (r, shard_world))
            scored += mine["scored_vectors"]
        assert scored == whole["scored_vectors"], (shard_world, scored, whole)
        last = ctx.stats()
        merged = shards[0].merge_shards(w["users"], blocks, len(w["q"]), K)
        assert ctx.stats() == last, "mdb_multi_spann_merge_shards changed the stats"
        assert_result_rows(merged, rows, len(w["q"]))
        for s in shards:
            s.close()


# =================================================================================== e. sequences on one context
SEQ = ("flat", "ivf-f32", "ivf-pq-fused", "hnsw-f32", "hnsw-pq", "spann")
# kind -> (call, options).  In device memory a SPANN call's merge launch remaps and saves the counters to words 24..27 (the next call
# finds the others clean); with MDB_SCAN_NO_FUSED_REMAP it merges and remaps in two launches and leaves them where they were counted.
# A host call reads no such switch: there the seventh kind repeats the sixth.
KINDS = dict({n: (n, {}) for n in SEQ}, **{"spann-remap-apart": ("spann", dict(MDB_SCAN_NO_FUSED_REMAP=1))})


@pytest.mark.parametrize("mode", ["host", "device"])
def test_stats_after_a_then_b_are_bs(calls, mode):
    """every ordered pair (A, B), the pair (A, A) included: behind A-then-B one context reports what B reports alone on a fresh
    context — the model's numbers.  One context serves all 49 pairs in a row, so every call is also the A of the next pair."""
    from muopdb_amd import lib as L
    ctx = L.Context(0)
    handles = {n: calls[n].load(ctx) for n in SEQ}

    def run(kind):
        n, opts = KINDS[kind]
        with options(ctx, **opts):
            if mode == "host":
                calls[n].check(calls[n].host(handles[n]))
                return ctx.stats()
            st, res = run_device(ctx, calls[n], handles[n])
            calls[n].check(res)
            return st
    try:
        for n in SEQ:    # B alone on a fresh context
            fresh = L.Context(0)
            g = calls[n].load(fresh)
            if mode == "host":
                calls[n].check(calls[n].host(g))
                alone = fresh.stats()
            else:
                alone, res = run_device(fresh, calls[n], g)
                calls[n].check(res)
            g.close()
            fresh.close()
            assert alone == calls[n].model, (n, alone, calls[n].model)
        for a in KINDS:
            for b_ in KINDS:
                run(a)
                st, alone = run(b_), calls[KINDS[b_][0]].model
                assert st == alone, "%s then %s (%s): mdb_get_stats gives %r, %s alone %r" % (a, b_, mode, st, b_, alone)
    finally:
        for h in handles.values():
            h.close()
        ctx.close()


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("read_each", [True, False], ids=["read-after-each", "read-after-the-last"])
def test_consecutive_fused_calls_use_both_counter_sets(oracle, world, mode, read_each):
    """three and four fused IVF-PQ calls with other probe counts on a fresh context: the step's two counter sets are used and reused"""
    from muopdb_amd import lib as L
    w = world["ivf"][True]
    for probe_counts in ((5, 2, 7), (3, 6, 1, 4)):
        ctx = L.Context(0)
        g = _ivf_gpu(ctx, w)
        try:
            for j, p in enumerate(probe_counts):
                q = w["q"][j:j + 4]
                probes = w["o"].find_nearest_centroids(q, p)
                rows, model = w["o"].search(q, K, probes=probes), M.ivf(w["pls"], probes, **w["row"])
                if mode == "host":
                    got = g.search(q, K, p)
                else:
                    d = Dev(q, K)
                    ctx.check(ctx.lib.mdb_ivf_search(g.h, vp(d.q.data_ptr()), sz(4), None, sz(p), sz(K), C.c_int(L.MEM_DEVICE), *d.outs()))
                    ctx.sync()
                    got = d.result()
                assert_result_rows(got, rows, 4)
                if read_each or j == len(probe_counts) - 1:
                    assert_stats(ctx, model, "fused call %d of %r" % (j, probe_counts))
        finally:
            g.close()
            ctx.close()


# =================================================================================== f. calls that do no search
def test_calls_that_do_no_search_leave_the_last_calls_stats(ctx, oracle, world, loaded, calls):
    """b == 0 and calls refused on the host leave the stats of the call before them — made on another kind of index each time, so
    per-unit sizes of the refused call under the counters of the last one would show"""
    from muopdb_amd import lib as L
    from muopdb_amd.index import SearchParams
    wi, wh, ws = world["ivf"][False], world["hnsw"]["three-layers"], world["spann"][False]
    gi, gh, gf, gs = loaded["ivf"][False], loaded["hnsw"]["three-layers"], loaded["flat"]["small"], loaded["spann"][False]
    fl = world["flat"]["small"]
    empty = {n: np.zeros((0, d), np.float32) for n, d in (("ivf", wi["d"]), ("hnsw", wh["d"]), ("flat", fl["base"].shape[1]), ("spann", ws["d"]))}
    big = SearchParams(K, 2 * 2048 + 1).with_num_explored_centroids(NEXP)
    idle = {
        "ivf": [lambda: gi.search(empty["ivf"], K, P), lambda: gi.search(wi["q"], 2049, P), lambda: gi.search(wi["q"], K, 21),
                lambda: gi.search(wi["q"], K, P, planner=wi["bm_each"][:3])],
        "hnsw": [lambda: gh.ann_search(empty["hnsw"], K, EF), lambda: gh.ann_search(wh["q"], 2049, EF), lambda: gh.ann_search(wh["q"], K, 4097)],
        "flat": [lambda: gf.search(empty["flat"], 3), lambda: gf.search(fl["q"], 2049)],
        "spann": [lambda: gs.search_for_user([], empty["spann"], _spann_params()),
                  lambda: gs.search_for_user(ws["users"], ws["q"], SearchParams(2049, EFC)), lambda: gs.search_for_user(ws["users"], ws["q"], big)],
    }
    last = {"ivf": ("ivf-f32", lambda: gi.search(wi["q"], K, P)), "hnsw": ("hnsw-f32", lambda: gh.ann_search(wh["q"], K, EF)),
            "flat": ("flat", lambda: gf.search(fl["q"], fl["k"])), "spann": ("multi-spann", lambda: _spann_search(gs, ws))}
    for before, (model_of, search) in last.items():
        for fam, attempts in idle.items():
            for j, attempt in enumerate(attempts):
                search()
                want = ctx.stats()
                assert want == calls[model_of].model
                try:
                    attempt()
                    assert j == 0, "%s attempt %d was not refused" % (fam, j)      # b == 0 returns MDB_OK
                except L.MuopdbError as e:
                    assert j > 0 and e.status in (UNSUPPORTED, OUT_OF_RANGE, INVALID_ARG), (fam, j, e)   # (21 probes of 20 lists; 3 bitmaps for 8 queries)
                assert ctx.stats() == want, "%s, then %s attempt %d: the stats changed to %r" % (before, fam, j, ctx.stats())


def test_k_zero_is_a_search(ctx, oracle, world, loaded):
    w, g = world["ivf"][False], loaded["ivf"][False]
    got = g.search(w["q"], 0, P)
    assert_stats(ctx, M.ivf(w["pls"], w["nearest"], **w["row"]), "IVF f32, k = 0")
    assert not got.counts.any()


def test_a_call_that_meets_a_nan_reports_its_own_stats(ctx, oracle, world, loaded):
    """MDB_ERR_NAN is decided on the device: the call ran to its end, and every entry it scanned is counted"""
    from muopdb_amd import lib as L
    from muopdb_amd.index import BlockBasedIvf
    w = world["ivf"][False]
    bad = w["v"].copy()
    bad[int(w["pls"][w["longest"]][0]), 3] = np.nan        # a row of a list that query 0 probes
    g = BlockBasedIvf(ctx, w["index"], F.write_vector_file(bad))
    loaded["hnsw"]["two-layers"].ann_search(world["hnsw"]["two-layers"]["q"], K, EF)      # another family's stats in front
    with pytest.raises(L.MuopdbError) as e:
        g.search(w["q"], K, P)
    assert e.value.status == ERR_NAN
    assert_stats(ctx, M.ivf(w["pls"], w["nearest"], **w["row"]), "IVF f32 with a NaN row")
    g.close()


# =================================================================================== 3. mdb_set_profiling / mdb_get_profile
@pytest.mark.parametrize("mask", [1, 2, 3])
def test_profiling_brackets_by_mask_and_changes_nothing(ctx, calls, mask):
    import math
    scans, graphs = ("ivf-f32", "flat"), ("hnsw-f32",)
    handles = {n: calls[n].load(ctx) for n in scans + graphs}
    try:
        for n, h in handles.items():
            calls[n].check(calls[n].host(h))
            assert ctx.stats() == calls[n].model
        ctx.set_profiling(mask)
        try:
            assert ctx.get_profile() == (0.0, 0)
            for n, h in handles.items():
                calls[n].check(calls[n].host(h))               # rows with profiling on
                assert ctx.stats() == calls[n].model           # all four stats with profiling on
                ms, launches = ctx.get_profile()
                bracketed = bool(mask & (1 if n in scans else 2))
                assert (launches >= 1) if bracketed else (launches == 0), (n, mask, launches)
                if launches:
                    assert math.isfinite(ms) and ms > 0, (n, mask, ms)
                else:
                    assert ms == 0
                assert ctx.get_profile() == (0.0, 0), "a second mdb_get_profile must report nothing"
        finally:
            ctx.set_profiling(0)
        handles["ivf-f32"].search(calls["ivf-f32"].q, K, P)
        assert ctx.get_profile() == (0.0, 0)
    finally:
        for h in handles.values():
            h.close()

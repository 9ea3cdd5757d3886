"""Caller-given IVF probe tables in every scan form (-m gpu).

mdb_ivf_search, _search_points, _search_filtered, _search_submit and _search_shard take a probe table from the caller
(probes != NULL, [b][num_probes]): the reference's search_with_centroids_and_remap over any Vec<usize>
(rs/index/src/ivf/block_based/index.rs:250-286).  The columns are scanned in the order given, a list named m times is scanned m
times and offers each of its points m times (no dedup), and a list id >= num_clusters is Err("Index out of bound")
(storage.rs:280-286) — here MDB_ERR_FORMAT for the call.  List-sharded multi-GPU search feeds such tables (merged coarse keys,
another process's rows), and every other test that passes probes= passes what find_nearest_centroids returned: distinct, in range,
nearest first.

Here every scan form — the f32 scan at its three block sizes and three merges, the one-phase PQ scans, the two-phase PQ scan with and
without an overflowing candidate list, the fused small-batch step with and without its overflow pass — gets tables that are none of
that: one list repeated up to 1 025 times, columns drawn with replacement (the empty list included), farthest first, only the
empty list, the only candidates behind the 512-column chunk seam (MAP_PCH, PQ2_PCH), and 64 | 65 columns on both sides of the fused
step's limit.  Every comparison is bit-exact against the oracle: doc ids, score bits, counts, padding.  The out-of-range branch of
every scan kernel is reached with one bad id in one row: status 2, a message, and the handle serves the next call.

Those errors are decided by valid kernels (every index they read with is guarded by the branch under test) and reported by the
host; nothing here faults.

tests/test_oracle_kat.py::test_probe_tables_are_the_concatenation_of_their_columns pins the oracle on the same tables without its heap.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_limits import assert_padding, device_rows, doc_ids_for, rows_to_result
from tests.test_gpu_parity import assert_result_rows

pytestmark = pytest.mark.gpu

FORMAT = 2                                           # MDB_ERR_FORMAT
NLISTS, B = 7, 8
COLS = (1, 2, 63, 64, 65, 511, 512, 513, 1025)      # around the fused step's 64 columns and the tile maps' chunks of 512
F32_SIZES = (197, 104, 0, 381, 9, 224, 285)         # 1 200 points: list 2 empty, list 4 short, list 3 the longest
PQ_SIZES = (310, 150, 420, 0, 12, 250, 358)         # 1 500 points: list 3 empty, list 2 the longest
D_F32, D_PQ, SUB = 20, 32, 8
BIG_B = 300                                          # above 256: the f32 scan's default block is the 256-thread one


# ----------------------------------------------------------------------------------- worlds and tables (plain numpy: the CPU test shares them)
def f32_world_data(seed=7):
    """1 200 x 20 around 6 well-separated centres (sizes F32_SIZES, point ids interleaved) and a centroid far from all of them"""
    rng = np.random.default_rng(seed)
    cent = rng.uniform(0, 200, (NLISTS, D_F32)).astype(np.float32)
    cent[F32_SIZES.index(0)] = 5000.0
    own = rng.permutation(np.repeat(np.arange(NLISTS), F32_SIZES))
    v = (cent[own] + rng.normal(0, 4, (len(own), D_F32))).astype(np.float32)
    q = (v[rng.integers(0, len(v), BIG_B)] + rng.normal(0, 2, (BIG_B, D_F32))).astype(np.float32)
    return v, cent, q


def pq_world_data(seed=11):
    """1 500 x 32 of integer components 0..3 (+ 5 c in cluster c), every cluster drawn with replacement from size / 8 distinct rows:
    equal points, equal codes, equal distances.  Sizes PQ_SIZES; a centroid far from all of them."""
    rng = np.random.default_rng(seed)
    cent = np.stack([np.full(D_PQ, 1.5 + 5 * c, np.float32) for c in range(NLISTS)])
    cent[PQ_SIZES.index(0)] = 1000.0
    own = rng.permutation(np.repeat(np.arange(NLISTS), PQ_SIZES))
    v = np.zeros((len(own), D_PQ), np.float32)
    for c, size in enumerate(PQ_SIZES):
        if size:
            base = rng.integers(0, 4, (max(size // 8, 1), D_PQ)).astype(np.float32) + 5 * c
            v[own == c] = base[rng.integers(0, len(base), size)]
    q = (v[rng.integers(0, len(v), B)] + rng.normal(0, 0.4, (B, D_PQ))).astype(np.float32)
    return v, cent, q


def probe_tables(sizes, nearest, b=B, seed=5):
    """name -> [b][cols] uint32.  `nearest`: the oracle's find_nearest_centroids(q, NLISTS)."""
    rng = np.random.default_rng(seed)
    longest, empty = int(np.argmax(sizes)), sizes.index(0)
    t = {}
    for c in COLS:
        t["one-list-x%d" % c] = np.full((b, c), longest, np.uint32)
        t["shuffled-dups-x%d" % c] = rng.integers(0, NLISTS, (b, c)).astype(np.uint32)      # another draw in every row
    t["farthest-first"] = np.ascontiguousarray(np.asarray(nearest, np.uint32)[:b, ::-1])
    for c in (1, 64, 65):
        t["empty-only-x%d" % c] = np.full((b, c), empty, np.uint32)
    seam = np.full((b, 513), empty, np.uint32)
    seam[:, 512] = longest
    t["seam"] = seam                                                                       # the only candidates: in the second chunk
    t["seam-mirror"] = np.ascontiguousarray(seam[:, ::-1])
    return t


def build_world(oracle, kind, docs_for):
    """files, oracles and tables of one world; `docs_for`: n -> doc ids"""
    if kind == "f32":
        v, cent, q = f32_world_data()
        sizes = F32_SIZES
        index, vec, pls = H.build_ivf_files(v, docs_for(len(v)), cent)
        quant = lambda m: oracle.Quant(oracle.QUANT_NONE, m)
        cb = None
    else:
        v, cent, q = pq_world_data()
        sizes = PQ_SIZES
        cb = H.train_pq_codebook(v, SUB, 8, iters=1, seed=3)
        codes = oracle.ProductQuantizer(D_PQ, SUB, 8, cb).quantize(v)
        index, vec, pls = H.build_ivf_files(v, docs_for(len(v)), cent, quantize=lambda x: codes)
        quant = lambda m: oracle.Quant(oracle.QUANT_PQ, m, SUB, 8, cb)
    assert tuple(len(p) for p in pls) == sizes
    w = dict(kind=kind, v=v, q=q[:B], q_big=q, docs=docs_for(len(v)), pls=pls, sizes=sizes, index=index, vec=vec, cb=cb, quant=quant,
             longest=int(np.argmax(sizes)), empty=sizes.index(0))
    for name, m in (("l2", 0), ("dot", 1)):
        w["o_" + name] = oracle.BlockBasedIvf(index, vec, quant(m))
    w["tables"] = probe_tables(sizes, w["o_l2"].find_nearest_centroids(q[:B], NLISTS))
    return w


def doc_counts(res, i):
    ids = res.doc_ids(i)
    return {d: ids.count(d) for d in set(ids)}


def check_guards(w, name, k, want, live_longest=None):
    """what makes a case real, asserted on the ORACLE's rows"""
    cols = w["tables"][name].shape[1] if name in w["tables"] else None
    if name.startswith("one-list"):
        n = w["sizes"][w["longest"]] if live_longest is None else live_longest
        assert np.all(want.counts == min(k, cols * n)), name
        for i in range(len(want.counts)):
            ids, m = want.doc_ids(i), doc_counts(want, i)
            # the k smallest (distance, point id) keys of a list named `cols` times: whole groups of `cols` copies and one remainder
            assert len(m) == -(-len(ids) // cols) and sorted(m.values())[1:] == [cols] * (len(m) - 1), (name, k, i)
            if w["kind"] == "f32" or k <= cols:   # (equal PQ distances of distinct points may put the remainder's group first)
                assert len(set(ids[:min(k, cols)])) == 1, (name, k, i)
    if name.startswith("shuffled-dups") and cols >= 63 and k >= 10:
        assert any(max(doc_counts(want, i).values()) > 1 for i in range(len(want.counts))), name
    if name.startswith("empty-only"):
        assert not want.counts.any()
    if name.startswith("seam"):
        assert np.all(want.counts == min(k, w["sizes"][w["longest"]]))


# ----------------------------------------------------------------------------------- fixtures
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


def gpu_quant(w, m):
    from muopdb_amd.index import NoQuantizer, ProductQuantizer
    return NoQuantizer(D_F32, m) if w["kind"] == "f32" else ProductQuantizer(D_PQ, SUB, 8, w["cb"], m)


class Worlds:
    """both worlds with their GPU handles, and the oracle's rows: computed once per (world, metric, table, k), shared, never changed"""

    def __init__(self, ctx, oracle):
        from muopdb_amd.index import BlockBasedIvf
        self.ctx, self.oracle, self.rows = ctx, oracle, {}
        self.w = {kind: build_world(oracle, kind, doc_ids_for) for kind in ("f32", "pq")}
        for w in self.w.values():
            for name, m in (("l2", 0), ("dot", 1)):
                w["g_" + name] = BlockBasedIvf(ctx, w["index"], w["vec"], gpu_quant(w, m))
            rng = np.random.default_rng(9)
            w["dups7"] = rng.integers(0, NLISTS, (B, 7)).astype(np.uint32)
            w["tables_big"] = {"shuffled-dups-x65": rng.integers(0, NLISTS, (BIG_B, 65)).astype(np.uint32)}

    def table(self, kind, name):
        w = self.w[kind]
        if name == "dups7":
            return w["dups7"]
        if name == "dups3":
            return np.ascontiguousarray(w["dups7"][:, :3])
        if name.startswith("big:"):
            return w["tables_big"][name[4:]]
        return w["tables"][name]

    def want(self, kind, metric, name, k, drop_row=None):
        key = (kind, metric, name, k, drop_row)
        if key not in self.rows:
            w, t = self.w[kind], self.table(kind, name)
            q = w["q_big"] if name.startswith("big:") else w["q"]
            if drop_row is not None:
                q, t = np.delete(q, drop_row, 0), np.delete(t, drop_row, 0)
            res = w["o_" + metric].search(q, k, probes=t, threads=8)
            check_guards(w, name, k, res)
            self.rows[key] = res
        return self.rows[key]

    def close(self):
        for w in self.w.values():
            w["g_l2"].close()
            w["g_dot"].close()


@pytest.fixture(scope="module")
def worlds(ctx, oracle):
    ws = Worlds(ctx, oracle)
    yield ws
    ws.close()


# ----------------------------------------------------------------------------------- forms
class Form:
    def __init__(self, name, kind, metric, opts, ks, max_cols=None):
        self.name, self.kind, self.metric, self.opts, self.ks, self.max_cols = name, kind, metric, opts, ks, max_cols

    def takes(self, table):
        return self.max_cols is None or table.shape[1] <= self.max_cols


K_F32, K_PQ1, K_PQ3 = (1, 10, 64, 2048), (1, 10, 100), (1, 10, 64)
FORMS = []
# ivf_scan_f32_kernel<M, 64 | 128 | 256> over TileMap::build.  One split: the block's row is the result; 3: merge_sorted_rows (3 k 8 bytes fit
# 48 KB up to k = 2 048); 16: merge_sorted_rows up to k = 64 and merge_keys at k = 2 048.  The splits are capped by the columns (mdb_ivf.hip:311).
for blk in (64, 128, 256):
    for ns in (1, 3, 16):
        for m in ("l2", "dot"):
            FORMS.append(Form("f32-%s-blk%d-nsplit%d" % (m, blk, ns), "f32", m, dict(MDB_SCAN_F32_BLK=blk, MDB_SCAN_F32_NSPLIT=ns), K_F32))
FORMS.append(Form("f32-l2-no-fused-remap", "f32", "l2", dict(MDB_SCAN_NO_FUSED_REMAP=1, MDB_SCAN_F32_NSPLIT=3), K_F32))
FORMS.append(Form("f32-l2-default", "f32", "l2", {}, K_F32))                   # the host's own nsplit from the column count
# one-phase PQ scans (16 splits per query at this batch, merge_sorted_rows behind them)
FORMS.append(Form("pq-l2-one-phase", "pq", "l2", dict(MDB_PQ_NO_FUSED=1), K_PQ1))                                   # ivf_scan_pq2_kernel<.., FILT>
FORMS.append(Form("pq-l2-no-filter", "pq", "l2", dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FILTER=1), K_PQ1))               # ivf_scan_pq2_kernel
FORMS.append(Form("pq-l2-no-fast", "pq", "l2", dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FAST=1), K_PQ1))                   # ivf_scan_pq_kernel
FORMS.append(Form("pq-dot-one-phase", "pq", "dot", dict(MDB_PQ_NO_FUSED=1), K_PQ1))
FORMS.append(Form("pq-dot-no-fast", "pq", "dot", dict(MDB_PQ_NO_FUSED=1, MDB_PQ_NO_FAST=1), K_PQ1))
# two-phase PQ scan: ivf_scan_pq3_kernel + ivf_pq3_refine_kernel, one block per query (MDB_PQ_BLOCKS = 1: the scan takes it for direct rows only)
PQ3 = dict(MDB_PQ_NO_FUSED=1, MDB_PQ_TWO_PHASE_MIN_B=1, MDB_PQ_BLOCKS=1)
for blk3 in (512, 1024):
    FORMS.append(Form("pq-l2-two-phase-blk%d" % blk3, "pq", "l2", dict(PQ3, MDB_PQ3_BLOCK=blk3), K_PQ3))
FORMS.append(Form("pq-l2-two-phase-cap16", "pq", "l2", dict(PQ3, MDB_PQ3_CAP=16), K_PQ3))   # overflow: the gated one-phase launch gives the rows
# ivf_pq_fused_kernel<.., 0>: probes given, up to 64 columns (IvfSet::fused_ok)
FORMS.append(Form("pq-l2-fused", "pq", "l2", {}, K_PQ3, max_cols=64))
FORMS.append(Form("pq-l2-fused-cap16", "pq", "l2", dict(MDB_PQF_CAP=16), K_PQ3, max_cols=64))                      # its in-kernel overflow pass
FORM_IDS = [f.name for f in FORMS]
ENTRY_FORMS = [f for f in FORMS if f.name in ("f32-l2-blk128-nsplit3", "f32-dot-blk256-nsplit16", "pq-l2-one-phase", "pq-l2-fused")]
ENTRY_IDS = [f.name for f in ENTRY_FORMS]
ENTRY_TABLES = ("one-list-x64", "one-list-x65", "shuffled-dups-x63", "shuffled-dups-x513", "farthest-first", "empty-only-x1", "seam")


def collect(failures, what, check):
    """runs one comparison; a failure is kept with its case, so that one run names every failing (table, k) of a form"""
    try:
        check()
    except AssertionError as e:
        failures.append("%s: %s" % (what, str(e).splitlines()[0] if str(e) else "rows differ"))


def assert_rows_and_padding(got, want, b, k):
    assert_result_rows(got, want, b)
    assert_padding(got, b, k)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_probe_tables(ctx, worlds, form):
    """every table a form can take, at every k of the form: the oracle's rows, counts and score bits, and the padding behind them"""
    w = worlds.w[form.kind]
    g, q, failures = w["g_" + form.metric], w["q"], []
    with options(ctx, **form.opts):
        for name, table in w["tables"].items():
            if not form.takes(table):
                continue
            for k in form.ks:
                want = worlds.want(form.kind, form.metric, name, k)
                got = g.search_with_centroids_and_remap(q, table, k)
                collect(failures, "%s k=%d" % (name, k), lambda: assert_rows_and_padding(got, want, B, k))
    assert not failures, "%s: %d cases differ from the oracle\n%s" % (form.name, len(failures), "\n".join(failures[:40]))


@pytest.mark.parametrize("form", [f for f in FORMS if f.kind == "f32" and ("nsplit3" in f.name or f.name == "f32-l2-default")],
                         ids=lambda f: f.name)
def test_probe_table_at_batch_300(ctx, worlds, form):
    """above 256 queries the f32 scan's default block is the 256-thread one and the host asks for fewer splits per query"""
    w = worlds.w["f32"]
    g, q, name = w["g_" + form.metric], w["q_big"], "big:shuffled-dups-x65"
    with options(ctx, **form.opts):
        for k in (10, 2048):
            got = g.search_with_centroids_and_remap(q, worlds.table("f32", name), k)
            assert_rows_and_padding(got, worlds.want("f32", form.metric, name, k), BIG_B, k)


def test_fused_step_stops_at_64_columns(ctx, worlds):
    """IvfSet::fused_ok takes 64 given columns and hands 65 to the unfused step: the same kind of table on both sides, the oracle's
    rows from both, and both scanned something"""
    w = worlds.w["pq"]
    g, q = w["g_l2"], w["q"]
    for cap in (2048, 16):
        with options(ctx, MDB_PQF_CAP=cap):
            for kind_ in ("one-list", "shuffled-dups"):
                for cols in (64, 65):
                    name = "%s-x%d" % (kind_, cols)
                    for k in K_PQ3:
                        ctx.stats()
                        got = g.search_with_centroids_and_remap(q, w["tables"][name], k)
                        scored = ctx.stats()["scored_vectors"]
                        assert_rows_and_padding(got, worlds.want("pq", "l2", name, k), B, k)
                        assert scored > 0, (name, k)
                        if kind_ == "one-list":     # every occurrence is scanned on either side of the limit (the fused overflow pass rescans)
                            assert scored >= B * cols * w["sizes"][w["longest"]], (name, k, scored)


# ----------------------------------------------------------------------------------- entry points
def point_rows(w, ids, sc, cn, k):
    """search_points' rows mapped through the doc-id table and ordered by (score, doc id); its own order must be (distance, point id)"""
    out = []
    for i in range(len(cn)):
        n = int(cn[i])
        own = [(float(sc[i, j]), int(ids[i, j])) for j in range(n)]
        assert own == sorted(own), "row %d is not in (distance, point id) order" % i
        out.append(sorted((float(sc[i, j]), w["docs"][int(ids[i, j])], int(np.asarray(sc[i, j:j + 1], np.float32).view(np.uint32)[0]))
                          for j in range(n)))
    return out


def assert_point_rows(w, got, want, k):
    ids, sc, cn = got
    rows = point_rows(w, ids, sc, cn, k)
    for i, row in enumerate(rows):
        assert len(row) == int(want.counts[i]), i
        assert [d for _, d, _ in row] == want.doc_ids(i), i
        assert [b_ for _, _, b_ in row] == [int(x) for x in np.asarray(want.scores[i, :len(row)], np.float32).view(np.uint32)], i


def entry_tables(w, form):
    return [(n, w["tables"][n]) for n in ENTRY_TABLES if form.takes(w["tables"][n])]


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_search_points_with_given_tables(ctx, worlds, form):
    w = worlds.w[form.kind]
    g, q = w["g_" + form.metric], w["q"]
    with options(ctx, **form.opts):
        for name, table in entry_tables(w, form):
            for k in (10, 64):
                assert_point_rows(w, g.search_points(q, k, 0, probes=table), worlds.want(form.kind, form.metric, name, k), k)


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_filtered_search_with_given_tables(ctx, oracle, worlds, form):
    """planner = the even point ids: a list named m times still returns an allowed point m times, a filtered point never appears"""
    from muopdb_amd.index import allow_bitmap
    w = worlds.w[form.kind]
    g, o, q, n = w["g_" + form.metric], w["o_" + form.metric], w["q"], len(w["v"])
    bm = allow_bitmap(np.arange(0, n, 2), n)
    even = {w["docs"][p] for p in range(0, n, 2)}
    with options(ctx, **form.opts):
        for name, table in entry_tables(w, form):
            for k in (10, 64):
                with oracle.planner_filter(bm):
                    want = o.search(q, k, probes=table)
                got = g.search_with_centroids_and_remap(q, table, k, planner=bm)
                assert_rows_and_padding(got, want, B, k)
                cols = table.shape[1]
                for i in range(B):
                    assert set(want.doc_ids(i)) <= even
                    if name.startswith("one-list") and k <= cols:
                        assert len(set(want.doc_ids(i))) == 1 and int(want.counts[i]) == k, (name, k, i)


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_tombstones_with_given_tables(ctx, oracle, worlds, form):
    """the nearest point of the longest list, invalidated on both sides: the one-list table returns the runner-up, repeated"""
    from muopdb_amd.index import BlockBasedIvf
    w = worlds.w[form.kind]
    m = 0 if form.metric == "l2" else 1
    g, o, q = BlockBasedIvf(ctx, w["index"], w["vec"], gpu_quant(w, m)), oracle.BlockBasedIvf(w["index"], w["vec"], w["quant"](m)), w["q"]
    one = np.full((B, 1), w["longest"], np.uint32)
    first = [o.search(q, 1, probes=one).doc_ids(i)[0] for i in range(B)]
    dead = sorted(set(first))
    for doc in dead:
        assert g.invalidate(doc) and o.invalidate(doc)
    live = w["sizes"][w["longest"]] - len(dead)
    with options(ctx, **form.opts):
        for name, table in entry_tables(w, form):
            for k in (10, 64):
                want = o.search(q, k, probes=table)
                check_guards(w, name, k, want, live_longest=live)
                assert_rows_and_padding(g.search_with_centroids_and_remap(q, table, k), want, B, k)
                for i in range(B):
                    assert not set(want.doc_ids(i)) & set(dead)
                    if name.startswith("one-list"):
                        assert want.doc_ids(i)[0] != first[i]
    g.close()


def submit_with_probes(ctx, g, q, table, k):
    """mdb_ivf_search_submit with a probe table (the Python wrapper passes none); returns the output buffers, mdb_wait is the caller's"""
    from muopdb_amd import lib as L
    from muopdb_amd.index import _OutBuf
    q, table = L.f32(q), np.ascontiguousarray(table, np.uint32)
    out = _OutBuf(len(q), k)
    st = ctx.lib.mdb_ivf_search_submit(g.h, L.ptr(q, C.c_float), C.c_size_t(len(q)), L.ptr(table, C.c_uint32), C.c_size_t(table.shape[1]),
                                       C.c_size_t(k), None, C.c_size_t(0), C.c_size_t(0), *out.args())
    return st, out


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_submit_and_wait_with_given_tables(ctx, worlds, form):
    w = worlds.w[form.kind]
    g, q = w["g_" + form.metric], w["q"]
    with options(ctx, **form.opts):
        for name, table in entry_tables(w, form):
            st, out = submit_with_probes(ctx, g, q, table, 10)
            assert st == 0, name
            ctx.check(ctx.lib.mdb_wait(ctx.h))
            assert_rows_and_padding(out.result(), worlds.want(form.kind, form.metric, name, 10), B, 10)


class DeviceSide:
    """a second context on a stream that torch uses too, with handles attached to the worlds' resident indexes"""

    def __init__(self, torch, worlds):
        from muopdb_amd import lib as L
        self.T, self.L = torch, L
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream()
        self.ctx = L.Context(0)
        self.ctx.set_stream(self.stream.cuda_stream)
        self.g = {(kind, m): w["g_" + m].attach(self.ctx) for kind, w in worlds.w.items() for m in ("l2", "dot")}

    def search(self, g, q, table, k):
        """mdb_ivf_search with queries, probes and outputs on the device; everything is enqueued on the borrowed stream and the
        status of the CALL is returned — rows() after mdb_sync"""
        T, L = self.T, self.L
        b = len(q)
        with T.cuda.stream(self.stream):
            qd = T.from_numpy(np.ascontiguousarray(q, np.float32)).to(self.dev)
            pd = T.from_numpy(np.ascontiguousarray(table, np.uint32).view(np.int32)).to(self.dev)
            ids, sc, cn, _ = device_rows(T, b, k)
            st = self.ctx.lib.mdb_ivf_search(g.h, C.c_void_p(qd.data_ptr()), C.c_size_t(b), C.c_void_p(pd.data_ptr()), C.c_size_t(table.shape[1]),
                                             C.c_size_t(k), C.c_int(L.MEM_DEVICE), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
                                             C.c_void_p(cn.data_ptr()))
        return st, (b, k, ids, sc, cn, qd, pd)

    def rows(self, bufs):
        b, k, ids, sc, cn = bufs[:5]
        with self.T.cuda.stream(self.stream):
            return rows_to_result(b, k, ids, sc, cn)

    def close(self):
        self.T.cuda.synchronize()
        for g in self.g.values():
            g.close()
        self.ctx.close()
        self.stream = None


@pytest.fixture(scope="module")
def device_side(worlds):
    torch = pytest.importorskip("torch")
    d = DeviceSide(torch, worlds)
    yield d
    d.close()


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_device_memory_call_with_given_tables(worlds, device_side, form):
    w, d = worlds.w[form.kind], device_side
    g, q = d.g[(form.kind, form.metric)], w["q"]
    with options(d.ctx, **form.opts):
        for name, table in entry_tables(w, form):
            for k in (10, 64):
                st, bufs = d.search(g, q, table, k)
                assert st == 0, name
                d.ctx.sync()
                assert_rows_and_padding(d.rows(bufs), worlds.want(form.kind, form.metric, name, k), B, k)


@pytest.mark.parametrize("form", ENTRY_FORMS, ids=ENTRY_IDS)
def test_three_shards_get_the_same_hostile_table(ctx, worlds, form):
    """every shard scans the table's columns it owns (most copies name lists of the other two); the merged blocks are the unsharded
    rows and the oracle's"""
    pytest.importorskip("torch")
    from muopdb_amd.index import BlockBasedIvf
    w = worlds.w[form.kind]
    m = 0 if form.metric == "l2" else 1
    g, q = w["g_" + form.metric], w["q"]
    shards = [BlockBasedIvf(ctx, w["index"], w["vec"], gpu_quant(w, m), shard_rank=r, shard_world=3) for r in range(3)]
    assert sum(s.num_resident_vectors() for s in shards) == len(w["v"]) and all(s.num_resident_vectors() for s in shards)
    with options(ctx, **form.opts):
        for name, table in entry_tables(w, form):
            for k in (10, 64):
                want = worlds.want(form.kind, form.metric, name, k)
                merged = shards[1].merge_shards([s.search_shard(q, k, probes=table) for s in shards], B, k)
                assert_rows_and_padding(merged, want, B, k)
                assert_rows_and_padding(g.merge_shards([g.search_shard(q, k, probes=table)], B, k), want, B, k)
        # a list id out of range is an error on EVERY shard, whichever would have owned it; the handles then serve the clean table
        for bad_id in BAD_IDS:
            for s in shards:
                assert_format_error(ctx, lambda: s.search_shard(q, 10, probes=bad_table(worlds, form.kind, bad_id)))
        clean = worlds.table(form.kind, "dups7")
        merged = shards[0].merge_shards([s.search_shard(q, 10, probes=clean) for s in shards], B, 10)
        assert_rows_and_padding(merged, worlds.want(form.kind, form.metric, "dups7", 10), B, 10)
    for s in shards:
        s.close()


# ----------------------------------------------------------------------------------- list ids out of range
BAD_ROW, BAD_COL = 3, 4
BAD_IDS = (NLISTS, 0xFFFFFFFF)          # num_clusters itself, and the value the fused kernel pads its unused probe lanes with


def bad_table(worlds, kind, bad_id, hollow=False):
    """`dups7` with one id out of range in one row (not row 0).  hollow: the rest of that row names the empty list, so the row has no
    tiles at all — in a split f32 scan every block of the row then leaves through the early return, which must raise the flag itself
    (mdb_ivf_scan.hip.h, `split * NW >= T0`)"""
    t = worlds.table(kind, "dups7").copy()
    if hollow:
        t[BAD_ROW, :] = worlds.w[kind]["empty"]
    t[BAD_ROW, BAD_COL] = bad_id
    return t


def assert_format_error(ctx, call):
    from muopdb_amd import lib as L
    with pytest.raises(L.MuopdbError) as e:
        call()
    assert e.value.status == FORMAT, e.value
    assert (ctx.lib.mdb_last_error(ctx.h) or b"").decode()


def test_oracle_refuses_the_bad_tables(worlds):
    for kind, w in worlds.w.items():
        for bad_id, hollow in ((BAD_IDS[0], False), (BAD_IDS[1], False), (BAD_IDS[0], True)):
            t = bad_table(worlds, kind, bad_id, hollow)
            for m in ("l2", "dot"):
                with pytest.raises(ValueError):
                    w["o_" + m].search(w["q"], 10, probes=t)
                w["o_" + m].search(np.delete(w["q"], BAD_ROW, 0), 10, probes=np.delete(t, BAD_ROW, 0))    # the other rows are fine


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_out_of_range_list_id(ctx, worlds, form):
    """one id >= num_clusters in one row: MDB_ERR_FORMAT and a message; then the clean table, and the batch without the bad row, on
    the same handle: the oracle's rows.  Three columns stay below every kernel's padding: status OK."""
    w = worlds.w[form.kind]
    g, q = w["g_" + form.metric], w["q"]
    with options(ctx, **form.opts):
        for bad_id, hollow in ((BAD_IDS[0], False), (BAD_IDS[1], False), (BAD_IDS[0], True)):
            t = bad_table(worlds, form.kind, bad_id, hollow)
            for k in form.ks[:2]:
                assert_format_error(ctx, lambda: g.search_with_centroids_and_remap(q, t, k))
                assert_rows_and_padding(g.search_with_centroids_and_remap(q, worlds.table(form.kind, "dups7"), k),
                                        worlds.want(form.kind, form.metric, "dups7", k), B, k)
                got = g.search_with_centroids_and_remap(np.delete(q, BAD_ROW, 0), np.delete(t, BAD_ROW, 0), k)
                assert_rows_and_padding(got, worlds.want(form.kind, form.metric, "dups7", k, drop_row=BAD_ROW), B - 1, k)
        for k in form.ks[:2]:
            assert_rows_and_padding(g.search_with_centroids_and_remap(q, worlds.table(form.kind, "dups3"), k),
                                    worlds.want(form.kind, form.metric, "dups3", k), B, k)


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_out_of_range_list_id_on_the_other_entry_points(ctx, worlds, device_side, form):
    """search_points, the filtered search and the shard block fail at once; submit fails in mdb_wait; a device-memory call returns OK
    and mdb_sync reports the error once, with the oracle's rows from the clean call issued behind it"""
    from muopdb_amd import lib as L
    from muopdb_amd.index import allow_bitmap
    w, d = worlds.w[form.kind], device_side
    g, q, n, k = w["g_" + form.metric], w["q"], len(w["v"]), 10
    clean, want = worlds.table(form.kind, "dups7"), worlds.want(form.kind, form.metric, "dups7", k)
    bm = allow_bitmap(np.arange(n), n)
    for bad_id in BAD_IDS:
        t = bad_table(worlds, form.kind, bad_id)
        with options(ctx, **form.opts):
            for call in (lambda: g.search_points(q, k, 0, probes=t),
                         lambda: g.search_with_centroids_and_remap(q, t, k, planner=bm),
                         lambda: g.search_shard(q, k, probes=t)):
                assert_format_error(ctx, call)
                assert_rows_and_padding(g.search_with_centroids_and_remap(q, clean, k), want, B, k)
            st, out = submit_with_probes(ctx, g, q, t, k)
            assert st == 0
            assert ctx.lib.mdb_wait(ctx.h) == FORMAT and (ctx.lib.mdb_last_error(ctx.h) or b"").decode()
            assert ctx.lib.mdb_wait(ctx.h) == 0
            st, out = submit_with_probes(ctx, g, q, clean, k)
            assert st == 0
            ctx.check(ctx.lib.mdb_wait(ctx.h))
            assert_rows_and_padding(out.result(), want, B, k)
        with options(d.ctx, **form.opts):
            gd = d.g[(form.kind, form.metric)]
            st_bad, _bad = d.search(gd, q, t, k)
            st_ok, bufs = d.search(gd, q, clean, k)                       # behind the bad call, before any sync
            assert (st_bad, st_ok) == (0, 0)
            with pytest.raises(L.MuopdbError) as e:
                d.ctx.sync()
            assert e.value.status == FORMAT and (d.ctx.lib.mdb_last_error(d.ctx.h) or b"").decode()
            d.ctx.sync()                                                  # reported once
            assert_rows_and_padding(d.rows(bufs), want, B, k)

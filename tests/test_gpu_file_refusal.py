"""GPU tests (-m gpu) of the loaders over the mutation table (tests/file_mutations.py).

Every refused case is refused by the loader's host half (muopdb_amd/csrc/mdb_files.cpp) before the first device call:
tests/test_file_refusal.py establishes the statuses without a device, and `mdb_*_load` calls the same function.  So no case here puts
unvalidated offsets on the device, and no handle whose file the checker refused is ever searched: if a load returns MDB_OK for such a
case the test frees the handle and fails there.

- refused loads behave: the loader returns the checker's status and message, hands out no handle, and the same context then loads
  the unmutated files and returns the oracle's rows (nothing pending, nothing deferred to mdb_sync).  "No handle" is a deliberate
  reading of "`*out` is not written": every `*_load` of this ABI sets `*out = NULL` on entry, before it looks at anything — a caller's
  stale pointer never survives a failed load — so the test seeds `*out` with a pattern and requires NULL afterwards, never the pattern
  (the loader did not run its first line) and never anything else (a handle);
- refused loads leak nothing: the device's free bytes move around 20 refused loads as they move around none;
- benign mutations are served: every accepted case loads, and rows, scores and counts equal the oracle's on the same bytes."""
import ctypes as C
import re

import numpy as np
import pytest

from muopdb_amd import lib as L
from tests import file_mutations as M
from tests.test_gpu_parity import assert_result_rows

pytestmark = pytest.mark.gpu

NO_HANDLE = 0x5A5A5A5A5A5A5A50      # what `*out` holds before a load: a refused load leaves NULL there, never a handle
FREE = dict(hnsw="mdb_hnsw_free", ivf="mdb_ivf_free", spann="mdb_spann_free", multi="mdb_multi_spann_free")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def raw_load(ctx, case):
    """(status, handle or None, mdb_last_error) of the case's loader, called as a binder calls it"""
    lib, a, sz = ctx.lib, case.args, C.c_size_t
    q, keep = M.quant_desc(a.get("quant"))
    qp = C.byref(q) if q is not None else None
    h = C.c_void_p(NO_HANDLE)
    if case.loader in ("hnsw", "ivf"):
        bufs = M.file_args(case, ("index", "vectors"))
        (ip, il), (vp, vl) = bufs[0]
        common = (ctx.h, ip, il, sz(a.get("index_offset", 0)), vp, vl, sz(a.get("vectors_offset", 0)), qp)
        if case.loader == "hnsw":
            st = lib.mdb_hnsw_load(*common, C.byref(h))
        else:
            st = lib.mdb_ivf_load(*common, C.c_uint32(a.get("shard_rank", 0)), C.c_uint32(a.get("shard_world", 1)), C.byref(h))
    else:
        bufs = M.file_args(case, ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors"))
        (hp, hl), (hvp, hvl), (ip, il), (vp, vl) = bufs[0]
        if case.loader == "spann":
            st = lib.mdb_spann_load(ctx.h, hp, hl, sz(0), hvp, hvl, sz(0), ip, il, sz(0), vp, vl, sz(0), qp, C.byref(h))
        else:
            users, n = M.user_records(case.files["user_table"])
            st = lib.mdb_multi_spann_load(ctx.h, users, sz(n), C.c_uint32(a["num_features"]), hp, hl, hvp, hvl, ip, il, vp, vl, qp,
                                          C.c_uint32(a.get("shard_rank", 0)), C.c_uint32(a.get("shard_world", 1)), C.byref(h))
    del bufs, keep
    return int(st), h.value, (lib.mdb_last_error(ctx.h) or b"").decode()


def refused_load(ctx, case):
    """loads a case the checker refuses; a handle that comes back all the same is freed, never searched"""
    st, handle, msg = raw_load(ctx, case)
    if st == M.OK and handle not in (None, NO_HANDLE):
        getattr(ctx.lib, FREE[case.loader])(C.c_void_p(handle))
    assert st != M.OK, "%s: the loader accepted a file its own host half refuses" % case.name
    return st, handle, msg


def quantizers(oracle, q):
    """(product quantizer, oracle Quant) of a table descriptor"""
    from muopdb_amd.index import ProductQuantizer
    if q is None or q["kind"] == 0:
        return None, None
    return (ProductQuantizer(q["dimension"], q["subvector_dimension"], q["num_bits"], q["codebook"]),
            oracle.Quant(oracle.QUANT_PQ, oracle.METRIC_L2, q["subvector_dimension"], q["num_bits"], q["codebook"]))


def _queries(seed, b=6):
    return np.random.default_rng(seed).standard_normal((b, M.DIM)).astype(np.float32)


def serve(ctx, oracle, loader, files, args):
    """loads the files on the device and in the oracle, searches both and holds the rows, scores and counts equal"""
    from muopdb_amd.index import BlockBasedHnsw, BlockBasedIvf, MultiSpannIndex, SearchParams, Spann
    gq, oq = quantizers(oracle, args.get("quant"))
    q = _queries(len(files))
    if loader == "hnsw":
        g = BlockBasedHnsw(ctx, files["index"], files["vectors"], M.DIM, gq)
        o = oracle.BlockBasedHnsw(files["index"], files["vectors"], M.DIM, oq)
        for k, ef in ((5, 12), (3, 300)):
            assert_result_rows(g.ann_search(q, k, ef), o.ann_search(q, k, ef), len(q))
    elif loader == "ivf":
        g = BlockBasedIvf(ctx, files["index"], files["vectors"], gq)
        o = oracle.BlockBasedIvf(files["index"], files["vectors"], oq)
        probes = min(3, o.num_clusters)
        assert_result_rows(g.search(q, 5, probes), o.search(q, 5, num_probes=probes), len(q))
    else:
        p = SearchParams(5, 20).with_num_explored_centroids(3).with_centroid_distance_ratio(0.5)
        op = oracle.SearchParams(5, 20, num_explored_centroids=3, centroid_distance_ratio=0.5)
        four = [files[k] for k in ("hnsw_index", "hnsw_vectors", "ivf_index", "ivf_vectors")]
        if loader == "spann":
            g, o = Spann(ctx, *four, gq), oracle.Spann(*four, oq)
            r, ro = g.search(q, p), o.search(q, op)
        else:
            table = files["user_table"]
            users = [int.from_bytes(table[i:i + 16], "little") for i in range(0, len(table), 112)] + [999]   # (999: an unknown user)
            ids = [users[i % len(users)] for i in range(len(q))]
            g = MultiSpannIndex(ctx, table, args["num_features"], *four, gq)
            o = oracle.MultiSpannIndex(table, args["num_features"], *four, oq)
            r, ro = g.search_for_user(ids, q, p), o.search_for_user(ids, q, op)
        assert [bool(f) for f in r.found] == [bool(f) for f in ro.found]
        assert_result_rows(r, ro, len(q))
    g.close()
    ctx.sync()   # nothing deferred


def _site(msg):
    return re.sub(r"\d+", "#", msg)


def refusal_classes(loader):
    """one case per distinct refusal message (numbers aside) of the loader's cases, by the host-only checker"""
    seen, out = set(), []
    for c in M.cases():
        if c.loader != loader or c.status == M.OK:
            continue
        st, msg = M.check(c)
        if st != M.OK and _site(msg) not in seen:
            seen.add(_site(msg))
            out.append((c, st, msg))
    return out


@pytest.mark.parametrize("loader", ["hnsw", "ivf", "spann", "multi"])
def test_refused_loads_behave(ctx, oracle, loader):
    classes = refusal_classes(loader)
    assert len(classes) >= {"hnsw": 20, "ivf": 20, "spann": 4, "multi": 8}[loader], [m for _, _, m in classes]
    bases = [(n, b) for n, b in M.base().items() if b[0] == loader]
    for i, (case, want, why) in enumerate(classes):
        st, handle, msg = refused_load(ctx, case)
        assert (st, msg) == (want, why), case.name
        assert handle is None, "%s: `*out` holds %r after a refused load" % (case.name, handle)
        if i % 4 == 0 or i == len(classes) - 1:   # the same context serves the unmutated files: nothing pending, nothing deferred
            name, (_, files, args) = bases[(i // 4) % len(bases)]
            serve(ctx, oracle, loader, files, args)


def test_refused_loads_leak_nothing(ctx, oracle):
    """Free bytes of the device (mdb_device_mem_info, after the stream has drained) around 20 refused loads and around none, after one
    warm-up cycle of the same loads and one valid load-and-free of the same files.  Among the 20: the SPANN pair whose IVF half
    passes and whose graph half is refused, and the collection whose LAST user is corrupt, in its lists and in its graph — both
    halves of every user are planned before either is uploaded (spann_plan_files), so these too are refused with nothing on the device.
    Observed on the MI355X: 0 bytes around none and 0 around the 20, so no allowance for pooling is made."""
    by_name = {c.name: c for c in M.cases()}
    names = ["spann.graph_dimension_differs", "spann.graph_edge_out_of_range", "spann_pq.graph_vectors_cut", "multi.last_user_graph_edge_out_of_range",
             "multi.last_user_ivf_version", "multi.users_disagree_on_num_features", "multi.num_features_argument_differs",
             "hnsw.doc_ids_one_short", "hnsw.entry_slot_past_vectors", "hnsw_pq.edge_nv_upper", "ivf.header_counts_one_more_vector",
             "ivf_pq.list_header_L_64", "ivf.index_cut_0", "hnsw.degree_257", "ivf_pq.descriptor_codebook_short"]
    batch = [by_name[n] for n in names] + [by_name[n] for n in names[:5]]
    assert len(batch) == 20

    def cycle():
        for case in batch:
            refused_load(ctx, case)
    cycle()                                            # warm-up: pinned staging, scratch, the runtime's own pools
    for name in ("spann", "multi"):
        _, files, args = M.base()[name]
        serve(ctx, oracle, name, files, args)
    a0 = ctx.mem_info()[0]
    a1 = ctx.mem_info()[0]
    b0 = ctx.mem_info()[0]
    cycle()
    b1 = ctx.mem_info()[0]
    print("free bytes around none: %d, around 20 refused loads: %d" % (a1 - a0, b1 - b0))
    assert b1 - b0 == a1 - a0


ACCEPTED = [c for c in M.cases() if c.status == M.OK]


@pytest.mark.parametrize("loader", ["hnsw", "ivf", "spann", "multi"])
def test_benign_mutations_are_served(ctx, oracle, loader):
    mine = [c for c in ACCEPTED if c.loader == loader]
    assert len(mine) >= {"hnsw": 10, "ivf": 4, "spann": 2, "multi": 3}[loader], [c.name for c in mine]
    for case in mine:
        st, msg = M.check(case)
        assert (st, msg) == (M.OK, ""), case.name
        try:
            serve(ctx, oracle, loader, case.files, case.args)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (case.name, e))

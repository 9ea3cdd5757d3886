"""mdb_flat_search_filtered: the exact scan under per-call allow bitmaps over row ids (-m gpu).

Reference: oracle.flat_topk(metric, base[rows], q, k) over the allowed rows alone, ids mapped back: ids, score BITS, counts, padding.
Every bitmap runs with MDB_FLAT_ALLOW_DENSE = 0 (every tile in place), 65 (every row through the ring) and the default, on the default
grid and on a few blocks that loop over many tile groups, from host and from device memory: the same bits and stats every time."""
import numpy as np
import pytest
from muopdb_amd import lib as L
from muopdb_amd.index import FlatIndex, pack_allow

pytestmark = pytest.mark.gpu
INVALID_ARG, ERR_NAN, UNSUPPORTED = 1, 5, 7
# (n, d, MDB_FLAT_BLOCKS of the looping form): a ragged last tile in a ragged last group, d = 29 the whole 16/8/4/scalar cascade
SHAPES = {"d16": (64 * 4 * 3 + 37, 16, 1), "d29": (64 * 4 * 3 + 37, 29, 1), "big": (20000, 32, 8)}

def _mixed(n, rng):   # tiles alternate full and 15 live rows (sparse under the default 16): the ring fills in a block's third group, drains, refills
    return (np.arange(n) // 64 % 2 == 0) | (np.arange(n) % 64 < 15)

def _per_query(n, rng):
    m = np.stack([rng.random(n) < rho for rho in (1 / 2, 1 / 64, 1 / 4, 1 / 64, 1 / 2, 1 / 4)])
    m[:, n - 70] = np.arange(6) == 0   # a row that one query of the group allows alone
    return m

BITMAPS = {   # (n, rng) -> bool [n] shared, or [6][n] one row per query
    "ones": lambda n, rng: np.ones(n, bool),
    "zeros": lambda n, rng: np.zeros(n, bool),
    "single": lambda n, rng: np.arange(n) == n - 5,   # in the last, partial tile
    "sparse": lambda n, rng: rng.random(n) < 1 / 64,
    "half": lambda n, rng: rng.random(n) < 1 / 2,
    "mixed": _mixed,
    "few": lambda n, rng: np.isin(np.arange(n), rng.choice(n, 7, replace=False)),   # fewer rows than k
    "past_n": lambda n, rng: rng.random(n) < 1 / 2,   # packed with every bit past n set and a word more than needed
    "per_query": _per_query,
}

@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()

@pytest.fixture(scope="module")
def worlds(ctx):
    out = {}
    for name, (n, d, few) in SHAPES.items():
        rng = np.random.default_rng(n + d)
        base = rng.standard_normal((n, d)).astype(np.float32)
        q = (base[rng.integers(0, n, 6)] + 0.5 * rng.standard_normal((6, d))).astype(np.float32)
        out[name] = dict(n=n, d=d, few=few, base=base, q=q, idx={m: FlatIndex(ctx, base, m) for m in (L.METRIC_L2, L.METRIC_DOT)})
    return out

def expected(oracle, metric, base, q, k, mask):
    ids, dist, counts = [], [], []
    for i in range(len(q)):
        rows = np.flatnonzero(mask[i] if mask.ndim == 2 else mask)
        oi, od = oracle.flat_topk(metric, base[rows], q[i:i + 1], k)
        ids.append(np.where(oi[0] != 0xFFFFFFFF, np.append(rows, 0)[np.minimum(oi[0], len(rows))], 0xFFFFFFFF).astype(np.uint32))
        dist.append(od[0])
        counts.append(min(k, len(rows)))
    return np.stack(ids), np.stack(dist), np.asarray(counts, np.uint32), int(np.broadcast_to(mask, (len(q), mask.shape[-1])).sum())

def check(got, want, what):   # ids, score bits, counts
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2]), what

@pytest.mark.parametrize("bitmap", list(BITMAPS))
@pytest.mark.parametrize("metric", [L.METRIC_L2, L.METRIC_DOT], ids=["l2", "dot"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_filtered_rows_and_stats_match_the_oracle(ctx, oracle, worlds, shape, metric, bitmap):
    import torch
    w = worlds[shape]
    n, d, idx = w["n"], w["d"], w["idx"][metric]
    mask6 = BITMAPS[bitmap](n, np.random.default_rng(7))
    default = ctx.get_option("MDB_FLAT_ALLOW_DENSE")
    forms = [(0, 0, False), (65, 0, False), (default, 0, False), (default, w["few"], False), (65, w["few"], True)]
    for b in (1, 3, 6):   # QT 1, a padded group of 4 (or two of 2), more than one group
        q, mask = w["q"][:b], (mask6[:b] if mask6.ndim == 2 else mask6)
        bm = pack_allow(mask)
        if bitmap == "past_n":
            bm = np.concatenate([bm, np.full(bm.shape[:-1] + (1,), 0xFFFFFFFF, np.uint32)], -1)
            bm[..., n // 32] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
        for k in (1, 10, 70):
            want = expected(oracle, metric, w["base"], q, k, mask)
            if bitmap == "ones":
                check(idx.search(q, k), want, "unfiltered b=%d k=%d" % (b, k))
            for dense, blocks, device in forms:
                what = "%s b=%d k=%d dense=%d blocks=%d device=%d" % (bitmap, b, k, dense, blocks, device)
                with ctx.option("MDB_FLAT_ALLOW_DENSE", dense), ctx.option("MDB_FLAT_BLOCKS", blocks):
                    dev = torch.from_numpy(mask if bitmap != "past_n" else bm.view(np.int32)).cuda() if device else None   # bool rows: packed on the GPU
                    got = idx.search(q, k, allow=dev if device else bm)
                check(got, want, what)
                assert ctx.stats() == dict(scored_vectors=want[3], distance_evals=0, expanded_nodes=0,
                                           algorithmic_bytes=want[3] * d * 4 + b * d * 4 + b * k * 8), what

def enqueue(idx, q_t, k, allow_t):   # the raw MDB_MEM_DEVICE call on torch tensors: only enqueues; (status, reader of the rows)
    import torch
    b = q_t.shape[0]
    ids, dist, counts = (torch.empty(s, dtype=t, device=q_t.device) for s, t in (((b, k), torch.int32), ((b, k), torch.float32), (b, torch.int32)))
    nb, words = (1, allow_t.shape[0]) if allow_t.dim() == 1 else allow_t.shape
    st = idx.ctx.lib.mdb_flat_search_filtered(idx.h, q_t.data_ptr(), b, k, L.MEM_DEVICE, allow_t.data_ptr(), nb, words,
                                              ids.data_ptr(), dist.data_ptr(), counts.data_ptr())
    return st, lambda: (ids.cpu().numpy().view(np.uint32), dist.cpu().numpy(), counts.cpu().numpy().view(np.uint32))

def test_borrowed_stream_without_host_synchronisation(oracle, worlds):
    import torch
    w = worlds["big"]
    mask = _per_query(w["n"], np.random.default_rng(3))
    ctx2 = L.Context(0)
    idx = FlatIndex(ctx2, w["base"])
    s = torch.cuda.Stream()
    ctx2.set_stream(s.cuda_stream)
    hq, hb = torch.from_numpy(w["q"]).pin_memory(), torch.from_numpy(pack_allow(mask).view(np.int32)).pin_memory()
    with torch.cuda.stream(s):   # the inputs arrive by copies enqueued on the borrowed stream; nothing waits for them before the call
        st, rows = enqueue(idx, hq.to("cuda", non_blocking=True), 10, hb.to("cuda", non_blocking=True))
    assert st == 0
    ctx2.sync()
    check(rows(), expected(oracle, L.METRIC_L2, w["base"], w["q"], 10, mask), "borrowed stream")
    ctx2.close()

@pytest.mark.parametrize("dense", [0, 65, 16])
def test_nan_counts_only_in_an_allowed_row(ctx, oracle, worlds, dense):
    import torch
    w = worlds["d16"]
    base, q, bad = w["base"].copy(), w["q"][:3], 300
    base[bad, 3] = np.nan
    idx = FlatIndex(ctx, base)
    mask = np.random.default_rng(5).random(w["n"]) < 1 / 2
    with ctx.option("MDB_FLAT_ALLOW_DENSE", dense):
        for allowed in (False, True):
            mask[bad] = allowed
            bm = pack_allow(mask)
            st, rows = enqueue(idx, torch.from_numpy(q).cuda(), 10, torch.from_numpy(bm.view(np.int32)).cuda())
            assert st == 0   # device memory: the call only enqueues, a NaN is mdb_sync's to report
            if not allowed:
                ctx.sync()
                want = expected(oracle, L.METRIC_L2, base, q, 10, mask)
                check(rows(), want, "NaN row not allowed, device")
                check(idx.search(q, 10, allow=bm), want, "NaN row not allowed, host")
            for call in (ctx.sync, lambda: idx.search(q, 10, allow=bm)) if allowed else ():
                with pytest.raises(L.MuopdbError) as e:
                    call()
                assert e.value.status == ERR_NAN

def test_refusals_leave_the_handle_and_the_stats_as_they_were(ctx, oracle, worlds):
    w = worlds["d29"]
    n, idx, q = w["n"], w["idx"][L.METRIC_L2], w["q"][:3]
    mask = np.random.default_rng(9).random((3, n)) < 1 / 4
    bm = pack_allow(mask)
    want = expected(oracle, L.METRIC_L2, w["base"], q, 10, mask)
    check(idx.search(q, 10, allow=bm), want, "before")
    stats = ctx.stats()
    assert stats["scored_vectors"] == want[3] == mask.sum() and bm.shape[1] == (n + 31) // 32
    for allow, k, status in ((bm[:, :-1], 10, INVALID_ARG), (bm[:2], 10, INVALID_ARG), (bm, 2049, UNSUPPORTED)):   # a word short; 1 < n_bitmaps < b; k past the limit
        with pytest.raises(L.MuopdbError) as e:
            idx.search(q, k, allow=allow)
        assert e.value.status == status and ctx.stats() == stats
        check(idx.search(q, 10, allow=bm), want, "after a refusal")

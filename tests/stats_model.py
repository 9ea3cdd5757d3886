"""A host model of mdb_stats (include/muopdb_hip.h, "mdb_stats: the contract"): plain numpy, no GPU, none of the library's code.

Every function returns the four fields of mdb_stats as a dict of Python ints, from what a test already holds: the posting lists, the
probe rows, the tombstoned point ids, the allow bitmaps, the oracle's graph counters and the shapes.  The per-unit bytes are the
published ones (BASELINE.md's workload table), restated here:

    flat     one pass over the base + the queries + the outputs     n d 4 + b d 4 + b k 8
    graph    a row and its edge id per distance evaluation          d 4 + 4   (f32 rows)     m + 4   (PQ codes of m bytes)
             the offsets of an expanded node's adjacency            16
    lists    a row and its point id per scored posting-list entry   d 4 + 4   (f32 lists)    m + 4   (PQ lists)

What counts as SCORED in a posting-list scan is one rule: an entry of a probed list whose point is neither tombstoned nor dropped by
the query's allow bitmap, once per occurrence of its list in the query's probe row (a list named three times is scanned three
times).  tests/test_stats_model.py holds the model to the oracle's own counts.
"""
import numpy as np

FIELDS = ("scored_vectors", "distance_evals", "expanded_nodes", "algorithmic_bytes")
EXPANDED_BYTES = 16


def _stats(scored, evals, expanded, nbytes):
    return dict(scored_vectors=int(scored), distance_evals=int(evals), expanded_nodes=int(expanded), algorithmic_bytes=int(nbytes))


def row_bytes(d=None, m=None):
    """bytes of one stored row and its 4-byte id: f32 rows of dimension d, or PQ codes of m bytes"""
    assert (d is None) != (m is None)
    return (d * 4 if m is None else m) + 4


def flat(n, d, b, k):
    return _stats(b * n, 0, 0, n * d * 4 + b * d * 4 + b * k * 8)


def hnsw(evals, expanded, d=None, m=None):
    """(evals, expanded): the oracle's counters of the call"""
    return _stats(0, evals, expanded, evals * row_bytes(d, m) + expanded * EXPANDED_BYTES)


def allowed(allow, qi, point):
    """bit `point` of query qi's bitmap: `allow` is None (no filter), uint32 [words] (shared) or [n_bitmaps][words] (one per query)"""
    if allow is None:
        return True
    a = np.asarray(allow, np.uint32)
    row = a if a.ndim == 1 else a[qi]
    return bool((int(row[point >> 5]) >> (point & 31)) & 1)


def ivf_scored(posting_lists, probes, dead=(), allow=None, owned=None):
    """(query, entry) pairs the scan evaluates.  posting_lists[c]: the point ids of list c; probes: [b] rows of list ids (any
    length, repeats count); dead: tombstoned point ids; owned: the lists this shard holds (None: all)"""
    dead = set(int(p) for p in dead)
    live = [[int(p) for p in pl if int(p) not in dead] for pl in posting_lists]
    total = 0
    for qi, row in enumerate(probes):
        for c in row:
            c = int(c)
            if owned is not None and c not in owned:
                continue
            total += len(live[c]) if allow is None else sum(1 for p in live[c] if allowed(allow, qi, p))
    return total


def ivf(posting_lists, probes, d=None, m=None, dead=(), allow=None, owned=None):
    s = ivf_scored(posting_lists, probes, dead, allow, owned)
    return _stats(s, 0, 0, s * row_bytes(d, m))


def ratio_filter(list_ids, distances, ratio):
    """Spann::search's filter over the centroid graph's rows (nearest first): list i is kept when, in f32,
    distance[i] - nearest <= nearest * ratio.  -> the kept list ids, in order"""
    dist = np.asarray(distances, np.float32)
    if len(dist) == 0:
        return []
    nearest = dist[0]
    rhs = np.float32(nearest * np.float32(ratio))
    return [int(c) for c, x in zip(list_ids, dist) if np.float32(x - nearest) <= rhs]


def spann(evals, expanded, scored, d, m=None):
    """the centroid graphs' counters summed over the batch (f32 rows of dimension d, always) + the scan of the kept lists
    (f32 lists of dimension d, or PQ lists of m bytes)"""
    return _stats(scored, evals, expanded, evals * row_bytes(d) + expanded * EXPANDED_BYTES + scored * row_bytes(None if m else d, m))


def balanced_owner(list_sizes, world):
    """the rank that holds each list of ONE sharded index: lists taken longest first (equal lengths: the lower
    index first), each to the rank with the least entries so far (equal loads: the lower rank)"""
    load, owner = [0] * world, [0] * len(list_sizes)
    for c in sorted(range(len(list_sizes)), key=lambda c: (-int(list_sizes[c]), c)):
        r = min(range(world), key=lambda r: (load[r], r))
        owner[c] = r
        load[r] += int(list_sizes[c])
    return owner


def modulo_owner(num_lists, world):
    """multi-user collections: list c of every user on rank c % world"""
    return [c % world for c in range(num_lists)]


def add(a, b):
    return {k: a[k] + b[k] for k in FIELDS}

"""CPU model of the frontier form's theta over the points NOT YET VISITED, with the selects taken late and reused downwards (what
mdb_hnsw_closure.hip.h runs; no GPU, no product code).  It chains tests/closure_bound_model.py's closure_bound_layer — the counted stop
test under any valid bound — over the upper layers of one query, which share one visited set as the reference's ann_search does.

THE POOL.   A layer evaluates its entry point and the points it discovers that no layer above has visited.  So all that theta has to
            promise — at most ef - 2 OTHER points THAT THIS LAYER CAN EVALUATE are as near as a point with d < theta — is a statement
            about (set \\ visited on entry) + {entry point}, not about the whole set the layer's points come from.
THE RANK.   The entry point is marked visited before the select runs, and the select simply skips every visited point: it takes
            index ef - 2 (the (ef - 1)-th smallest) of the unvisited rest.  With the entry point put back that value sits at index
            ef - 2 or ef - 1 of the pool, so it is never above the pool's own index ef - 1: one rank conservative when the entry point
            is farther than it, exact when it is nearer.  An unvisited rest of <= ef - 1 points makes a pool of <= ef points: +inf.
LATE.       A select runs at the first layer that uses it, behind that layer's entry into the visited set: the layers above have left
            their visits there.  Layers that are certain as a whole (the tiny top layers at ef >= 64) take no select.
REUSE.      A select taken at layer l over a set serves every lower layer that uses the same set: the visited set only grows, and a
            lower layer's entry point was evaluated by the layer above it — it was unvisited, or the entry point, when the select ran.
            Every lower pool is a subset of (rest at the select) + {its entry point}, whose index ef - 1 is no smaller than the select's
            index ef - 2 of the rest.

`select_rest` is the select in exact form (any totally ordered distances), `select_rest_hist` restates cl_theta's two histogram passes
on canonical images (never above the exact form).  `drop` and `rank` exist for the tests that show a wrong pool or a wrong rank can be
told.  A flagged layer is re-run by the sequential form (tests/closure_model.search_layer), as the product does.
"""
import collections

from tests import closure_bound_model as BM
from tests import closure_model as CM

LayerRun = collections.namedtuple("LayerRun", "layer ep visited_in theta selected rest state info")


def select_rest(dist, members, visited, ef, rank=None, drop=()):
    """index `rank` (default ef - 2) of the sorted distances of members \\ visited \\ drop; None = +inf when the set holds <= ef points
    or the rest <= rank + 1; -> (theta, size of the rest)"""
    rank = ef - 2 if rank is None else rank
    if len(members) <= ef:
        return None, None
    rest = sorted(dist[p] for p in members if p not in visited and p not in drop)
    if rank < 0:
        return min(dist[p] for p in members), len(rest)     # nothing is nearer than the set's minimum: every point is popped alone
    if len(rest) <= rank + 1:
        return None, len(rest)
    return rest[rank], len(rest)


def select_rest_hist(keys, members, visited, ef):
    """cl_theta: `keys[p]` are canonical images (ints).  The key range comes from the WHOLE set (a range over a superset is still a
    range), the two passes of up to 11 bits skip the visited points, the first pass's grand total is the size of the rest."""
    if len(members) <= ef:
        return None, None
    if ef < 2:
        return 0, None
    kmin = min(keys[p] for p in members)
    hi = (max(keys[p] for p in members) - kmin).bit_length()
    rest = [keys[p] for p in members if p not in visited]
    if hi == 0:
        return kmin, len(rest)                              # one image throughout: no pass, nothing is below it
    prefix, k = 0, ef - 2
    for npass in range(2):
        if hi == 0:
            break
        bits = min(hi, 11)
        lo = hi - bits
        counts = [0] * (1 << bits)
        for v in rest:
            kp = v - kmin
            if kp >> hi == prefix:
                counts[(kp >> lo) & ((1 << bits) - 1)] += 1
        if npass == 0 and sum(counts) <= ef - 1:
            return None, len(rest)
        digit = 0
        while k >= counts[digit]:
            k -= counts[digit]
            digit += 1
        prefix, hi = (prefix << bits) | digit, lo
    return kmin + (prefix << hi), len(rest)


def chain(layers, dist, entry, ef, set_of, members, all_certain=(), select=select_rest, pop_cap=None):
    """layers: [(layer number, rows)] from the top down; set_of[layer]: the name of the set its select runs over, members[name]: that
    set's points; all_certain: layers that take theta = +inf.  -> [LayerRun], one per layer, each started from the state above it."""
    visited, ep = set(), entry
    taken = {}                                              # set name -> theta of the select already taken over it
    runs = []
    for layer, rows in layers:
        visited_in = set(visited)
        selected, rest = False, None
        if layer in all_certain:
            theta = None
        else:
            name = set_of[layer]
            if name not in taken:                           # late: behind this layer's entry into the visited set
                taken[name], rest = select(dist, members[name], visited_in | {ep}, ef)
                selected = True
            theta = taken[name]
        state, info = BM.closure_bound_layer(rows, dist, ep, ef, visited_in, theta, pop_cap)
        runs.append(LayerRun(layer, ep, visited_in, theta, selected, rest, state, info))
        if state.hazard:                                    # flagged: the sequential form re-runs the layer
            state = CM.search_layer(rows, dist, ep, ef, visited_in)
        visited, ep = state.visited, state.nearest
    return runs

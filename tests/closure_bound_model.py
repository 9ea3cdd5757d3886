"""CPU model of the frontier form of mdb_hnsw_closure.hip.h as the kernels run it now (no GPU, no product code): tests/closure_model.py's
closure_layer with two changes.

theta is a BOUND.  closure_layer takes theta = the ef-th smallest distance of the layer's row.  All it uses of theta is that at most
            ef - 2 other points are as near as a point with d < theta; that holds for every theta' <= theta as well.  A smaller theta'
            only moves points from the frontiers to the single pops: a point with theta' <= d < theta still has at most ef - 2 others
            as near, so when it is the minimum pending point the stop test lets it through (lt <= ef - 2) and cannot flag it
            (le - 1 <= ef - 2), and it is expanded as it would have been in a frontier.  The kernels take the lower edge of the
            histogram bin that holds index ef - 1 (cl_theta).

the stop test is COUNTED, not scanned.  At a single pop the frontiers have run dry: every discovered certain point is expanded, so
            every pending point is uncertain, and u is the nearest of them.  A point closer than u is therefore expanded: it is a
            certain point (d < theta' <= d_u) or an earlier single pop of this layer.  Hence
                lt = #{evaluated, d < d_u}  = ncert + #{earlier pops p : d_p < d_u}
                le = #{evaluated, d <= d_u} = lt + #{pending, d = d_u} + #{earlier pops p : d_p = d_u}
            with ncert counted at discovery (the entry point included when it is certain), the pending ties counted by the pass that
            finds u, and the earlier pops kept in a list of `pop_cap` entries.  A pop that finds the list full flags the query
            (`cap_hit`): the product re-runs it with the sequential kernels, which is exact.
"""
import collections

import numpy as np

from tests.closure_model import LayerState

BoundInfo = collections.namedtuple("BoundInfo", "cap_hit tied_with_earlier_pop entry_uncertain")


def closure_bound_layer(rows, dist, ep, ef, visited, theta_b, pop_cap=None):
    """theta_b: any value <= closure_model.theta_of(row, ef) (None = +inf, valid only where theta_of gives None); returns
    (LayerState, BoundInfo).  LayerState.hazard is the tie flag or the full pop list."""
    visited = set(visited)
    visited.add(ep)
    evaluated, expanded_set = {ep}, set()
    evals, expanded, rounds = 1, 0, 0
    popped = []                                          # (distance, id) of this layer's single pops
    tied_with_earlier_pop = False

    def certain(p):
        return theta_b is None or dist[p] < theta_b

    ncert = 1 if certain(ep) else 0

    def expand(frontier):
        nonlocal evals, expanded, ncert
        nxt = []
        for f in frontier:
            expanded_set.add(f)
            row = rows.get(f, ())
            if len(row):
                expanded += 1
            for e in row:
                e = int(e)
                if e in visited:
                    continue
                visited.add(e)
                evaluated.add(e)
                evals += 1
                if certain(e):
                    ncert += 1
                    nxt.append(e)
        return nxt

    frontier = [ep] if certain(ep) else []
    hazard = cap_hit = False
    for _ in range(len(dist) + 2):
        while frontier:
            rounds += 1
            frontier = expand(frontier)
        pending = evaluated - expanded_set
        if not pending:
            break
        # ONE pass over the pending points: the minimum in the candidates heap's order, and how many tie with it
        u = min(pending, key=lambda p: (dist[p], -p))
        ties_pending = sum(1 for p in pending if dist[p] == dist[u])
        lt = ncert + sum(1 for d, _ in popped if d < dist[u])
        ties_popped = sum(1 for d, _ in popped if d == dist[u])
        tied_with_earlier_pop |= ties_popped > 0
        le = lt + ties_pending + ties_popped
        if lt >= ef:
            break
        if le - 1 >= ef:
            hazard = True
            break
        if pop_cap is not None and len(popped) >= pop_cap:
            hazard = cap_hit = True
            break
        popped.append((dist[u], u))
        frontier = expand([u])
    nearest = min(evaluated, key=lambda p: (dist[p], p))
    return (LayerState(visited, evals, expanded, nearest, hazard, rounds, len(popped)),
            BoundInfo(cap_hit, tied_with_earlier_pop, not certain(ep)))


NAN_KEY = 0xFFFFFFFE


def images(dist32):
    """the canonical images (rk_canon o f32_orderable) of float32 distances, as Python ints: their order is the distances', a NaN last"""
    d = np.ascontiguousarray(dist32, dtype=np.float32)
    u = d.view(np.uint32).astype(np.int64)
    img = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return [NAN_KEY if v != v else int(i) for v, i in zip(d.tolist(), img.tolist())]


def theta_bound(keys, ef):
    """cl_theta on the CPU: the lower edge of the bin that holds index ef - 1 of sorted(keys) after two histogram passes of up to
    11 bits each over the bits the key range has (None = +inf for <= ef keys).  Never above closure_model.theta_of(keys, ef)."""
    if len(keys) <= ef:
        return None
    kmin = min(keys)
    hi = (max(keys) - kmin).bit_length()
    prefix, k = 0, ef - 1
    for width in (11, 11):
        if hi == 0:
            break
        bits = min(hi, width)
        lo = hi - bits
        counts = [0] * (1 << bits)
        for v in keys:
            kp = v - kmin
            if kp >> hi == prefix:
                counts[(kp >> lo) & ((1 << bits) - 1)] += 1
        digit = 0
        while k >= counts[digit]:
            k -= counts[digit]
            digit += 1
        prefix, hi = (prefix << bits) | digit, lo
    return kmin + (prefix << hi)

"""CPU model of one upper layer of BlockBasedHnsw::ann_search in two forms (no GPU, no product code).

search_layer    the reference's loop (rs/index/src/hnsw/block_based/index.rs:212-287, restated as oracle/muopdb_oracle.cpp does):
                candidates popped one at a time, nearest first, the largest id among exact ties.
closure_layer   the form mdb_hnsw_closure.hip.h runs when every distance of the layer is known up front.  With theta the ef-th
                smallest distance of the layer (index ef - 1 of the sorted row, +inf for a layer of <= ef points) a point with
                d < theta is CERTAIN: at most ef - 2 other points are as near, so it is accepted whenever it is discovered and the
                `distance > furthest` break cannot fire on it, nor on anything popped while it is pending.  Every certain point that
                is discovered is therefore expanded, in any order — whole frontiers at once — and only the uncertain rest is popped
                one at a time, with the reference's stop test restated as a count over the evaluated set.

Both return the same LayerState; everything a layer hands on is a union, a count or a minimum.  `hazard` (closure form only) marks the
one case the counts cannot decide — an uncertain pop that passes the strict test while ef other evaluated points are no farther: whether
the reference ever accepted it depends on the discovery order.  The product re-runs such a query with the sequential kernels.

Distances are any totally ordered values without NaN (the product sends a NaN to the sequential kernels before anything else).
"""
import collections
import heapq

LayerState = collections.namedtuple("LayerState", "visited evals expanded nearest hazard rounds pops")


def search_layer(rows, dist, ep, ef, visited):
    """rows[p]: neighbours of p on this layer in edge order (missing / empty: no edges); dist[p]; visited: set of points (not changed)"""
    visited = set(visited)
    visited.add(ep)
    evals, expanded = 1, 0
    cand = [(dist[ep], -ep)]          # pop: smallest distance, LARGEST id among ties (max-heap on (-d, id))
    work = [(-dist[ep], -ep)]         # top: largest (distance, id)
    while cand:
        d, nid = heapq.heappop(cand)
        if d > -work[0][0]:
            break
        row = rows.get(-nid, ())
        if len(row) == 0:
            continue
        expanded += 1
        for e in row:
            e = int(e)
            if e in visited:
                continue
            visited.add(e)
            furthest = -work[0][0]
            evals += 1
            if dist[e] < furthest or len(work) < ef:
                heapq.heappush(cand, (dist[e], -e))
                heapq.heappush(work, (-dist[e], -e))
                if len(work) > ef:
                    heapq.heappop(work)
    nearest = min((-nd, -ni) for nd, ni in work)[1]
    return LayerState(visited, evals, expanded, nearest, False, 0, 0)


def theta_of(pool, ef):
    """the ef-th smallest value of `pool` (the layer's row, or any superset of it), None = +inf when it holds <= ef values"""
    if len(pool) <= ef:
        return None
    return sorted(pool)[ef - 1]


def closure_layer(rows, dist, ep, ef, visited, theta):
    visited = set(visited)
    visited.add(ep)
    evaluated, expanded_set = {ep}, set()
    evals, expanded, rounds, pops = 1, 0, 0, 0

    def certain(p):
        return theta is None or dist[p] < theta

    def expand(frontier):
        nonlocal evals, expanded
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
                    nxt.append(e)
        return nxt

    frontier = [ep] if certain(ep) else []
    hazard = False
    for _ in range(len(dist) + 2):                       # every pass expands at least one new point
        while frontier:
            rounds += 1
            frontier = expand(frontier)
        pending = evaluated - expanded_set
        if not pending:
            break
        u = min(pending, key=lambda p: (dist[p], -p))    # the candidates heap's order
        closer = sum(1 for p in evaluated if dist[p] < dist[u])
        if closer >= ef:
            break
        if sum(1 for p in evaluated if p != u and dist[p] <= dist[u]) >= ef:
            hazard = True
            break
        pops += 1
        frontier = expand([u])
    nearest = min(evaluated, key=lambda p: (dist[p], p))
    return LayerState(visited, evals, expanded, nearest, hazard, rounds, pops)


def same(a, b):
    return a.visited == b.visited and (a.evals, a.expanded, a.nearest) == (b.evals, b.expanded, b.nearest)


def csr_rows(node_ids, indptr, edges):
    """{point: its edge list} of one layer in synth._layer_graph's CSR form"""
    return {int(p): [int(e) for e in edges[int(indptr[i]):int(indptr[i + 1])]] for i, p in enumerate(node_ids)}

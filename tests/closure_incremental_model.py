"""CPU model of the single pop's INCREMENTAL pass of mdb_hnsw_closure.hip.h (no GPU, no product code): tests/closure_bound_model.py's
closure_bound_layer with the one pass over the pending points replaced by the per-thread bookkeeping the kernels keep.

The evaluated bitmap has a word per 32 points.  A block of `nt` threads gives a word to 2^ltpw threads (the largest power of two <= 32
with words * 2^ltpw <= nt), a slice of 32 >> ltpw bits each.  Where every thread owns at most ONE slice (words << ltpw <= nt) it keeps,
across the pops of a layer,
    seen    the bits of its slice already folded
    mu      its minimum pending key (distance, -id)
    mties   pending points at that minimum distance
    me      its minimum evaluated key (distance, id)
and a pop folds only the bits evaluated since (ev & ~seen), skipping the expanded ones.  At a pop the frontiers have run dry, so
every certain point is expanded and never enters mu; the only pending points that stop being pending are the single pops, and the
thread whose slice holds the popped u forgets the slice (seen = 0, mu = max, mties = 0) and walks it again at the next pop.  Ties of u
owned by other threads stay folded.  All four values are reset at every layer (a call of this function is one layer).  With more
slices than threads every thread walks all its slices at every pop, mu and mties from nothing: the form before this one.

`trace` receives, per pop, what the block decided (u, lt, le) together with the sets it stood on, so that a test can hold every pop
against the scan over the pending set.
"""
from tests.closure_bound_model import BoundInfo
from tests.closure_model import LayerState

KEY_MAX = (float("inf"), 0)


def slices(n, nt, words=None):
    """(words, ltpw, bits per slice, every thread owns at most one slice); words: the bitmap's size where it is not the n bits rounded up"""
    words = (n + 31) // 32 if words is None else words
    assert 32 * words >= n
    ltpw = 0
    while ltpw < 5 and (words << (ltpw + 1)) <= nt:
        ltpw += 1
    return words, ltpw, 32 >> ltpw, (words << ltpw) <= nt


class _Thread:
    __slots__ = ("seen", "mu", "mties", "me")

    def __init__(self):
        self.seen, self.mu, self.mties, self.me = 0, KEY_MAX, 0, KEY_MAX

    def fold(self, first, bits, dist, expanded_set):
        """the points first + b of the set bits b: every one into me, the unexpanded ones into mu and mties"""
        b = 0
        while bits >> b:
            if (bits >> b) & 1:
                c = first + b
                self.me = min(self.me, (dist[c], c))
                if c not in expanded_set:
                    d = dist[c]
                    self.mties = 1 if d < self.mu[0] else self.mties + (1 if d == self.mu[0] else 0)
                    self.mu = min(self.mu, (d, -c))
            b += 1


def new_threads(nt):
    return [_Thread() for _ in range(nt)]


def closure_incremental_layer(rows, dist, ep, ef, visited, theta_b, nt, pop_cap=None, trace=None, threads=None, words=None):
    """one layer over the points 0 .. len(dist) - 1 by a block of `nt` threads; returns (LayerState, BoundInfo) as closure_bound_layer does.
    threads: None, as the kernels do it — every layer starts from fresh values; a test hands in the list a layer above used (new_threads)
    to show that values that survive a layer can be told"""
    n = len(dist)
    words, ltpw, wbits, own_one = slices(n, nt, words)
    wmask = (1 << wbits) - 1
    visited = set(visited)
    visited.add(ep)
    ev = [0] * words                                     # the evaluated bitmap; the expanded one is `expanded_set`
    ev[ep >> 5] |= 1 << (ep & 31)
    evaluated, dirty = {ep}, set(range(words))          # the bitmap's points as a set, for `trace`; words to look at in the next pass
    expanded_set = set()
    evals, expanded, rounds = 1, 0, 0
    popped = []
    tied_with_earlier_pop = False
    if threads is None:
        threads = new_threads(nt)                        # (reset at every layer: a new set per call)

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
                ev[e >> 5] |= 1 << (e & 31)
                evaluated.add(e)
                dirty.add(e >> 5)
                evals += 1
                if certain(e):
                    ncert += 1
                    nxt.append(e)
        return nxt

    frontier = [ep] if certain(ep) else []
    hazard = cap_hit = False
    for _ in range(n + 2):
        while frontier:
            rounds += 1
            frontier = expand(frontier)
        # ---- the pass
        if own_one:
            # (only the threads of the words written since the last pass, or forgotten then, have anything to fold)
            for t in sorted(t for w in dirty for t in range(w << ltpw, (w + 1) << ltpw)):
                th = threads[t]
                w, b0 = t >> ltpw, (t & ((1 << ltpw) - 1)) * wbits
                new = ((ev[w] >> b0) & wmask) & ~th.seen
                th.seen |= new
                th.fold(32 * w + b0, new, dist, expanded_set)
            dirty.clear()
        else:
            for t in range(nt):
                th = threads[t]
                th.mu, th.mties = KEY_MAX, 0             # (me runs on: the evaluated set only grows)
                for item in range(t, words << ltpw, nt):
                    w, b0 = item >> ltpw, (item & ((1 << ltpw) - 1)) * wbits
                    th.fold(32 * w + b0, (ev[w] >> b0) & wmask, dist, expanded_set)
        ukey = min(th.mu for th in threads)
        nearest = min(th.me for th in threads)[1]
        if ukey == KEY_MAX:
            break
        du, u = ukey[0], -ukey[1]
        ties_pending = sum(th.mties for th in threads if th.mties and th.mu[0] == du)
        lt = ncert + sum(1 for d in popped if d < du)
        ties_popped = sum(1 for d in popped if d == du)
        tied_with_earlier_pop |= ties_popped > 0
        le = lt + ties_pending + ties_popped
        if trace is not None:
            trace.append(dict(u=u, lt=lt, le=le, evaluated=set(evaluated), expanded=set(expanded_set), nearest=nearest))
        if lt >= ef:
            break
        if le - 1 >= ef:
            hazard = True
            break
        if pop_cap is not None and len(popped) >= pop_cap:
            hazard = cap_hit = True
            break
        popped.append(du)
        if own_one:                                      # the owner of u's slice forgets it
            owner = threads[((u >> 5) << ltpw) + ((u & 31) >> (5 - ltpw))]
            owner.seen, owner.mu, owner.mties = 0, KEY_MAX, 0
            dirty.add(u >> 5)
        frontier = expand([u])
    return (LayerState(visited, evals, expanded, nearest, hazard, rounds, len(popped)),
            BoundInfo(cap_hit, tied_with_earlier_pop, not certain(ep)))

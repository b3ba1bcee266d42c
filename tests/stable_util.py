"""Stable RB matching restated in NumPy (include/d2d_stable.h), for the tests of the kernel.

The semantics, once more.  link_pref, rb_pref: float32 [M, R] (row = link, column = RB), higher is better; quota int [R], each in
[0, M], 0: the RB is closed.  A pair (a, r) is ACCEPTABLE iff both entries are finite.  Link a ranks its acceptable RBs by
(link_pref descending, r ascending), RB r the links by (rb_pref descending, a ascending); comparisons are float32 comparisons, so
+0.0 and -0.0 tie and the index decides.  The result is the link-optimal stable matching of the college-admissions problem these
orders and quotas define: col int32 [M] (-1: unmatched), load int32 [R], proposals (the sum over the rows of the 1-based position of
col in the row's acceptable order, an unmatched row counting the length of its order) and unmatched.

Two restatements of deferred acceptance - `sequential` (one free link at a time, the lowest index first) and `rounds` (every free
link at once) - which must agree exactly, because the link-proposing result and its set of proposals do not depend on the order
(McVitie and Wilson 1971); a brute-force finder of blocking pairs that compares the floats themselves, not the orders; an enumerator
of every stable matching of a tiny instance; and the table of the GPU tests' cases.
"""
import heapq
import itertools
from typing import NamedTuple

import numpy as np


class Matching(NamedTuple):
    col: np.ndarray            # int32 [M]
    load: np.ndarray           # int32 [R]
    proposals: int
    unmatched: int


def acceptable(link_pref, rb_pref):
    return np.isfinite(link_pref) & np.isfinite(rb_pref)


def orders(link_pref, rb_pref):
    """(lists, rank): lists[a] the acceptable RBs of link a, best first; rank[a, r] the place of link a in RB r's order (0: the
    best) - among acceptable links the only places that are ever compared."""
    m, r = link_pref.shape
    ok = acceptable(link_pref, rb_pref)
    by_link = np.lexsort((np.broadcast_to(np.arange(r), (m, r)), -link_pref), axis=1)        # stable in r: -(+0.0) == +0.0 ties
    lists = [[int(c) for c in by_link[a] if ok[a, c]] for a in range(m)]
    by_rb = np.lexsort((np.broadcast_to(np.arange(m)[:, None], (m, r)), -rb_pref), axis=0)
    rank = np.empty((m, r), dtype=np.int64)
    rank[by_rb, np.arange(r)[None, :]] = np.arange(m)[:, None]
    return lists, rank


def _result(col, quota, lists):
    m, r = len(col), len(quota)
    load = np.bincount(col[col >= 0], minlength=r).astype(np.int32)
    assert (load <= quota).all()
    return np.asarray(col, dtype=np.int32), load


def sequential(link_pref, rb_pref, quota) -> Matching:
    """Deferred acceptance, one proposal at a time: the free link of the lowest index that has an RB left proposes to the next RB
    of its order; an RB under quota holds it, a full one keeps the better of it and its worst holder.  Counts the proposals."""
    m, r = link_pref.shape
    quota = np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,))
    lists, rank = orders(link_pref, rb_pref)
    nxt = [0] * m
    col = np.full(m, -1, dtype=np.int64)
    holders = [[] for _ in range(r)]                  # heaps of (-rank, link): the worst holder on top
    free = [a for a in range(m) if lists[a]]
    heapq.heapify(free)
    made = 0
    while free:
        a = heapq.heappop(free)
        c = lists[a][nxt[a]]
        nxt[a] += 1
        made += 1
        out = a
        if len(holders[c]) < quota[c]:
            heapq.heappush(holders[c], (-rank[a, c], a)); col[a] = c; out = -1
        elif quota[c] > 0 and rank[a, c] < -holders[c][0][0]:
            out = heapq.heapreplace(holders[c], (-rank[a, c], a))[1]; col[a] = c; col[out] = -1
        if out >= 0 and nxt[out] < len(lists[out]):
            heapq.heappush(free, out)
    col, load = _result(col, quota, lists)
    return Matching(col, load, made, int((col < 0).sum()))


def rounds(link_pref, rb_pref, quota) -> Matching:
    """Deferred acceptance in synchronous rounds: every free link with an RB left proposes at once; every RB keeps the best quota of
    (holders, proposers) by its order.  proposals is computed from the result, as the header defines it."""
    m, r = link_pref.shape
    quota = np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,))
    lists, rank = orders(link_pref, rb_pref)
    nxt = [0] * m
    col = np.full(m, -1, dtype=np.int64)
    while True:
        asked = {}
        for a in range(m):
            if col[a] < 0 and nxt[a] < len(lists[a]):
                asked.setdefault(lists[a][nxt[a]], []).append(a)
                nxt[a] += 1
        if not asked:
            break
        for c, who in asked.items():
            pool = sorted([int(a) for a in np.nonzero(col == c)[0]] + who, key=lambda a: rank[a, c])
            col[pool[:quota[c]]] = c
            col[pool[quota[c]:]] = -1
    made = sum(len(lists[a]) if col[a] < 0 else lists[a].index(col[a]) + 1 for a in range(m))
    col, load = _result(col, quota, lists)
    return Matching(col, load, int(made), int((col < 0).sum()))


def solve_batch(link_pref, rb_pref, quota, how=sequential):
    """(col [B, M], load [B, R], proposals [B], unmatched [B]) int32 of [B, M, R] tensors, env by env."""
    res = [how(link_pref[b], rb_pref[b], quota) for b in range(link_pref.shape[0])]
    return (np.stack([x.col for x in res]), np.stack([x.load for x in res]), np.array([x.proposals for x in res], dtype=np.int32),
            np.array([x.unmatched for x in res], dtype=np.int32))


def blocking_pairs(link_pref, rb_pref, quota, col):
    """Every pair (a, r) that blocks the matching `col`, by brute force on the float32 values themselves: (a, r) is acceptable, a
    prefers r to its match or is unmatched, and r is under quota or prefers a to its worst holder."""
    m, r = link_pref.shape
    quota = np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,))
    ok = acceptable(link_pref, rb_pref)
    link_prefers = lambda a, c, d: link_pref[a, c] > link_pref[a, d] or (link_pref[a, c] == link_pref[a, d] and c < d)
    rb_prefers = lambda c, a, e: rb_pref[a, c] > rb_pref[e, c] or (rb_pref[a, c] == rb_pref[e, c] and a < e)
    found = []
    for a in range(m):
        for c in range(r):
            if not ok[a, c] or col[a] == c or quota[c] == 0:
                continue
            if col[a] >= 0 and not link_prefers(a, c, col[a]):
                continue
            held = [e for e in range(m) if col[e] == c]
            if len(held) < quota[c] or any(rb_prefers(c, a, e) for e in held):
                found.append((a, c))
    return found


def feasible(link_pref, rb_pref, quota, col) -> bool:
    """Every matched pair is acceptable and no RB is over its quota."""
    m, r = link_pref.shape
    quota = np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,))
    ok = acceptable(link_pref, rb_pref)
    col = np.asarray(col)
    on = col >= 0
    return bool((col < r).all() and ok[np.nonzero(on)[0], col[on]].all() and (np.bincount(col[on], minlength=r) <= quota).all())


def all_stable_matchings(link_pref, rb_pref, quota):
    """Every stable matching of a tiny instance: all (R + 1)^M placements, kept if feasible and free of blocking pairs."""
    m, r = link_pref.shape
    return [np.array(col) for col in itertools.product(range(-1, r), repeat=m)
            if feasible(link_pref, rb_pref, quota, col) and not blocking_pairs(link_pref, rb_pref, quota, col)]


def link_weakly_prefers(link_pref, a, c, d) -> bool:
    """Link a likes column c at least as much as column d (-1: unmatched, the worst)."""
    if c == d or d < 0:
        return True
    if c < 0:
        return False
    return bool(link_pref[a, c] > link_pref[a, d] or (link_pref[a, c] == link_pref[a, d] and c < d))


# ------------------------------------------------------------------------------------------ instances
NON_FINITE = (np.nan, np.inf, -np.inf)
ALPHABET = np.array([-0.0, 0.0, 1.0], dtype=np.float32)             # three values, both zeros among them: heavy ties


def random_instance(rng, m, r, alphabet=None, holes=0.15, popular=0.0):
    """(link_pref, rb_pref) float32 [M, R]: values of the alphabet (None: normals rounded to one decimal, which ties too and has
    both zeros), with entries that are not finite - of every kind - sprinkled into both tensors.  popular > 0 adds a popularity
    of that spread, common to all rows, to every column of both tensors before the rounding: the links contend for the same RBs,
    the RBs for the same links, and there are rejections to make."""
    def plane(common):
        x = rng.choice(alphabet, (m, r)) if alphabet is not None else np.round(rng.normal(size=(m, r)) + popular * common, 1)
        x = x.astype(np.float32)
        hole = rng.random((m, r)) < holes
        x[hole] = rng.choice(NON_FINITE, int(hole.sum()))
        return x
    return plane(rng.normal(size=(1, r))), plane(rng.normal(size=(m, 1)))


# the GPU tests' cases: name -> (B, M, R, quota, what the preferences are).  'random': normals with a popularity per RB and per link,
# rounded to one decimal, with the common perturbations (entries that are not finite in both tensors, row M // 2 of env 0 wholly unacceptable, the last env wholly
# unacceptable where B >= 2); 'identical': every link has the order 0, 1, 2, ... and every RB likes the lower link better - link a
# is rejected a times; 'equal': every entry a zero of random sign.
CASES = {
    'smallest': (3, 1, 1, 1, 'random'),
    'closed_rb': (2, 5, 3, [2, 1, 0], 'random'),
    'wave_edge': (4, 64, 64, 1, 'random'),
    'wave_edge_odd': (2, 65, 63, 1, 'random'),
    'more_rows_than_threads': (2, 257, 100, 3, 'random'),
    'many_per_rb': (1, 300, 7, 50, 'random'),
    'several_passes': (1, 40, 4101, 1, 'random'),
    'row_limit': (1, 2048, 256, 8, 'random'),
    'rejection_chain': (2, 128, 128, 1, 'identical'),
    'pure_index_order': (2, 50, 25, 2, 'equal'),
}


def dead_env(rng, m, r):
    """An env without an acceptable pair whose tensors still hold finite values: every pair has a hole in one tensor or the other."""
    lp, rp = (np.round(rng.normal(size=(m, r)), 1).astype(np.float32) for _ in range(2))
    side = rng.random((m, r)) < 0.5
    side.flat[0] = False                              # rb_pref has a hole even in an env of one pair
    lp[side] = rng.choice(NON_FINITE, int(side.sum()))
    rp[~side] = rng.choice(NON_FINITE, int((~side).sum()))
    return lp, rp


def case(name):
    """(link_pref, rb_pref float32 [B, M, R], quota int32 [R]) of a row of CASES, the same arrays on every call."""
    b, m, r, quota, what = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 2024)
    quota = np.broadcast_to(np.asarray(quota, dtype=np.int32), (r,)).copy()
    if what == 'identical':
        lp = np.broadcast_to(-np.arange(r, dtype=np.float32)[None, None, :], (b, m, r)).copy()
        rp = np.broadcast_to(-np.arange(m, dtype=np.float32)[None, :, None], (b, m, r)).copy()
        return lp, rp, quota
    if what == 'equal':
        zeros = lambda: np.where(rng.random((b, m, r)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        return zeros(), zeros(), quota
    lp, rp = (np.stack(x) for x in zip(*(random_instance(rng, m, r, holes=0.05, popular=1.5) for _ in range(b))))
    lp[0, m // 2] = rng.choice(NON_FINITE, r)                           # a wholly unacceptable row
    if b >= 2:
        lp[b - 1], rp[b - 1] = dead_env(rng, m, r)                       # a wholly unacceptable env among live ones
    return lp, rp, quota

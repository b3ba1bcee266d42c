"""The NumPy restatement of the conflict-graph RB colouring (include/d2d_color.h): the conflict graph in float32, the turns in
integers, no float64 anywhere - so that the kernel's outputs are compared for equality - and the synthetic cases the CPU and the
GPU tests share."""
from types import SimpleNamespace

import numpy as np


def conflict_graph(score, tx_bias, rx_thr):
    """bool [N, N] of one env: {i, j} is an edge iff i != j and (d(i<-j) or d(j<-i)), d(i<-j) = score[i, j] + tx_bias[j] >= rx_thr[i]
    in float32 (one addition, none with tx_bias None); a NaN on either side compares false."""
    score, rx_thr = np.asarray(score), np.asarray(rx_thr)
    assert score.dtype == np.float32 and rx_thr.dtype == np.float32 and score.shape == rx_thr.shape * 2
    with np.errstate(invalid='ignore', over='ignore'):
        x = score if tx_bias is None else score + np.asarray(tx_bias, dtype=np.float32)[None, :]
        assert x.dtype == np.float32
        d = x >= rx_thr[:, None]
    np.fill_diagonal(d, False)
    return d | d.T


def turn_takers(n, r, movable, allowed):
    """bool [N]: movable (None: every link) and at least one allowed RB (None: every RB)."""
    turn = np.ones(n, dtype=bool) if movable is None else np.asarray(movable, dtype=bool).copy()
    if allowed is not None:
        turn &= np.asarray(allowed, dtype=bool)[:, :r].any(axis=1)
    return turn


def dsatur(adj, rb, turn, allowed, r, pack):
    """One env: (rb_out int32 [N], conflicts, rbs_used, proper).  adj bool [N, N], rb int [N] (read for the background only), turn
    bool [N], allowed bool [N, R] or None."""
    n = len(rb)
    adj = np.asarray(adj, dtype=bool)
    col = np.asarray(rb, dtype=np.int64).copy()
    deg = adj.sum(axis=1).astype(np.int64)
    coloured = ~turn
    on = coloured & (col >= 0) & (col < r)
    col[turn] = -1
    load = np.bincount(col[on], minlength=r).astype(np.int64)
    member = np.zeros((n, r), dtype=np.int64)
    member[np.nonzero(on)[0], col[on]] = 1
    nb = adj.astype(np.int64) @ member              # nb[v, q]: the coloured neighbours of v on RB q
    sat = (nb > 0).sum(axis=1)
    every = np.arange(r)
    for _ in range(int(turn.sum())):
        cand = turn & ~coloured
        v = int(np.argmax(np.where(cand, sat * (n + 1) + deg, -1)))     # the largest (sat, deg); argmax keeps the lowest index
        ok = every if allowed is None else np.nonzero(np.asarray(allowed[v], dtype=bool)[:r])[0]
        key = (nb[v, ok] * (n + 1) + (0 if pack else load[ok])) * r + ok
        q = int(ok[np.argmin(key)])
        col[v] = q
        coloured[v] = True
        load[q] += 1
        fresh = adj[v] & (nb[:, q] == 0)
        sat[fresh] += 1
        nb[adj[v], q] += 1
    on = (col >= 0) & (col < r)
    same = adj & (col[:, None] == col[None, :]) & on[:, None] & on[None, :] & (turn[:, None] | turn[None, :])
    conflicts = int(np.triu(same, 1).sum())
    return col.astype(np.int32), conflicts, len(np.unique(col[turn])), int(conflicts == 0)


def color_graph(score, tx_bias, rx_thr, rb, r, movable=None, allowed=None, pack=False):
    """Every env: (rb_out int32 [B, N], conflicts int32 [B], rbs_used int32 [B], proper uint8 [B]) - what d2d_color_graph writes."""
    b, n = rb.shape
    turn = turn_takers(n, r, movable, allowed)
    res = [dsatur(conflict_graph(score[e], None if tx_bias is None else tx_bias[e], rx_thr[e]), rb[e], turn, allowed, r, pack)
           for e in range(b)]
    return (np.stack([x[0] for x in res]), np.asarray([x[1] for x in res], dtype=np.int32),
            np.asarray([x[2] for x in res], dtype=np.int32), np.asarray([x[3] for x in res], dtype=np.uint8))


def from_adjacency(adj):
    """(score float32 [1, N, N], rx_thr float32 [1, N]) whose conflict graph is adj (made symmetric): 1 on the edges against 0.5."""
    a = np.asarray(adj, dtype=bool)
    return (a | a.T).astype(np.float32)[None], np.full((1, len(a)), 0.5, dtype=np.float32)


def color_adjacency(adj, r, pack, rb=None, movable=None, allowed=None):
    """dsatur() of one adjacency matrix through the float32 front door; rb None: every link on RB 0 before."""
    score, thr = from_adjacency(adj)
    rb = np.zeros((1, len(adj)), dtype=np.int32) if rb is None else np.asarray(rb, dtype=np.int32)[None]
    out = color_graph(score, None, thr, rb, r, movable, allowed, pack)
    return out[0][0], int(out[1][0]), int(out[2][0]), int(out[3][0])


def same_rb_edges(adj, col, turn, r):
    """The definition of `conflicts` by a plain double loop: edges with an end that took a turn and both ends on one RB in [0, R)."""
    n, found = len(col), 0
    for i in range(n):
        for j in range(i + 1, n):
            if adj[i, j] and (turn[i] or turn[j]) and col[i] == col[j] and 0 <= col[i] < r:
                found += 1
    return found


def lds_bytes(n, r, allowed):
    """The header's formula, restated."""
    r16 = lambda x: (x + 15) // 16 * 16
    w, words = (n + 31) // 32, (r + 31) // 32
    return r16(4 * n * w) + (1 + bool(allowed)) * r16(4 * n * words) + 3 * r16(4 * n) + 2 * r16(4 * r) + r16(4 * words) + 64


# the synthetic cases of the GPU comparison - (B, N, R): what varies with it.  half: every second link movable; bg: the RBs the
# background holds beside 0 .. R - 1; masked: an allowed mask with empty rows; bias: with a tx_bias plane
SHAPES = {
    (1, 2, 1): dict(half=False, masked=False, bias=False, density=0.5),
    (3, 37, 5): dict(half=True, masked=True, bias=True, density=0.15),
    (2, 64, 32): dict(half=False, masked=False, bias=True, density=0.3),
    (2, 65, 33): dict(half=True, masked=True, bias=False, density=0.3),
    (2, 300, 40): dict(half=True, masked=True, bias=True, density=0.1),
    (1, 800, 24): dict(half=False, masked=False, bias=True, density=0.02),
}


def synthetic(b, n, r, seed=None, **how):
    """The inputs of a SHAPES case on the host (or of any shape, with `how` giving what SHAPES would): scores drawn so that about
    `density` of the directed pairs conflict, thresholds and biases that vary by link, background RBs that include -1, R and R + 5."""
    o = how or SHAPES[(b, n, r)]
    rng = np.random.default_rng(1000 * n + r if seed is None else seed)
    score = rng.normal(size=(b, n, n)).astype(np.float32)
    bias = (0.25 * rng.normal(size=(b, n))).astype(np.float32) if o['bias'] else None
    # P(normal >= t) = density at t = the normal quantile; scattered a little per receiver
    from statistics import NormalDist
    t = NormalDist().inv_cdf(1.0 - o['density'])
    thr = (t + 0.1 * rng.normal(size=(b, n))).astype(np.float32)
    rb = rng.integers(0, r, size=(b, n)).astype(np.int32)
    rb[:, 0::7] = -1
    rb[:, 3::7] = r
    rb[:, 5::7] = r + 5
    movable = None
    if o['half']:
        movable = np.zeros(n, dtype=bool)
        movable[0::2] = True
    allowed = None
    if o['masked']:
        allowed = rng.random((n, r)) < 0.6
        allowed[2::5] = False                                           # empty rows: those links are background
        allowed[4::9] = False
        allowed[4::9, r - 1] = True                                     # one allowed RB, the last bit of the last word
    return SimpleNamespace(b=b, n=n, r=r, score=score, tx_bias=bias, rx_thr=thr, rb=rb, movable=movable, allowed=allowed)

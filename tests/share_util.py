"""What the exact RB sharing tests share (test_share_cpu.py, test_gpu_share.py): the NumPy restatement of the solver kernel, brute
force over all R^M placements, the float64 reference of the value block on read_side_util.pair_pl_db, and the seeded cases of the
direct launches of csrc/d2d_share.hip.

The restatement (solve_ref) is the recurrence include/d2d_share.h states, vectorised over the targets T for each S, S ascending
with a strict >, so that equal sums stay with the lowest S.  Every candidate is one float64 addition and max is exact, so the kernel,
which evaluates them in another order, must give the same words.

The reference block (values_ref) is the simulator's definition (simulator.py:93-151) as evaluate_util.evaluate_ref states it: on RB
r under subset S the members are the background links of r and the movable links of S, each member's interference is the sum over
the other members, and the entry is the sum of the members' capacities."""
import itertools
from functools import lru_cache

import numpy as np

import evaluate_util as evu
import read_side_util as rsu

BAR = rsu.BAR                                # |d| <= BAR max(|ref|, 1) on a value (Mbps)
THRESHOLD_DB = evu.THRESHOLD_DB              # an SINR this close to the sensitivity flips a whole capacity: the entry is not compared
THRESHOLD_CAP = evu.THRESHOLD_CAP            # ... at most this share of a case
MAX_MOVABLE, MAX_BACKGROUND = 12, 64         # include/d2d_share.h


def popcount(x):
    x = np.asarray(x, dtype=np.int64)
    n = np.zeros_like(x)
    for bit in range(16):
        n += (x >> bit) & 1
    return n


# ------------------------------------------------------------------------------------------ the solver
def solve_ref(values, quota=None):
    """(col int32 [B, M], value float64 [B], feasible int32 [B]) of a float64 block [B, R, 2^M]; quota None, an int or [R] ints."""
    v = np.asarray(values, dtype=np.float64)
    b, r, nt = v.shape
    m = nt.bit_length() - 1
    assert nt == 1 << m and m >= 1
    q = np.full(r, m) if quota is None else np.maximum(np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,)), 0)
    targets = np.arange(nt)
    pop = popcount(targets)
    g = np.full((b, nt), -np.inf)
    g[:, 0] = 0.0
    choice = np.zeros((b, r, nt), dtype=np.int64)
    with np.errstate(invalid='ignore', over='ignore'):
        for layer in range(r):
            best = np.full((b, nt), -np.inf)
            for s in range(nt):
                if pop[s] > q[layer]:
                    continue
                f = v[:, layer, s]
                ok = np.isfinite(f)                                      # what is not finite is never chosen
                if not ok.any():
                    continue
                t = targets[(targets & s) == s]
                cand = np.where(ok[:, None], g[:, t ^ s] + f[:, None], -np.inf)          # ONE addition per candidate
                better = cand > best[:, t]                               # strict: equal sums stay with the lower S
                rows, cols = np.nonzero(better)
                best[rows, t[cols]] = cand[rows, cols]
                choice[rows, layer, t[cols]] = s
            g = best
    top = g[:, nt - 1]
    feasible = (top > -np.inf).astype(np.int32)
    col = np.full((b, m), -1, dtype=np.int32)
    for e in np.nonzero(feasible)[0]:
        t = nt - 1
        for layer in range(r - 1, -1, -1):
            s = int(choice[e, layer, t])
            for a in range(m):
                if (s >> a) & 1:
                    col[e, a] = layer
            t ^= s
        assert t == 0
    return col, np.where(feasible == 1, top, 0.0), feasible


def brute_force(values, quota=None):
    """(best value or None, the placements [R^M][M] that reach it) of ONE float64 block [R, 2^M], by enumeration.  The value of a
    placement is the chain the recurrence makes: ((0.0 + f_0[S_0]) + f_1[S_1]) + ... in RB order, every S_r admissible."""
    v = np.asarray(values, dtype=np.float64)
    r, nt = v.shape
    m = nt.bit_length() - 1
    q = np.full(r, m) if quota is None else np.maximum(np.broadcast_to(np.asarray(quota, dtype=np.int64), (r,)), 0)
    best, where = None, []
    for cols in itertools.product(range(r), repeat=m):
        total, ok = 0.0, True
        for layer in range(r):
            s = sum(1 << a for a in range(m) if cols[a] == layer)
            f = v[layer, s]
            if not np.isfinite(f) or bin(s).count('1') > q[layer]:
                ok = False
                break
            total = total + f
        if not ok:
            continue
        if best is None or total > best:
            best, where = total, [cols]
        elif total == best:
            where.append(cols)
    return best, where


def random_block(rng, b, r, m, kind='continuous', holes=0.1):
    """A float64 block [B, R, 2^M]: 'continuous' normal values (maxima unique almost surely), 'integers' small integers (ties
    abound), 'equal' one value everywhere (every tie); a share `holes` of the entries -inf, NaN or +inf, none of them at S = 0, so
    that every RB can stay without a movable link."""
    nt = 1 << m
    if kind == 'continuous':
        v = rng.normal(10.0, 4.0, (b, r, nt))
    elif kind == 'integers':
        v = rng.integers(0, 3, (b, r, nt)).astype(np.float64)
    else:
        v = np.full((b, r, nt), 2.5)
    if holes:
        hole = rng.random((b, r, nt)) < holes
        hole[:, :, 0] = False
        v[hole] = rng.choice([-np.inf, np.nan, np.inf], int(hole.sum()))
    return v


# name -> (B, R, M, kind, quota): the direct launches of the solver.  M = 1, 6, 7, 12; R = 1, 2, 25, 300; B = 1 and 70
SOLVE_CASES = {
    'smallest': (1, 1, 1, 'continuous', None),
    'one_bit_300_rbs': (70, 300, 1, 'continuous', 1),                   # the layer loop and the choice block past 256
    'one_wave': (70, 2, 6, 'continuous', None),                          # 64 targets: one wave, every lane a low part
    'two_waves_25_rbs': (70, 25, 7, 'integers', 2),                      # ties and quotas
    'two_waves_300_rbs': (1, 300, 7, 'continuous', 3),
    'limit': (1, 5, 12, 'continuous', None),                             # 96 KiB of layers, 1024 threads
    'limit_ties': (1, 2, 12, 'integers', 7),
    'every_tie': (2, 25, 6, 'equal', None),                              # all values equal: everybody on RB 0 by the lowest-S rule
    'one_open_rb': (3, 5, 6, 'continuous', (0, 0, 6, 0, 0)),             # quota 0 on every RB but one
    'quota_short': (2, 3, 7, 'continuous', 2),                           # quotas sum to 6 < 7: infeasible
    'dead_between': (3, 4, 6, 'continuous', None),                       # env 1 has an RB without an admissible subset
}


@lru_cache(maxsize=None)
def solve_case(name):
    """(values float64 [B, R, 2^M], quota) of a SOLVE_CASES entry, seeded; the same arrays on every call."""
    b, r, m, kind, quota = SOLVE_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    holes = 0.0 if name in ('smallest', 'every_tie', 'one_open_rb') else 0.1
    v = random_block(rng, b, r, m, kind, holes)
    if name == 'dead_between':
        v[1, 2] = rng.choice([-np.inf, np.nan, np.inf], 1 << m)         # RB 2 of env 1: nothing is admissible, not even S = 0
    v.setflags(write=False)
    return v, quota


@lru_cache(maxsize=None)
def solve_case_ref(name):
    return solve_ref(*solve_case(name))


# ------------------------------------------------------------------------------------------ the value block, float64
def values_ref(c, links, allowed=None, pwr=None, pl=None):
    """(values float64 [B, R, 2^M], closed int [B, R], near bool [B, R, 2^M]).  c: a case of read_side_util; links: the movable
    links, ascending; allowed: bool [N, R] or None; pwr: int [B, N] in place of the case's.  near: some member's SINR lies within
    THRESHOLD_DB of its sensitivity."""
    if pwr is not None:
        c = dict(c, pwr=np.asarray(pwr))
    pl = rsu.pair_pl_db(c) if pl is None else pl
    mw, _ = rsu._received_mw(c, pl)                                       # [b, j, i], zero diagonal
    sig, noise_dbm = rsu.signal_dbm(c, pl)
    b, n, r = c['b'], c['n'], c['r']
    tx, rx = np.asarray(c['tx']), np.asarray(c['rx'])
    noise = 10.0 ** (noise_dbm / 10.0)
    bw_mhz, sens = 1e-6 * c['ocols'].bw_hz[tx], c['ocols'].sens_dbm[rx]
    rb = np.asarray(c['rb'], dtype=np.int64)
    links = np.asarray(links, dtype=np.int64)
    m, nt = len(links), 1 << len(links)
    movable = np.zeros(n, bool)
    movable[links] = True
    subsets = np.arange(nt)
    values = np.zeros((b, r, nt))
    near = np.zeros((b, r, nt), bool)
    closed = np.zeros((b, r), dtype=np.int64)
    for e in range(b):
        for layer in range(r):
            bg = np.nonzero(~movable & (rb[e] == layer))[0]
            closed[e, layer] = len(bg) > MAX_BACKGROUND
            union = np.sort(np.concatenate([bg, links]))
            bit = np.full(n, -1)
            bit[links] = np.arange(m)
            on = np.where(bit[union][None, :] < 0, True, ((subsets[:, None] >> np.maximum(bit[union], 0)[None, :]) & 1) == 1)   # [S, p]
            if closed[e, layer]:
                on = on[:1]
            ix = on.astype(np.float64) @ mw[e][np.ix_(union, union)]       # [S, i]: the members j != i into receiver i
            s = sig[e, union][None, :] - 10.0 * np.log10(ix + noise[union][None, :])
            cap = np.where(s > sens[union][None, :], bw_mhz[union][None, :] * np.log2(1.0 + 10.0 ** (s / 10.0)), 0.0)
            row = (cap * on).sum(axis=1)
            near_row = ((np.abs(s - sens[union][None, :]) <= THRESHOLD_DB) & on).any(axis=1)
            if closed[e, layer]:
                row = np.concatenate([row, np.full(nt - 1, -np.inf)])
                near_row = np.concatenate([near_row, np.zeros(nt - 1, bool)])
            if allowed is not None:
                forbid = sum(1 << a for a in range(m) if not allowed[links[a], layer])
                row = np.where(subsets & forbid, -np.inf, row)
            values[e, layer], near[e, layer] = row, near_row
    return values, closed, near


def placement_total(values, cols):
    """The sum of values [R, 2^M] along the placement cols [M] (the RB of mask bit a), in RB order."""
    r, nt = values.shape
    total = 0.0
    for layer in range(r):
        total += values[layer, sum(1 << a for a, col in enumerate(cols) if col == layer)]
    return total


# name -> (B, cues, due pairs, R, M): the direct launches of the value kernel, N = cues + due pairs
VALUE_CASES = {
    'one_link': (3, 3, 6, 3, 1),
    'one_wave': (2, 5, 15, 4, 6),                # 64 subsets: one wave
    'two_waves': (2, 6, 15, 4, 7),
    'limit': (1, 10, 30, 5, 12),                 # 4096 subsets, sixteen per thread
    'closed': (2, 100, 200, 7, 5),               # RB 0: exactly 64 background members, RB 1: 65 (closed), RB 2: none
}
LAWS = ('ld2', 'mixed', 'ld35')


@lru_cache(maxsize=None)
def value_case(name, law):
    """(case, links int32 [M], allowed bool [N, R], other powers int32 [B, N]) of a VALUE_CASES entry under a law, seeded.  The
    movable links mix CUE and DUE links; allowed leaves links[M // 2] no RB and forbids a fifth of the other pairs."""
    b, cues, dues, r, m = VALUE_CASES[name]
    c = dict(rsu.build_case(cues, dues, r, law, b=b))
    n = c['n']
    rng = np.random.default_rng(11 + sum(map(ord, name + law)))
    links = np.sort(rng.choice(n, m, replace=False)).astype(np.int32)
    if name == 'closed':
        rb = np.empty((b, n), dtype=np.int32)
        bg = np.setdiff1d(np.arange(n), links)
        for e in range(b):
            order = rng.permutation(bg)
            rb[e, order[:64]], rb[e, order[64:129]] = 0, 1
            rb[e, order[129:]] = rng.integers(3, r, len(order) - 129)
            rb[e, order[-3:]] = (-1, r, 2 ** 31 - 1)                      # background links on no RB
            rb[e, links] = rng.integers(0, r, m)                          # where the movable links are plays no part
        c = rsu.with_rb(c, rb)
    allowed = rng.random((n, r)) < 0.8
    allowed[links[m // 2]] = False
    other = rng.integers(0, 24, (b, n)).astype(np.int32)
    return c, links, allowed, other


def candidates(c, links, pwr=None):
    """(rb, pwr int32 [B, R 2^M, N]): for every (r, S) the candidate "S on r, every other movable link on RB index R (no RB), the
    background as it is", candidate r 2^M + S."""
    b, n, r = c['b'], c['n'], c['r']
    m = len(links)
    nt = 1 << m
    rb = np.repeat(np.asarray(c['rb'], dtype=np.int32)[:, None, :], r * nt, axis=1)
    on = ((np.arange(nt)[:, None] >> np.arange(m)[None, :]) & 1) == 1                       # [S, a]
    for layer in range(r):
        rb[:, layer * nt:(layer + 1) * nt, links] = np.where(on, layer, r)[None]
    p = np.asarray(c['pwr'] if pwr is None else pwr, dtype=np.int32)
    return rb, np.repeat(p[:, None, :], r * nt, axis=1)


def values_from_capacity(cap, rb_cand, r, m):
    """float64 [B, R, 2^M] from evaluate()'s float32 capacity plane [B, R 2^M, N] of candidates(): the members of r summed in
    ascending link index, one addition after the other (cumsum; a link that is no member adds 0.0, which changes nothing)."""
    b, k, n = cap.shape
    nt = 1 << m
    layer = (np.arange(k) // nt)[None, :, None]
    part = np.where(rb_cand == layer, cap.astype(np.float64), 0.0)
    return np.cumsum(part, axis=2)[:, :, -1].reshape(b, r, nt)

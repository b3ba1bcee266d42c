"""What the RB matching tests share (test_assign_cpu.py, test_gpu_assign.py): the float64 reference of the weight planes on
read_side_util.pair_pl_db, the restatement of the matching kernel's shortest-augmenting-path method, brute force for small matrices,
and the seeded cases of the direct launches of csrc/d2d_assign.hip on read_side_util.build_case.

The reference planes are the simulator's definitions (simulator.py:93-151), as evaluate_util.evaluate_ref states them: the movable
links are off the air, the background stays; own[a, r] is link a's capacity with the background members of r as its interferers,
harm[a, r] the capacity those members lose to it."""
import itertools
from functools import lru_cache

import numpy as np

import evaluate_util as evu
import read_side_util as rsu

BAR = rsu.BAR                                # |d| <= BAR max(|ref|, 1) on weights and harm (Mbps)
THRESHOLD_DB = evu.THRESHOLD_DB              # an SINR this close to the sensitivity flips a whole capacity: the entry is not compared
THRESHOLD_CAP = evu.THRESHOLD_CAP            # ... at most this share of a case
B = 2

# (cues, due pairs, RBs, law): what it exercises.  The movable links are the DUE links.
WEIGHT_CASES = (
    (1, 2, 4, 'ld35'),               # the smallest shape
    (13, 50, 64, 'mixed'),           # one wave, not full
    (15, 50, 5, 'ld2'),              # many members per RB; weights only, since M > R
    (57, 200, 259, 'ld35'),          # second pass of the 256-thread loops, R % 4 != 0, R > 256
    (100, 200, 1, 'ld2'),            # 100-member walks
    (60, 200, 4000, 'mixed'),        # mostly empty RBs
    (300, 700, 8, 'mixed'),          # past 64 KiB of LDS
)
SCATTERED = (13, 50, 64, 'mixed')    # once more with a movable mask that mixes CUE and DUE links, and with allowed
TIE_CASES = ((2, 5, 7, 'ld35'), (13, 50, 64, 'mixed'))      # objective 'own' against evaluate(), bit for bit
# the matching alone, rows x columns
SOLVE_SHAPES = ((1, 1), (1, 3), (3, 4), (64, 64), (64, 65), (200, 259), (257, 257), (5, 4000))


def lds_bytes(n, r, power_law):
    """The dynamic LDS a weights launch asks for, by the layout written in csrc/d2d_assign.hip."""
    r16 = lambda x: (x + 15) & ~15
    n4 = (n + 3) & ~3
    return 16 * n + (r16(8 * n) if power_law else 0) + 32 * n + r16(8 * n4) + 3 * r16(4 * n) + r16(4 * (r + 1))


def solve_lds_bytes(m, r):
    r16 = lambda x: (x + 15) & ~15
    return r16(8 * m) + 2 * r16(8 * r) + 2 * r16(4 * r) + r16(4 * m) + 96


def case(cues, dues, r, law):
    return rsu.build_case(cues, dues, r, law, b=B)


def due_links(c, cues):
    return np.arange(cues, c['n'], dtype=np.int32)


def scattered_movable(c):
    """(links int32 [M], allowed bool [N, R]) of the SCATTERED case: every third link from link 1 on - CUE and DUE links alike -
    and about 70 % of the entries allowed, seeded."""
    rng = np.random.default_rng(5)
    links = np.arange(1, c['n'], 3, dtype=np.int32)
    return links, rng.random((c['n'], c['r'])) < 0.7


# ------------------------------------------------------------------------------------------ the weight planes, float64
def weights_ref(c, links, pl=None):
    """(own, harm, near), float64 / float64 / bool [B, M, R].  c: a case of read_side_util (pos, tx, rx, rb, pwr, ocols, law_cols,
    b, n, r); links: the movable links, ascending.  near[b, a, r]: the SINR of link a on r, or of any background member of r with a
    added, lies within THRESHOLD_DB of its sensitivity."""
    pl = rsu.pair_pl_db(c) if pl is None else pl
    mw, _ = rsu._received_mw(c, pl)                                       # [b, j, i], zero diagonal
    sig, noise_dbm = rsu.signal_dbm(c, pl)
    b, n, r = c['b'], c['n'], c['r']
    tx, rx = np.asarray(c['tx']), np.asarray(c['rx'])
    noise = 10.0 ** (noise_dbm / 10.0)
    bw_mhz, sens = 1e-6 * c['ocols'].bw_hz[tx], c['ocols'].sens_dbm[rx]
    rb = np.asarray(c['rb'], dtype=np.int64)
    links = np.asarray(links, dtype=np.int64)
    movable = np.zeros(n, bool)
    movable[links] = True
    m = len(links)

    def cap_of(sinr_db, who):
        return np.where(sinr_db > sens[who], bw_mhz[who] * np.log2(1.0 + 10.0 ** (sinr_db / 10.0)), 0.0)
    own, harm, near = np.zeros((b, m, r)), np.zeros((b, m, r)), np.zeros((b, m, r), bool)
    for e in range(b):
        bg = np.nonzero(~movable & (rb[e] >= 0) & (rb[e] < r))[0]        # the background links on an RB
        member = np.zeros((r, len(bg)))
        member[rb[e, bg], np.arange(len(bg))] = 1.0                        # [r, k]
        # link a on r: the background members of r into its receiver
        ix_own = (member @ mw[e][np.ix_(bg, links)]).T                     # [a, r]
        s_own = sig[e, links][:, None] - 10.0 * np.log10(ix_own + noise[links][:, None])
        own[e] = cap_of(s_own, links[:, None])
        near[e] = np.abs(s_own - sens[links][:, None]) <= THRESHOLD_DB
        if not len(bg):
            continue
        # the background alone, and with link a added at every member k of its RB
        same = rb[e, bg][:, None] == rb[e, bg][None, :]
        ix_bg = (mw[e][np.ix_(bg, bg)] * same).sum(axis=0)                 # [k]; the diagonal of mw is 0
        s_without = sig[e, bg] - 10.0 * np.log10(ix_bg + noise[bg])
        s_with = sig[e, bg][None, :] - 10.0 * np.log10(ix_bg[None, :] + mw[e][np.ix_(links, bg)] + noise[bg][None, :])   # [a, k]
        loss = cap_of(s_without, bg)[None, :] - cap_of(s_with, bg[None, :])
        harm[e] = loss @ member.T
        near[e] |= ((np.abs(s_with - sens[bg][None, :]) <= THRESHOLD_DB).astype(np.float64) @ member.T) > 0
    return own, harm, near


@lru_cache(maxsize=None)
def case_ref(cues, dues, r, law):
    """weights_ref of a WEIGHT_CASES entry with the DUE links movable, computed once and left unchanged."""
    c = case(cues, dues, r, law)
    return weights_ref(c, due_links(c, cues))


@lru_cache(maxsize=None)
def scattered_ref():
    c = case(*SCATTERED)
    links, _ = scattered_movable(c)
    return weights_ref(c, links)


def background_candidate(c, links):
    """rb int32 [B, N]: the case's plane with the movable links on rb -1 - the background-only sub-case."""
    rb = np.array(c['rb'], dtype=np.int32)
    rb[:, np.asarray(links)] = -1
    return rb


def placement_candidate(c, links, cols):
    """rb int32 [B, N]: the case's plane with movable link links[a] on cols[b, a]."""
    rb = np.array(c['rb'], dtype=np.int32)
    rb[:, np.asarray(links)] = cols
    return rb


# ------------------------------------------------------------------------------------------ the matching
def solve_ref(w):
    """(col int32 [M], value float32, feasible) of ONE matrix [M, R], M <= R: the method include/d2d_assign.h states, line for
    line, in float64 - the additions and subtractions the kernel makes, in its order, so the assignment is the kernel's.  A float64
    matrix is solved as it is (a reference optimum); anything else is taken as the kernel's float32."""
    w = np.asarray(w)
    w = w if w.dtype == np.float64 else w.astype(np.float32)
    m, r = w.shape
    assert m <= r
    with np.errstate(invalid='ignore'):
        cost = np.where(np.isfinite(w), -w.astype(np.float64), np.inf)
    u, v = np.zeros(m), np.zeros(r)
    col4row, row4col = np.full(m, -1), np.full(r, -1)
    path = np.full(r, -1)
    for cur in range(m):
        shortest = np.full(r, np.inf)
        scanned = np.zeros(r, bool)
        minval, i, sink = 0.0, cur, -1
        while sink < 0:
            red = ((minval + cost[i]) - u[i]) - v
            better = ~scanned & (red < shortest)
            shortest[better] = red[better]
            path[better] = i
            j = int(np.argmin(np.where(scanned, np.inf, shortest)))        # equal values: the lowest j
            if scanned[j] or not shortest[j] < np.inf:
                return np.full(m, -1, dtype=np.int32), np.float32(0.0), 0
            minval = shortest[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        u[cur] += minval
        for j in np.nonzero(scanned)[0]:
            d = minval - shortest[j]
            if j != sink:
                u[row4col[j]] += d
            v[j] -= d
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    value = 0.0
    for a in range(m):
        value += float(w[a, col4row[a]])
    return col4row.astype(np.int32), np.float32(value), 1


def brute_force(w):
    """The largest sum of finite entries over the injective row -> column maps of a small matrix, or None if there is none."""
    w = np.asarray(w, dtype=np.float64)
    m, r = w.shape
    best = None
    for cols in itertools.permutations(range(r), m):
        vals = w[np.arange(m), cols]
        if np.isfinite(vals).all() and (best is None or vals.sum() > best):
            best = float(vals.sum())
    return best


def chain_matrix(n=65):
    """n x n: row a < n - 1 has column a (2.0) and column a + 1 (1.0), the last row has column 0 (1.0) alone.  Rows 0 .. n - 2 take
    their diagonal first; the last row's augmentation then pushes every one of them a column to the right - it passes through
    every row."""
    w = np.full((n, n), -np.inf, dtype=np.float32)
    for a in range(n - 1):
        w[a, a], w[a, a + 1] = 2.0, 1.0
    w[n - 1, 0] = 1.0
    return w


def solve_matrix(m, r, seed=0):
    """The seeded float32 matrix of a SOLVE_SHAPES entry: normal weights, a tenth of them forbidden where that leaves a matching."""
    rng = np.random.default_rng(100 * m + r + seed)
    w = rng.normal(10.0, 4.0, (m, r)).astype(np.float32)
    if r > 1:
        forbid = rng.random((m, r)) < 0.1
        forbid[np.arange(m), rng.permutation(r)[:m]] = False               # one complete matching stays
        w[forbid] = -np.inf
    return w


@lru_cache(maxsize=None)
def solve_case_ref(m, r):
    w = solve_matrix(m, r)
    return (w,) + solve_ref(w)

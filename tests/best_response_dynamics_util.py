"""What the best-response-dynamics tests share: the seeded cases, and the reference restatement of the dynamics in float64 NumPy on
the oracle's path loss (oracle/d2d_oracle.py: pair_path_loss_db and the link budget of step()), which also says which envs a
float32 comparison may legitimately decide the other way.

The dynamics (include/d2d_brdyn.h), Gauss-Seidel, per env:

    for round t = 1, 2, ...; for i = 0 .. N - 1, movable links on an RB with an allowed RB only:
        s[r] = link i's sinr_db on RB r with every other link where it is now;  best = the allowed argmax, ties to the lowest r
        gain = s[best] - s[rb_i];  if gain > min_gain_db: rb_i = best, at once
    stop after a round that moved nobody (converged) or after max_rounds rounds that each moved a link

AMBIGUITY.  The kernel's float32 values differ from the oracle's by up to the project's bar, 1e-5 max(|ref|, 1), so two values
that close may compare the other way, and the difference then propagates through the rest of the run.  With m = 2e-5 max(|top|, 1)
(a difference of two values, each off by the bar) a decision is ambiguous when
    - the link moves or may move (gain > min_gain_db - m) and a second allowed RB lies within m of the top one - exact ties among
      RBs nobody else uses aside: they are the same arithmetic on the same operands and resolve to the lowest r on both sides - or
    - |gain - min_gain_db| < m with gain != 0 (gain == 0 exactly is a link already on its best RB, or tied with it: it stays).
An env is AMBIGUOUS when any of its decisions is.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import power_control_util as pcu
from oracle import d2d_oracle as orc
from sim_util import default_links

BAR = pcu.BAR                                # the project's bar on dB quantities: |d| <= BAR max(|ref|, 1)
M = 2e-5                                     # two values, each within the bar
CAP = 0.25                                   # at most this share of a case's envs may be ambiguous
B = 64
MIN_GAIN_DB, MAX_ROUNDS = 3.0, 8             # the oracle comparison's setting
BIG_MOVABLE = (0, 31, 32, 63, 64, 255, 256, 1023, 1024, 1500, 2046, 2047)       # word edges and the ends of 2048 links

# name: (cues, due pairs, R, law, cell radius m), then optionally a dict: b (envs; large shapes take 4 to 8, not 64), seed, movable
# (the links that take turns; None: all), max_rounds, rb_below (the seeded RBs are folded into [0, rb_below))
CASES = {
    'n37_r5': (12, 25, 5, 'ld2', 40.0),
    'n50_r6_ld35_40': (20, 30, 6, 'ld35', 40.0),
    'n50_r6_ld35_120': (20, 30, 6, 'ld35', 120.0),
    'n50_r6_hata': (20, 30, 6, 'urban', 40.0),
    'n131_r33': (40, 91, 33, 'ld2', 40.0),
    'n300_r7_40': (100, 200, 7, 'ld2', 40.0),
    'n300_r7_500': (100, 200, 7, 'ld2', 500.0),
    'n20_r64': (6, 14, 64, 'ld2', 40.0),
    # ---- the paths of brdyn_kernel that need more than 64 RBs or more than 64 KiB (d2d_brdyn.hip; threads = min(256, R rounded up to 64))
    'n150_r65': (50, 100, 65, 'ld2', 40.0, dict(b=8)),                  # TWO WAVES (128 threads): the cross-wave half of the argmax
    'n300_r129': (100, 200, 129, 'ld2', 40.0, dict(b=8)),               # THREE WAVES: the 192-thread launch
    'n300_r200': (100, 200, 200, 'ld2', 40.0, dict(b=8, seed=1)),       # FOUR WAVES, the last one partly filled (lanes 200..255 idle)
    'n400_r256': (100, 300, 256, 'ld2', 40.0, dict(b=8)),               # R = 256 exactly: every lane owns one RB, none owns two
    'n400_r300': (100, 300, 300, 'ld2', 40.0, dict(b=8)),               # R > 256: lanes 0..43 own TWO RBs (r and r + 256)
    # LARGE LDS through the links: 152 KiB, the MaxDynamicSharedMemorySize branch; link indices up to 2047, bitset words up to 63.
    # A dozen movable links at the word edges and the two ends keep the public-API loop at a few dozen turns
    'n2048_r256': (512, 1536, 256, 'ld2', 40.0, dict(b=4, max_rounds=3, movable=BIG_MOVABLE)),
    # LARGE LDS through the bitset: 10 words x 2500 RBs are 98 KiB of 112 KiB.  Most RBs are empty, and empty RBs tie exactly to
    # the lowest one; the seeded RBs are folded into [0, 280) so that the movers run out of empty RBs below 256 and go on above
    'n320_r2500': (100, 220, 2500, 'ld2', 40.0, dict(b=4, max_rounds=3, rb_below=280)),
}
DEFAULTS = dict(b=B, seed=None, movable=None, max_rounds=MAX_ROUNDS, rb_below=None)


def rb_blocks(r):
    """The block of every RB for the coverage conditions, int [R].  Up to 8 blocks: r // 64, the 64 RBs that one wave's lanes own in
    one pass of the kernel's `for r = tid; r < R; r += 256`.  Past that (R in the thousands, where an env cannot have a move into
    every 64 RBs) the wave that owns the RB, (r % 256) // 64."""
    k = np.arange(r)
    return k // 64 if r <= 512 else (k % 256) // 64


def covers(dest, r):
    """dest int [R], the moves that ended on each RB: whether the destinations fall in every block of rb_blocks(), and for R > 256
    on both sides of 256 (the first and the second RB of a lane)."""
    blk = rb_blocks(r)
    every = all(dest[blk == k].sum() > 0 for k in range(blk.max() + 1))
    return bool(every and (r <= 256 or (dest[:256].sum() > 0 and dest[256:].sum() > 0)))


def link_budget(pos, tx, rx, pwr, cols, spec):
    """(sig_db [B, N], gain_mw [B, j, i] with a zero diagonal, noise_mw [N]) of the oracle's step (simulator.py:93-107)."""
    pos = np.asarray(pos, dtype=np.float64)
    pl = orc.pair_path_loss_db(spec, pos, tx, rx, cols)                  # [B, j, i]
    eirp = np.asarray(pwr, dtype=np.float64) + cols.eirp_off_db[tx][None, :]
    n = len(tx)
    k = np.arange(n)
    sig = eirp - pl[:, k, k] + cols.rx_off_db[rx][None, :]
    gain = orc.db_to_linear(eirp[:, :, None] - pl)
    gain[:, k, k] = 0.0
    return sig, gain, orc.db_to_linear(cols.noise_dbm[rx])


def dynamics(pos, tx, rx, rb, pwr, cols, spec, r, allowed=None, movable=None, min_gain_db=MIN_GAIN_DB, max_rounds=MAX_ROUNDS, m=M):
    """The dynamics in float64.  rb, pwr [B, N]; allowed bool [N, R] or None; movable bool [N] or None.  Returns a namespace: rb int
    [B, N], sinr_db float64 [B, N] (NaN on no RB), rounds / moves int [B], converged bool [B], ambiguous bool [B], on_rb, and what
    the coverage conditions of the multi-wave cases read: dest int [R], the moves that ended on each RB (all envs), and moved int
    [N], the moves each link made."""
    rb = np.asarray(rb, dtype=np.int64).copy()
    b, n = rb.shape
    on = (rb >= 0) & (rb < r)
    allowed = np.ones((n, r), bool) if allowed is None else np.asarray(allowed, dtype=bool)
    movable = np.ones(n, bool) if movable is None else np.asarray(movable, dtype=bool)
    sig, gain, noise = link_budget(pos, tx, rx, pwr, cols, spec)
    rounds, moves = np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int64)
    conv, live, ambiguous = np.zeros(b, dtype=bool), np.ones(b, dtype=bool), np.zeros(b, dtype=bool)
    dest, moved_links = np.zeros(r, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for _ in range(max_rounds):
        e = np.nonzero(live)[0]
        if not len(e):
            break
        moved = np.zeros(len(e), dtype=bool)
        for i in range(n):
            if not movable[i] or not allowed[i].any():
                continue
            ok = on[e, i]
            if not ok.any():
                continue
            ee = e[ok]
            cur = rb[ee, i]
            rows = np.arange(len(ee))
            # per RB, the mW from the links that sit on it and their number, i left out: sums over the members in ascending j
            # (O(N + R) per env and turn; a [B, N, R] membership array would be 20 MB per env at 320 x 2500)
            others = on[ee].copy()
            others[:, i] = False
            at = (rows[:, None] * r + np.where(others, rb[ee], 0))[others]
            ix = np.bincount(at, weights=gain[ee, :, i][others], minlength=len(ee) * r).reshape(len(ee), r)
            count = np.bincount(at, minlength=len(ee) * r).reshape(len(ee), r)
            s = sig[ee, i, None] - orc.linear_to_db(ix + noise[i])
            cand = np.where(allowed[i][None, :], s, -np.inf)
            best = cand.argmax(axis=1)                                   # the first maximum: ties to the lowest r
            top, own = cand[rows, best], s[rows, cur]
            g = top - own
            move = g > min_gain_db
            # ambiguity: empty RBs (nobody else there) are one candidate, the lowest of them
            w = m * np.maximum(np.abs(top), 1.0)
            empty = count == 0
            rival = cand.copy()
            rival[rows, best] = -np.inf
            rival[empty & empty[rows, best][:, None]] = -np.inf
            second = rival.max(axis=1)
            amb = ((g > min_gain_db - w) & (top - second < w)) | ((np.abs(g - min_gain_db) < w) & (g != 0.0))
            ambiguous[ee] |= amb
            mv = ee[move]
            rb[mv, i] = best[move]
            moves[mv] += 1
            np.add.at(dest, best[move], 1)
            moved_links[i] += int(move.sum())
            moved[np.nonzero(ok)[0][move]] = True
        conv[e[~moved]] = True
        live[e[~moved]] = False
        rounds[e[moved]] += 1
    rb_eff = np.where(on, rb, r + np.arange(n)[None, :])                 # a link on no RB shares its pseudo RB with nobody
    sinr = orc.step(pos, tx, rx, rb_eff, pwr, cols, spec)['sinr_db']
    sinr[~on] = np.nan
    return SimpleNamespace(rb=rb, sinr_db=sinr, rounds=rounds, moves=moves, converged=conv, ambiguous=ambiguous, on_rb=on, dest=dest,
                           moved=moved_links)


@lru_cache(maxsize=None)
def make_case(name):
    """The seeded state of a case and everything the oracle needs for it."""
    cues, dues, r, law, cell = CASES[name][:5]
    o = dict(DEFAULTS, **(CASES[name][5] if len(CASES[name]) > 5 else {}))
    seed = sum(map(ord, name)) if o['seed'] is None else o['seed']
    pos, raw, rb, pwr = pcu.state(cues, dues, r, seed, cell, 0, o['b'])
    _, _, levels = pcu.bounds(cues, dues)
    if o['rb_below']:
        rb = rb % np.int32(o['rb_below'])
        raw = (rb * levels[None, :] + pwr).astype(np.int32)
    tx, rx, _ = default_links(cues, dues)
    movable = None
    if o['movable'] is not None:
        movable = np.zeros(cues + dues, dtype=bool)
        movable[list(o['movable'])] = True
    return SimpleNamespace(name=name, cues=cues, dues=dues, n=cues + dues, r=r, law=law, cell=cell, pos=pos, raw=raw, rb=rb, pwr=pwr,
                           tx=tx, rx=rx, levels=levels, spec=pcu.models()[law][1], b=o['b'], movable=movable, max_rounds=o['max_rounds'],
                           cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


@lru_cache(maxsize=None)
def oracle_side(name):
    """The reference run of a case, computed once."""
    c = make_case(name)
    return dynamics(c.pos, c.tx, c.rx, c.rb, c.pwr, c.cols, c.spec, c.r, movable=c.movable, max_rounds=c.max_rounds)

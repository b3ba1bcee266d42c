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

# name: (cues, due pairs, R, law, cell radius m)
CASES = {
    'n37_r5': (12, 25, 5, 'ld2', 40.0),
    'n50_r6_ld35_40': (20, 30, 6, 'ld35', 40.0),
    'n50_r6_ld35_120': (20, 30, 6, 'ld35', 120.0),
    'n50_r6_hata': (20, 30, 6, 'urban', 40.0),
    'n131_r33': (40, 91, 33, 'ld2', 40.0),
    'n300_r7_40': (100, 200, 7, 'ld2', 40.0),
    'n300_r7_500': (100, 200, 7, 'ld2', 500.0),
    'n20_r64': (6, 14, 64, 'ld2', 40.0),
}


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
    [B, N], sinr_db float64 [B, N] (NaN on no RB), rounds / moves int [B], converged bool [B], ambiguous bool [B], on_rb."""
    rb = np.asarray(rb, dtype=np.int64).copy()
    b, n = rb.shape
    on = (rb >= 0) & (rb < r)
    allowed = np.ones((n, r), bool) if allowed is None else np.asarray(allowed, dtype=bool)
    movable = np.ones(n, bool) if movable is None else np.asarray(movable, dtype=bool)
    sig, gain, noise = link_budget(pos, tx, rx, pwr, cols, spec)
    member = np.zeros((b, n, r))                                         # member[b, j, r] = link j sits on RB r
    eb, ej = np.nonzero(on)
    member[eb, ej, rb[eb, ej]] = 1.0
    rounds, moves = np.zeros(b, dtype=np.int64), np.zeros(b, dtype=np.int64)
    conv, live, ambiguous = np.zeros(b, dtype=bool), np.ones(b, dtype=bool), np.zeros(b, dtype=bool)
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
            others = member[ee].copy()
            others[:, i, :] = 0.0
            ix = np.einsum('bj,bjr->br', gain[ee, :, i], others)         # [envs, R] mW from the links on each RB, i left out
            s = sig[ee, i, None] - orc.linear_to_db(ix + noise[i])
            cand = np.where(allowed[i][None, :], s, -np.inf)
            best = cand.argmax(axis=1)                                   # the first maximum: ties to the lowest r
            rows = np.arange(len(ee))
            top, own = cand[rows, best], s[rows, cur]
            g = top - own
            move = g > min_gain_db
            # ambiguity: empty RBs (nobody else there) are one candidate, the lowest of them
            w = m * np.maximum(np.abs(top), 1.0)
            empty = others.sum(axis=1) == 0.0
            rival = cand.copy()
            rival[rows, best] = -np.inf
            rival[empty & empty[rows, best][:, None]] = -np.inf
            second = rival.max(axis=1)
            amb = ((g > min_gain_db - w) & (top - second < w)) | ((np.abs(g - min_gain_db) < w) & (g != 0.0))
            ambiguous[ee] |= amb
            mv = ee[move]
            member[mv, i, cur[move]] = 0.0
            member[mv, i, best[move]] = 1.0
            rb[mv, i] = best[move]
            moves[mv] += 1
            moved[np.nonzero(ok)[0][move]] = True
        conv[e[~moved]] = True
        live[e[~moved]] = False
        rounds[e[moved]] += 1
    rb_eff = np.where(on, rb, r + np.arange(n)[None, :])                 # a link on no RB shares its pseudo RB with nobody
    sinr = orc.step(pos, tx, rx, rb_eff, pwr, cols, spec)['sinr_db']
    sinr[~on] = np.nan
    return SimpleNamespace(rb=rb, sinr_db=sinr, rounds=rounds, moves=moves, converged=conv, ambiguous=ambiguous, on_rb=on)


@lru_cache(maxsize=None)
def make_case(name):
    """The seeded state of a case and everything the oracle needs for it."""
    cues, dues, r, law, cell = CASES[name]
    pos, raw, rb, pwr = pcu.state(cues, dues, r, sum(map(ord, name)), cell, 0, B)
    tx, rx, _ = default_links(cues, dues)
    _, _, levels = pcu.bounds(cues, dues)
    return SimpleNamespace(name=name, cues=cues, dues=dues, n=cues + dues, r=r, law=law, cell=cell, pos=pos, raw=raw, rb=rb, pwr=pwr,
                           tx=tx, rx=rx, levels=levels, spec=pcu.models()[law][1],
                           cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


@lru_cache(maxsize=None)
def oracle_side(name):
    """The reference run of a case, computed once."""
    c = make_case(name)
    return dynamics(c.pos, c.tx, c.rx, c.rb, c.pwr, c.cols, c.spec, c.r)

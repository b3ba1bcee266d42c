"""What the SINR-balancing tests share: the seeded cases (the states of power_control_util under a base, a grid and optionally a floor
and an adjustable set), and the float64 reference `balance_ref`: the search of include/d2d_balance.h with power_control_util.solve
as its probe.

    probe k      solve() for the target t_k = float32(base) + float32(margins[k]), the float32 sum the kernel forms
    passes iff   it converged, no adjustable link on an RB is at p_max with sinr_db < t_k, no link on an RB has sinr_db < floor
    search       probe 0; fails: level -1.  Else lo = 0, hi = K; while hi - lo > 1: mid = (lo + hi) // 2, pass: lo = mid, fail: hi = mid

AMBIGUITY.  An env is ambiguous when float32 may legitimately decide one of its probes the other way: a probe it ran is ambiguous by
solve's own rule (an update-deciding ceiling within W of a whole number), or a compared link - an adjustable one at p_max against
its target, any link with a finite floor against that - lies within W = 2e-4 dB of what it is compared with.  A different outcome
of one probe sends the search down another branch, so the env is excluded as a whole.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import power_control_util as pcu

W, CAP, BAR = pcu.W, pcu.CAP, pcu.BAR
NEG = -np.inf


def grid(lo, hi, step):
    """lo, lo + step, ..., hi as float32 (the steps used here are exact in binary)."""
    k = int(round((hi - lo) / step)) + 1
    return (np.float32(lo) + np.arange(k, dtype=np.float32) * np.float32(step)).astype(np.float32)


# name: (case of power_control_util, base dB, margins dB, floor dB or None, 'due' (only the DUE links adjustable) or None)
_CD = lambda cue, due: {'cue': cue, 'due': due}
TABLE = {
    'n37_r5': ('n37_r5', _CD(-10.0, 0.0), grid(-30, 30, 1), None, None),
    'n37_r5_floor': ('n37_r5', 0.0, grid(-30, 45, 0.5), _CD(-5.0, NEG), 'due'),
    'n20_r64': ('n20_r64', 0.0, grid(0, 90, 3), None, None),
    'n20_r64_top': ('n20_r64', 0.0, grid(-10, 20, 2), None, None),
    'n1': ('n1', 0.0, grid(0, 100, 0.25), None, None),
    'n1_top': ('n1', 0.0, grid(0, 40, 0.25), None, None),
    'n50_r6_hata': ('n50_r6_hata', _CD(-20.0, 0.0), grid(-40, 40, 1), None, None),
    'n50_r6_ld35_floor': ('n50_r6_ld35', _CD(-15.0, 0.0), grid(-20, 43, 1), _CD(-30.0, NEG), 'due'),
    'n50_r6_no_rb': ('n50_r6_no_rb', _CD(-10.0, 0.0), grid(-30, 30, 1), None, None),
}
# past the cap on the reference alone (17 / 64 and 27 / 64 envs ambiguous): compared exactly only, never with balance_ref
EXACT_ONLY = {
    'n300_r7': ('n300_r7', _CD(-20.0, 0.0), grid(-30, 20, 2), None, None),
    'n96_r1': ('n96_r1', _CD(-20.0, 0.0), grid(-40, 10, 1), None, None),
}
# the cases whose every level is scanned one by one
SCANNED = ('n37_r5', 'n37_r5_floor', 'n20_r64', 'n20_r64_top', 'n1', 'n1_top', 'n50_r6_hata', 'n50_r6_ld35_floor')


def row(name):
    """(power_control_util case, base float32 [N], margins float32 [K], floor float32 [N] or None, adjustable bool [N] or None)."""
    case, base, margins, floor, adj = {**TABLE, **EXACT_ONLY}[name]
    c = pcu.make_case(case)
    vec = lambda v: pcu.target_vector(v, c.cues, c.dues).astype(np.float32)
    return c, vec(base), margins, None if floor is None else vec(floor), None if adj is None else np.arange(c.n) >= c.cues


def probe(c, envs, base, margin, floor, adjustable, max_iters=64):
    """One probe of the envs `envs`: (passes bool [E], ambiguous bool [E], the solve)."""
    t = (base + np.float32(margin)).astype(np.float64)                  # the float32 sum, then exact
    fl = np.full(c.n, NEG) if floor is None else floor.astype(np.float64)
    s = pcu.solve(c.pos[envs], c.tx, c.rx, c.rb[envs], c.pwr[envs], c.cols, c.spec, c.r, t, c.p_min, c.p_max, adjustable, max_iters)
    capped = s.adjustable & (s.power_dbm == np.asarray(c.p_max)[None, :])
    with np.errstate(invalid='ignore'):
        short = capped & (s.sinr_db < t[None, :])
        low = s.on_rb & (s.sinr_db < fl[None, :])
        near = (capped & (np.abs(s.sinr_db - t[None, :]) < W)) | (s.on_rb & np.isfinite(fl)[None, :] & (np.abs(s.sinr_db - fl[None, :]) < W))
    return s.converged & ~short.any(axis=1) & ~low.any(axis=1), s.ambiguous | near.any(axis=1), s


def balance_ref(c, base, margins, floor=None, adjustable=None, max_iters=64):
    """The search in float64.  Returns a namespace: level, probes int [B], margin_db float [B], power_dbm int [B, N], sinr_db
    float64 [B, N] (those of probe `level`, of probe 0 where infeasible), ambiguous bool [B], on_rb bool [B, N]."""
    b, k_all = c.b, len(margins)
    lo, hi = np.full(b, -1), np.full(b, k_all)
    amb, probes = np.zeros(b, dtype=bool), np.zeros(b, dtype=np.int64)
    power, sinr, on_rb = np.zeros((b, c.n), dtype=np.int64), np.zeros((b, c.n)), np.zeros((b, c.n), dtype=bool)
    mid, live, first = np.zeros(b, dtype=np.int64), np.ones(b, dtype=bool), True
    while live.any():
        for k in np.unique(mid[live]):
            e = np.nonzero(live & (mid == k))[0]
            ok, a, s = probe(c, e, base, margins[k], floor, adjustable, max_iters)
            amb[e] |= a
            probes[e] += 1
            keep = e if first else e[ok]                                # probe 0 is kept whatever it says
            power[keep], sinr[keep], on_rb[keep] = s.power_dbm[ok | first], s.sinr_db[ok | first], s.on_rb[ok | first]
            lo[e[ok]] = k
            hi[e[~ok]] = k
        first = False
        live = (hi - lo > 1) & (lo >= 0)
        mid = (lo + hi) // 2
    margin = np.where(lo >= 0, margins.astype(np.float64)[np.maximum(lo, 0)], NEG)
    return SimpleNamespace(level=lo, probes=probes, margin_db=margin, power_dbm=power, sinr_db=sinr, ambiguous=amb, on_rb=on_rb)


def scan_ref(c, base, margins, floor=None, adjustable=None, max_iters=64):
    """Every level probed one by one: (passes bool [K, B], ambiguous bool [K, B])."""
    every = np.arange(c.b)
    out = [probe(c, every, base, m, floor, adjustable, max_iters)[:2] for m in margins]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@lru_cache(maxsize=None)
def reference(name):
    """balance_ref of a row of TABLE or EXACT_ONLY, computed once."""
    c, base, margins, floor, adj = row(name)
    return balance_ref(c, base, margins, floor, adj)

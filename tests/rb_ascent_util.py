"""What the RB-ascent tests share (test_rb_ascent_cpu.py, test_gpu_rb_ascent.py): the cases (seeded states of power_control_util
plus small ones of their own, under a movable set, an allowed mask and floors), the sequential float64 restatement `rb_ascent_ref`
on the oracle's step (oracle/d2d_oracle.py), the exact host loop `rb_ascent_by_evaluate` over env.evaluate(), and the fixed-point
check `reference_check`.

The statement (include/d2d_rbascent.h).  A link is on an RB iff 0 <= rb < R; the group of RB r is the set of links on r in ascending
link index.  A turn of the movable link i on RB c: with rb^r = rb with rb[i] = r and sinr^r, cap^r the planes of (rb^r, pwr),
With(r) is the sequential double sum of cap^r over group(r) u {i}, Without(r) the one over group(r) \\ {i} with i elsewhere (of
cap^c for r != c, of cap^r' for any r' != c for r == c), D(r) = With(r) - Without(r).  r is a candidate iff r != c, allowed[i][r]
and every m of group(r) u {i} with a floor above -inf has sinr^r_m >= floor or sinr^c_m < floor.  best is the lowest candidate
whose D is maximal among the candidates (a NaN D is never chosen); the link moves iff D(best) - D(c) > min_gain.  The movable links
take turns in ascending link index; a round that moves nobody ends the ascent, and so do max_rounds rounds that each moved a link.

`decide` is that turn on planes [R, N] of any precision: the restatement feeds it the oracle's float64 planes, the exact loop
evaluate()'s float32 ones.  The float64 restatement is no trajectory yardstick (D is nearly flat between similar RBs and float32
capacities may rank two of them the other way): it checks properties of the outcome; the path is checked word for word against
`rb_ascent_by_evaluate`.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import ascent_util as au
import power_control_util as pcu
from oracle import d2d_oracle as orc
from sim_util import default_links

W, CAP, BAR = pcu.W, pcu.CAP, pcu.BAR
NEG = -np.inf
FLOORS = {'cue': 0.0, 'due': 5.0}
sequential_sum = au.sequential_sum
floor_vector = au.floor_vector

# the small states of this module: name -> (cues, due pairs, R, law, cell radius m, envs)
OWN = {
    'n20_r300': (6, 14, 300, 'ld2', 500.0, 8),       # more RBs than threads; the last allowed word partly filled (300 = 9 * 32 + 12)
    'n96_r2': (32, 64, 2, 'ld2', 500.0, 2),          # two groups near 48
}
# name: (state, envs, every: movable = the agent links j with j % every == 0)
CASES = {
    'n37_r5': ('n37_r5', 16, 1),
    'n20_r64': ('n20_r64', 16, 1),                   # more RBs than links
    'n20_r300': ('n20_r300', 8, 1),
    'n96_r2': ('n96_r2', 2, 1),
    'n96_r1': ('n96_r1', 2, 1),                      # no candidate: zero moves, converged
    'n50_r6_hata': ('n50_r6_hata', 8, 1),            # the pow-k law
    'n50_r6_ld35': ('n50_r6_ld35', 8, 1),
    'n50_r6_no_rb': ('n50_r6_no_rb', 8, 1),          # a link on no RB
    'n300_r7': ('n300_r7', 4, 5),                    # more links than threads; ten bitset words
    'n1000_r64_ld35': ('n1000_r64_ld35', 2, 16),     # past 64 KiB of LDS
}
MIXED = ('n50_r6_mixed', 8, 1)                       # the general power law: no oracle model, exact checks only


@lru_cache(maxsize=None)
def make_case(name):
    """The seeded state of a case: power_control_util's, or one of OWN in the same form."""
    if name not in OWN:
        return pcu.make_case(name)
    cues, dues, r, law, cell, b = OWN[name]
    pos, raw, rb, pwr = pcu.state(cues, dues, r, sum(map(ord, name)), cell, 0, b)
    tx, rx, _ = default_links(cues, dues)
    p_min, p_max, levels = pcu.bounds(cues, dues)
    return SimpleNamespace(name=name, cues=cues, dues=dues, n=cues + dues, r=r, law=law, cell=cell, pos=pos, raw=raw, rb=rb, pwr=pwr, b=b,
                           tx=tx, rx=rx, p_min=p_min, p_max=p_max, levels=levels, spec=pcu.models()[law][1],
                           cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


def movable_mask(n, every):
    return np.arange(n) % every == 0


def allowed_mask(n, r, seed, rb=None):
    """A random bool [N, R]: a fifth of the rows all zero (the link never moves), and, with rb [N], every third link's own RB
    excluded (it may only leave)."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, r)) < 0.6
    mask[rng.random(n) < 0.2] = False
    if rb is not None:
        for i in range(0, n, 3):
            if 0 <= rb[i] < r:
                mask[i, rb[i]] = False
    return mask


# ------------------------------------------------------------------------------------------ one turn, on planes of any precision
def sets(rb, i, r_count):
    """(group(r) \\ {i}, group(r) u {i}) as bool [R, N] for the assignment rb [N]."""
    n = len(rb)
    m = (rb[None, :] == np.arange(r_count)[:, None])
    m[:, i] = False
    w = m.copy()
    w[:, i] = True
    return m, w


def presence(cap, rb, i, r_count):
    """(With, Without, D) double [R] from the capacity planes cap [R, N] (row r: rb with rb[i] = r)."""
    c = int(rb[i])
    m, w = sets(rb, i, r_count)
    cap = np.asarray(cap, dtype=np.float64)
    with_ = sequential_sum(np.where(w, cap, 0.0), axis=1)                # a link outside the set adds 0.0: the sum of the members
    without = sequential_sum(np.where(m, cap[c][None, :], 0.0), axis=1)  # cap^c: i where it is
    if r_count > 1:
        other = 0 if c != 0 else 1                                       # any r' != c
        without[c] = sequential_sum(np.where(m[c], cap[other], 0.0))
    with np.errstate(invalid='ignore'):
        return with_, without, with_ - without


def decide(sinr, cap, rb, i, allowed_i, floor, min_gain):
    """The turn of link i (on an RB) on the planes sinr, cap [R, N].  floor [N] in the planes' precision.  Returns (the RB to move
    to or None, D [R], candidate bool [R], admissible bool [R])."""
    r_count = sinr.shape[0]
    c = int(rb[i])
    _, _, d = presence(cap, rb, i, r_count)
    _, w = sets(rb, i, r_count)
    f = floor[None, :]
    with np.errstate(invalid='ignore'):
        ok = ~(f > NEG) | (sinr >= f) | (sinr[c][None, :] < f)
    adm = (ok | ~w).all(axis=1)
    cand = adm & np.asarray(allowed_i, dtype=bool) & (np.arange(r_count) != c) & ~np.isnan(d)
    if not cand.any():
        return None, d, cand, adm
    top = d[cand].max()
    best = int(np.nonzero(cand & (d == top))[0][0])
    with np.errstate(invalid='ignore'):
        return (best if d[best] - d[c] > min_gain else None), d, cand, adm


def candidates(rb, i, r_count):
    """int [R, N]: row r is rb with rb[i] = r."""
    cand = np.repeat(np.asarray(rb)[None, :], r_count, axis=0)
    cand[:, i] = np.arange(r_count)
    return cand


# ------------------------------------------------------------------------------------------ the float64 restatement
def oracle_planes(c, e, rb_rows, pwr):
    """The oracle's float64 (sinr_db, capacity_mbps) [K, N] of env e for the assignments rb_rows [K, N]; a link on no RB shares its
    pseudo RB with nobody."""
    rb_rows = np.asarray(rb_rows, dtype=np.int64)
    k, n = rb_rows.shape
    on = (rb_rows >= 0) & (rb_rows < c.r)
    rb_eff = np.where(on, rb_rows, c.r + np.arange(n)[None, :])
    pos = np.broadcast_to(c.pos[e].astype(np.float64), (k,) + c.pos[e].shape)
    out = orc.step(pos, c.tx, c.rx, rb_eff, np.repeat(np.asarray(pwr, dtype=np.float64)[None, :], k, axis=0), c.cols, au._table_spec(c, e),
                   chunk=k)
    return out['sinr_db'], out['capacity_mbps']


def _turns(c, rb_row, allowed, movable):
    on = (rb_row >= 0) & (rb_row < c.r)
    mov = np.ones(c.n, bool) if movable is None else np.asarray(movable, dtype=bool)
    some = np.ones(c.n, bool) if allowed is None else np.asarray(allowed, dtype=bool).any(axis=1)
    return [i for i in range(c.n) if on[i] and mov[i] and some[i]]


def rb_ascent_ref(c, envs, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """The sequential statement in float64 on the oracle's step, env by env.  Returns a namespace: rb int [E, N], rounds, moves int
    [E], converged bool [E], raised: list of (env, link, the env's oracle total before, after) per move, floor_changed bool [E]
    (some turn's choice differs from what it would have been without floors), start int [E, N]."""
    envs = np.asarray(envs)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    none = np.full(c.n, NEG)
    rb0 = np.asarray(c.rb)[envs].astype(np.int64)
    rb_all = rb0.copy()
    rounds, moves = np.zeros(len(envs), dtype=np.int64), np.zeros(len(envs), dtype=np.int64)
    conv, changed, raised = np.zeros(len(envs), dtype=bool), np.zeros(len(envs), dtype=bool), []
    every = np.ones(c.r, bool)
    for x, e in enumerate(envs):
        rb = rb_all[x]
        turns = _turns(c, rb, allowed, movable)                          # on an RB, marked, some allowed RB: moves keep all three
        for _ in range(max_rounds):
            moved = False
            for i in turns:
                sinr, cap = oracle_planes(c, e, candidates(rb, i, c.r), c.pwr[e])
                al = every if allowed is None else allowed[i]
                to, _, _, _ = decide(sinr, cap, rb, i, al, fl, min_gain)
                free, _, _, _ = decide(sinr, cap, rb, i, al, none, min_gain)
                changed[x] |= to != free
                if to is not None:
                    raised.append((int(e), i, float(sequential_sum(cap[rb[i]])), float(sequential_sum(cap[to]))))
                    rb[i] = to
                    moved = True
                    moves[x] += 1
            if not moved:
                conv[x] = True
                break
            rounds[x] += 1
    return SimpleNamespace(rb=rb_all, rounds=rounds, moves=moves, converged=conv, raised=raised, floor_changed=changed, start=rb0)


@lru_cache(maxsize=None)
def reference(name, floors=False, max_rounds=16):
    """rb_ascent_ref of a row of CASES on its envs, computed once."""
    case, b, every = CASES[name]
    c = make_case(case)
    return rb_ascent_ref(c, np.arange(b), None, movable_mask(c.n, every), FLOORS if floors else None, 0.0, max_rounds)


def reference_check(c, envs, rb_final, converged, allowed=None, movable=None, floor=None, min_gain=0.0):
    """The fixed-point inequality of the float64 oracle at the RBs `rb_final` [E, N] (of the envs `envs`), for the envs `converged`
    marks.  For every movable link i on RB c and every candidate r that the float64 floor test admits:

        D64(r) - D64(c) <= min_gain + BAR * sum(T64 + group size)

    over the four group sums involved (With(r), Without(r), With(c), Without(c)): what a per-capacity deviation of
    BAR max(|ref|, 1) allows on them.  A check is left out iff some member's float64 SINR lies within W of its floor or of its
    receiver sensitivity in either state (with i, without i; on r or on c).  Returns a namespace: checks, left_out (counts), worst
    (the largest left side less min_gain, over the bound's slack term: <= 1 passes), violations (list)."""
    envs = np.asarray(envs)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    sens = c.cols.sens_dbm[np.asarray(c.rx)]
    checks = left_out = 0
    worst, violations = -np.inf, []
    every = np.ones(c.r, bool)
    for x, e in enumerate(envs):
        if not converged[x]:
            continue
        rb = np.asarray(rb_final[x], dtype=np.int64)
        for i in _turns(c, rb, allowed, movable):
            cur = int(rb[i])
            sinr, cap = oracle_planes(c, e, candidates(rb, i, c.r), c.pwr[e])
            al = every if allowed is None else allowed[i]
            _, d, cand, _ = decide(sinr, cap, rb, i, al, fl, min_gain)
            with_, without, _ = presence(cap, rb, i, c.r)
            m, w = sets(rb, i, c.r)
            close = (np.abs(sinr - sens[None, :]) < W) | ((fl > NEG)[None, :] & (np.abs(sinr - fl[None, :]) < W))
            before = np.repeat(sinr[cur][None, :], c.r, axis=0)          # the members of r without i: the row of rb^c ...
            if c.r > 1:
                before[cur] = sinr[0 if cur != 0 else 1]                 # ... and those of c without i: any other row
            close_b = (np.abs(before - sens[None, :]) < W) | ((fl > NEG)[None, :] & (np.abs(before - fl[None, :]) < W))
            near = (close & w).any(axis=1) | (close_b & m).any(axis=1)
            size = w.sum(axis=1) + m.sum(axis=1)
            for r in np.nonzero(cand)[0]:
                checks += 1
                if near[r] or near[cur]:
                    left_out += 1
                    continue
                slack = BAR * (with_[r] + without[r] + with_[cur] + without[cur] + size[r] + size[cur])
                over = (d[r] - d[cur] - min_gain) / slack
                worst = max(worst, over)
                if over > 1.0:
                    violations.append((int(e), int(i), int(r), float(d[r]), float(d[cur])))
    return SimpleNamespace(checks=checks, left_out=left_out, worst=worst, violations=violations)


# ------------------------------------------------------------------------------------------ the exact host loop over evaluate()
def rb_ascent_by_evaluate(env, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """The statement as a host loop: one env.evaluate() call per link turn with K = R candidates (candidate r has rb[i] = r; every env
    takes link i's turn in the same call), the sums sequential double sums of the float32 capacity plane over the member sets the
    statement names, the floor comparisons in float32 on the sinr_db plane.  Without(c) comes from a candidate r' != c, Without(r)
    from candidate c.  Returns host arrays (rb int32, sinr_db, capacity_mbps float32 [B, N], rounds, moves int32 [B], converged
    uint8 [B]) and the number of evaluate() calls."""
    import torch
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    rb = env._t['rb'].cpu().numpy().astype(np.int64)
    pwr = env._t['pwr'].contiguous()
    mov = np.arange(n) >= n - env.num_agents
    if movable is not None:
        mov = mov & np.asarray(movable.cpu() if torch.is_tensor(movable) else movable, dtype=bool)
    al = None if allowed is None else np.asarray(allowed.cpu() if torch.is_tensor(allowed) else allowed, dtype=bool)
    if al is not None:
        mov = mov & al.any(axis=1)
    every = np.ones(r, bool)
    fl = floor_vector(floor, env.num_cues, n - env.num_cues)
    on = (rb >= 0) & (rb < r)                                            # a move keeps a link on an RB, and off one it never turns
    pwr_k = pwr[:, None, :].expand(b, r, n).contiguous()
    rounds, moves = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
    conv, live, calls = np.zeros(b, dtype=np.uint8), np.ones(b, dtype=bool), 0
    for _ in range(max_rounds):
        moved = np.zeros(b, dtype=bool)
        for i in np.nonzero(mov)[0]:
            turn = live & on[:, i]
            if not turn.any():
                continue
            cand = np.stack([candidates(rb[e], i, r) for e in range(b)])
            res = env.evaluate(torch.as_tensor(cand.astype(np.int32), device=env.device), pwr_k)
            calls += 1
            sinr, cap = res['sinr_db'].cpu().numpy(), res['capacity_mbps'].cpu().numpy()
            assert sinr.dtype == cap.dtype == np.float32
            for e in np.nonzero(turn)[0]:
                to, _, _, _ = decide(sinr[e], cap[e], rb[e], i, every if al is None else al[i], fl, min_gain)
                if to is not None:
                    rb[e, i] = to
                    moved[e] = True
                    moves[e] += 1
        conv[live & ~moved] = 1
        rounds[live & moved] += 1
        live &= moved
        if not live.any():
            break
    res = env.evaluate(torch.as_tensor(rb[:, None, :].astype(np.int32), device=env.device), pwr[:, None, :].contiguous())
    sinr, cap = res['sinr_db'].cpu().numpy()[:, 0].copy(), res['capacity_mbps'].cpu().numpy()[:, 0].copy()
    return (rb.astype(np.int32), sinr, cap, rounds, moves, conv), calls + 1

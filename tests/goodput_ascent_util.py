"""What the goodput-ascent tests share (test_goodput_ascent_cpu.py, test_gpu_goodput_ascent.py): the cases (rb_ascent_util's seeded
states under demand and weight patterns of their own), the turn `decide` on planes of any precision, the exact host loop
`goodput_by_evaluate` over env.evaluate(), the sequential float64 restatement `goodput_ref` on the oracle's step
(oracle/d2d_oracle.py) and the fixed-point check `reference_check`.

The statement (include/d2d_goodput.h).  For a state s = (rb, pwr): cap_m(s), sinr_m(s) are evaluate()'s float32 values; budget(c) is
rule 5 of include/d2d_queue.h (queue_util.budget_bits): floor(double(c) * bits_per_mbps) clipped to [0, 2^31 - 1], NaN, negative
and zero giving 0; served_m(s) = min(budget(cap_m(s)), max(demand_m, 0)); term_m(s) = int64(weight_m) * served_m(s); V(s) is the
sum of term_m(s) over ALL links.  A link takes turns iff it is on an RB, movable and, with RB moves only, has an allowed RB.  A turn
of link i on RB c at power p: the candidates are (r, p) for every allowed r != c (RB moves) and (c, q) for every level q != p of
the link's class (power moves); Delta = V(candidate) - V(s); a candidate is admissible iff every member m of group(c), group(r)
and link i with a floor above -inf has sinr_m(candidate) >= floor or sinr_m(s) < floor (float32, NaN compares false); best is the
admissible candidate of maximal Delta, ties to the lowest power, then to the lowest RB; the link moves iff Delta(best) > min_gain.
Links take turns in ascending index; a round that moves nobody ends the ascent, and so do max_rounds rounds that each moved a link.

`decide` is that turn on planes [K + 1, N] of any precision - row 0 the current state, rows 1 .. K the slots of `slots`, a fixed
superset of the candidates with the ones that are none marked invalid: the exact loop feeds it evaluate()'s float32 planes and
queue_util.budget_bits, the restatement the oracle's float64 planes and `budget64`.  The float64 restatement is no trajectory
yardstick (a budget is a floor() of a capacity: one ulp of float32 moves a bit); it checks properties of the outcome.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import ascent_util as au
import power_control_util as pcu
import rb_ascent_util as ru
from oracle import d2d_oracle as orc
from queue_util import budget_bits

W, CAP, BAR = pcu.W, pcu.CAP, pcu.BAR
NEG = -np.inf
FLOORS = ru.FLOORS
UNCAPPED = (1 << 31) - 1
MAX_WEIGHT = 1 << 20
BPM = 1000.0                                         # PacketTraffic's default step: 1 Mbps carries 1000 bits
SATURATING = 1.0e9                                   # every capacity above 2.15 Mbps hits the budget's clip; the others do not
MOVE_RB, MOVE_POWER = 1, 2
MOVES = {'rb': MOVE_RB, 'power': MOVE_POWER}
CASES = dict(ru.CASES)                               # name: (state, envs, every: movable = the agent links j with j % every == 0)
CASES['n1000_r64_ld35'] = ('n1000_r64_ld35', 2, 32)
CASES['n300_r7'] = ('n300_r7', 4, 10)
MIXED = ru.MIXED
make_case = ru.make_case
movable_mask = ru.movable_mask
allowed_mask = ru.allowed_mask
floor_vector = au.floor_vector


def mask_of(move):
    m = 0
    for name in ((move,) if isinstance(move, str) else move):
        m |= MOVES[name]
    return m


def pattern(kind, b, n, seed=0):
    """(demand_bits int32 [B, N] or the scalar 2^31 - 1, weight int32 [B, N] or None, bits_per_mbps) of a named pattern.

    zero       all demand zero: no Delta is positive
    uncapped   demand uncapped (2^31 - 1), weight 1 (None): the sum of the budgets
    mix        demand 0 on a third of the links, small (capped: ties go to the lowest power) on a third, uncapped on the rest;
               weights 0, 1 and 2^20
    saturate   the mix's weights, demand uncapped, a bits_per_mbps at which budgets saturate at 2^31 - 1"""
    rng = np.random.default_rng(1000 + seed)
    if kind == 'zero':
        return np.zeros((b, n), dtype=np.int32), None, BPM
    if kind == 'uncapped':
        return UNCAPPED, None, BPM
    third = rng.integers(0, 3, (b, n))
    weight = np.array([0, 1, MAX_WEIGHT], dtype=np.int32)[rng.integers(0, 3, (b, n))]
    if kind == 'saturate':
        return UNCAPPED, weight, SATURATING
    assert kind == 'mix', kind
    demand = np.where(third == 0, 0, np.where(third == 1, rng.integers(1, 400, (b, n)), UNCAPPED)).astype(np.int32)
    demand[:, ::7] = -5                              # a negative demand counts as 0
    return demand, weight, BPM


def budget64(capacity_mbps, bits_per_mbps):
    """The budget rule on float64 capacities, not rounded to float32 first: the restatement's."""
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.asarray(capacity_mbps, dtype=np.float64) * np.float64(bits_per_mbps)
        return np.floor(np.where(x > 0.0, np.minimum(x, 2147483647.0), 0.0)).astype(np.int64)


def planes_of(demand, weight, b, n):
    """int64 [B, N] demand (negative: 0; None: uncapped) and weight (None: 1)."""
    d = np.full((b, n), UNCAPPED, dtype=np.int64) if demand is None else np.maximum(np.broadcast_to(np.asarray(demand), (b, n)).astype(np.int64), 0)
    w = np.ones((b, n), dtype=np.int64) if weight is None else np.broadcast_to(np.asarray(weight), (b, n)).astype(np.int64)
    assert (w >= 0).all() and (w <= MAX_WEIGHT).all()
    return d, w


# ------------------------------------------------------------------------------------------ one turn, on planes of any precision
def slots(rb, pwr, i, r_count, lo, hi, mv):
    """The slots of link i's turn for the states rb, pwr int [E, N]: (rb_rows, pwr_rows int [E, K + 1, N], slot_r int [E, K + 1],
    slot_q int [E, K + 1], valid bool [E, K + 1]).  Row 0 is the current state; then, with RB moves, one slot per RB r (invalid where
    r is the link's own), then, with power moves, one slot per level q of [lo, hi] (invalid where q is the held power)."""
    e, n = rb.shape
    n_rb = r_count if mv & MOVE_RB else 0
    n_pw = hi - lo + 1 if mv & MOVE_POWER and lo <= pwr[:, i].min() and pwr[:, i].max() <= hi else 0
    k = 1 + n_rb + n_pw
    rb_rows, pwr_rows = np.repeat(rb[:, None, :], k, axis=1), np.repeat(pwr[:, None, :], k, axis=1)
    slot_r, slot_q = np.repeat(rb[:, i][:, None], k, axis=1), np.repeat(pwr[:, i][:, None], k, axis=1)
    slot_r[:, 1:1 + n_rb] = np.arange(n_rb)[None, :]
    slot_q[:, 1 + n_rb:] = lo + np.arange(n_pw)[None, :]
    rb_rows[:, :, i], pwr_rows[:, :, i] = slot_r, slot_q
    valid = (slot_r != rb[:, i][:, None]) | (slot_q != pwr[:, i][:, None])
    return rb_rows, pwr_rows, slot_r, slot_q, valid


def decide(sinr, cap, rb, i, slot_r, slot_q, valid, floor, demand, weight, bits_per_mbps, min_gain, budget=budget_bits):
    """The turn of link i (on an RB) of ONE env on the planes sinr, cap [K + 1, N] of `slots`.  rb int [N] (the current state), floor
    [N] in the planes' precision, demand / weight int64 [N].  Returns (the slot moved to or None, Delta int64 [K + 1], candidate bool
    [K + 1], affected bool [K + 1, N])."""
    term = weight[None, :] * np.minimum(budget(cap, bits_per_mbps), demand[None, :])
    delta = term.sum(axis=1) - term[0].sum()
    aff = (rb[None, :] == rb[i]) | (rb[None, :] == slot_r[:, None])
    aff[:, i] = True
    f = floor[None, :]
    with np.errstate(invalid='ignore'):
        ok = ~(f > NEG) | (sinr >= f) | (sinr[0][None, :] < f)
    cand = valid & (ok | ~aff).all(axis=1)
    if not cand.any():
        return None, delta, cand, aff
    top = delta[cand].max()
    tied = np.nonzero(cand & (delta == top))[0]
    best = int(tied[np.lexsort((slot_r[tied], slot_q[tied]))[0]])        # the lowest power, then the lowest RB
    return (best if top > min_gain else None), delta, cand, aff


def turn_links(rb, r_count, agent, movable, allowed, mv):
    """bool [E, N]: the links that take turns in the states rb [E, N]."""
    on = (rb >= 0) & (rb < r_count)
    mov = np.asarray(agent, dtype=bool).copy()
    if movable is not None:
        mov &= np.asarray(movable, dtype=bool)
    if allowed is not None and not mv & MOVE_POWER:
        mov &= np.asarray(allowed, dtype=bool).any(axis=1)
    return on & mov[None, :]


def _slot_valid(valid, slot_r, rb_col, allowed_i, r_count, mv):
    """An RB slot counts only where the link may move there."""
    if allowed_i is None or not mv & MOVE_RB:
        return valid
    ok = valid.copy()
    ok[:, 1:1 + r_count] &= np.asarray(allowed_i, dtype=bool)[None, :]
    return ok


# ------------------------------------------------------------------------------------------ the exact host loop over evaluate()
def goodput_by_evaluate(env, demand=None, weight=None, bits_per_mbps=BPM, move=('rb', 'power'), allowed=None, movable=None, floor=None,
                        min_gain=0, max_rounds=16):
    """The statement as a host loop: one env.evaluate() call per link turn whose candidate 0 is the current state and whose candidates
    1 .. K are the turn's slots (every env takes link i's turn in the same call), the terms formed in NumPy int64 from the float32
    capacity plane by queue_util.budget_bits, the floor comparisons in float32 on the sinr_db plane.  Returns host arrays (rb,
    power_dbm int32, sinr_db, capacity_mbps float32, served_bits int32 [B, N], value int64, rounds, moves int32, converged uint8 [B])
    and the number of evaluate() calls."""
    import torch
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    mv = mask_of(move)
    host = lambda x: None if x is None else np.asarray(x.cpu() if torch.is_tensor(x) else x)
    rb = env._t['rb'].cpu().numpy().astype(np.int64)
    pwr = env._t['pwr'].cpu().numpy().astype(np.int64)
    p_min, p_max = (np.asarray(a, dtype=np.int64) for a in env._class_bounds())
    dem, wgt = planes_of(host(demand), host(weight), b, n)
    al = None if allowed is None else host(allowed).astype(bool)
    takes = turn_links(rb, r, np.arange(n) >= n - env.num_agents, host(movable), al, mv)
    fl = floor_vector(floor, env.num_cues, n - env.num_cues)
    rounds, moves = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
    conv, live, calls = np.zeros(b, dtype=np.uint8), np.ones(b, dtype=bool), 0
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a.astype(np.int32)), device=env.device)
    for _ in range(max_rounds):
        moved = np.zeros(b, dtype=bool)
        for i in np.nonzero(takes.any(axis=0))[0]:
            turn = live & takes[:, i]
            if not turn.any():
                continue
            rb_rows, pwr_rows, slot_r, slot_q, valid = slots(rb, pwr, i, r, p_min[i], p_max[i], mv)
            if valid.shape[1] == 1:
                continue
            valid = _slot_valid(valid, slot_r, rb[:, i], None if al is None else al[i], r, mv)
            res = env.evaluate(dev(rb_rows), dev(pwr_rows))
            calls += 1
            sinr, cap = res['sinr_db'].cpu().numpy(), res['capacity_mbps'].cpu().numpy()
            assert sinr.dtype == cap.dtype == np.float32
            for e in np.nonzero(turn)[0]:
                to, _, _, _ = decide(sinr[e], cap[e], rb[e], i, slot_r[e], slot_q[e], valid[e], fl, dem[e], wgt[e], bits_per_mbps, min_gain)
                if to is not None:
                    rb[e, i], pwr[e, i] = slot_r[e, to], slot_q[e, to]
                    moved[e] = True
                    moves[e] += 1
        conv[live & ~moved] = 1
        rounds[live & moved] += 1
        live &= moved
        if not live.any():
            break
    res = env.evaluate(dev(rb[:, None, :]), dev(pwr[:, None, :]))
    sinr, cap = res['sinr_db'].cpu().numpy()[:, 0].copy(), res['capacity_mbps'].cpu().numpy()[:, 0].copy()
    served = np.minimum(budget_bits(cap, bits_per_mbps), dem)
    value = (wgt * served).sum(axis=1).astype(np.int64)
    return (rb.astype(np.int32), pwr.astype(np.int32), sinr, cap, served.astype(np.int32), value, rounds, moves, conv), calls + 1


# ------------------------------------------------------------------------------------------ the float64 restatement
def oracle_planes(c, e, rb_rows, pwr_rows):
    """The oracle's float64 (sinr_db, capacity_mbps) [K, N] of env e for the states (rb_rows, pwr_rows) [K, N]; a link on no RB shares
    its pseudo RB with nobody."""
    rb_rows = np.asarray(rb_rows, dtype=np.int64)
    k, n = rb_rows.shape
    on = (rb_rows >= 0) & (rb_rows < c.r)
    rb_eff = np.where(on, rb_rows, c.r + np.arange(n)[None, :])
    pos = np.broadcast_to(c.pos[e].astype(np.float64), (k,) + c.pos[e].shape)
    out = orc.step(pos, c.tx, c.rx, rb_eff, np.asarray(pwr_rows, dtype=np.float64), c.cols, au._table_spec(c, e), chunk=k)
    return out['sinr_db'], out['capacity_mbps']


def value64(c, e, rb, pwr, dem, wgt, bits_per_mbps):
    cap = oracle_planes(c, e, np.asarray(rb)[None, :], np.asarray(pwr)[None, :])[1][0]
    return int((wgt * np.minimum(budget64(cap, bits_per_mbps), dem)).sum())


def goodput_ref(c, envs, demand=None, weight=None, bits_per_mbps=BPM, move=('rb', 'power'), allowed=None, movable=None, floor=None,
                min_gain=0, max_rounds=16, rb0=None, pwr0=None):
    """The sequential statement in float64 on the oracle's step, env by env (demand / weight [E, N] of `envs`, or None).  Returns a
    namespace: rb, power_dbm int [E, N], value int [E] (V64 of the final state), rounds, moves int [E], converged bool [E], raised:
    list of (env, link, V64 before, V64 after) per move, start_rb / start_pwr."""
    envs = np.asarray(envs)
    mv = mask_of(move)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    rb = (np.asarray(c.rb)[envs] if rb0 is None else np.asarray(rb0)).astype(np.int64).copy()
    pwr = (np.asarray(c.pwr)[envs] if pwr0 is None else np.asarray(pwr0)).astype(np.int64).copy()
    start_rb, start_pwr = rb.copy(), pwr.copy()
    dem, wgt = planes_of(demand, weight, len(envs), c.n)
    takes = turn_links(rb, c.r, np.ones(c.n, bool), movable, allowed, mv)
    rounds, moves = np.zeros(len(envs), dtype=np.int64), np.zeros(len(envs), dtype=np.int64)
    conv, raised, value = np.zeros(len(envs), dtype=bool), [], np.zeros(len(envs), dtype=np.int64)
    for x, e in enumerate(envs):
        for _ in range(max_rounds):
            moved = False
            for i in np.nonzero(takes[x])[0]:
                rb_rows, pwr_rows, slot_r, slot_q, valid = slots(rb[x:x + 1], pwr[x:x + 1], i, c.r, c.p_min[i], c.p_max[i], mv)
                valid = _slot_valid(valid, slot_r, rb[x:x + 1, i], None if allowed is None else allowed[i], c.r, mv)
                sinr, cap = oracle_planes(c, e, rb_rows[0], pwr_rows[0])
                to, delta, _, _ = decide(sinr, cap, rb[x], i, slot_r[0], slot_q[0], valid[0], fl, dem[x], wgt[x], bits_per_mbps, min_gain, budget64)
                if to is not None:
                    before = int((wgt[x] * np.minimum(budget64(cap[0], bits_per_mbps), dem[x])).sum())
                    raised.append((int(e), int(i), before, before + int(delta[to])))
                    rb[x, i], pwr[x, i] = slot_r[0, to], slot_q[0, to]
                    moved = True
                    moves[x] += 1
            if not moved:
                conv[x] = True
                break
            rounds[x] += 1
        value[x] = value64(c, e, rb[x], pwr[x], dem[x], wgt[x], bits_per_mbps)
    return SimpleNamespace(rb=rb, power_dbm=pwr, value=value, rounds=rounds, moves=moves, converged=conv, raised=raised, start_rb=start_rb,
                           start_pwr=start_pwr)


def case_inputs(name, kind='mix'):
    """(c, b, movable bool [N], demand, weight, bits_per_mbps) of a row of CASES under a pattern."""
    case, b, every = CASES[name]
    c = make_case(case)
    demand, weight, bpm = pattern(kind, b, c.n, sum(map(ord, name)))
    return c, b, movable_mask(c.n, every), demand, weight, bpm


@lru_cache(maxsize=None)
def reference(name, floors=False, kind='mix', move=('rb', 'power'), max_rounds=16):
    """goodput_ref of a row of CASES on its envs under a pattern, computed once."""
    c, b, mov, demand, weight, bpm = case_inputs(name, kind)
    return goodput_ref(c, np.arange(b), demand, weight, bpm, move, None, mov, FLOORS if floors else None, 0, max_rounds)


def reference_check(c, envs, rb_final, pwr_final, converged, demand=None, weight=None, bits_per_mbps=BPM, move=('rb', 'power'), allowed=None,
                    movable=None, floor=None, min_gain=0):
    """The fixed-point inequality of the float64 oracle at the state (rb_final, pwr_final) [E, N] of the envs `envs`, for the envs
    `converged` marks.  For every link that takes turns and every candidate the float64 floor test admits:

        Delta64 <= min_gain + BAR * (sum of weight * budget64 over the affected members) + (sum of their weights)

    The first term of the slack is the project's bar on a capacity, the second one bit per member for the floor().  The budget sum
    is taken in the candidate state and in the current one and the SMALLER of the two counts: whichever state the bound is read
    for, this slack is not wider.  A check is left out iff some affected member's float64 SINR lies within W of its floor or of its
    receiver sensitivity in either state.  Returns a namespace: checks, left_out (counts), worst (the largest left side less
    min_gain, over the slack: <= 1 passes), violations (list)."""
    envs = np.asarray(envs)
    mv = mask_of(move)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    sens = c.cols.sens_dbm[np.asarray(c.rx)]
    rb_final, pwr_final = np.asarray(rb_final, dtype=np.int64), np.asarray(pwr_final, dtype=np.int64)
    dem, wgt = planes_of(demand, weight, len(envs), c.n)
    takes = turn_links(rb_final, c.r, np.ones(c.n, bool), movable, allowed, mv)
    checks = left_out = 0
    worst, violations = -np.inf, []
    for x, e in enumerate(envs):
        if not converged[x]:
            continue
        for i in np.nonzero(takes[x])[0]:
            rb_rows, pwr_rows, slot_r, slot_q, valid = slots(rb_final[x:x + 1], pwr_final[x:x + 1], i, c.r, c.p_min[i], c.p_max[i], mv)
            valid = _slot_valid(valid, slot_r, rb_final[x:x + 1, i], None if allowed is None else allowed[i], c.r, mv)
            sinr, cap = oracle_planes(c, e, rb_rows[0], pwr_rows[0])
            _, delta, cand, aff = decide(sinr, cap, rb_final[x], i, slot_r[0], slot_q[0], valid[0], fl, dem[x], wgt[x], bits_per_mbps, min_gain,
                                         budget64)
            close = (np.abs(sinr - sens[None, :]) < W) | ((fl > NEG)[None, :] & (np.abs(sinr - fl[None, :]) < W))
            near = ((close | close[0][None, :]) & aff).any(axis=1)
            wb = wgt[x][None, :] * budget64(cap, bits_per_mbps)
            for k in np.nonzero(cand)[0]:
                checks += 1
                if near[k]:
                    left_out += 1
                    continue
                members = aff[k]
                slack = BAR * float(min(wb[k][members].sum(), wb[0][members].sum())) + float(wgt[x][members].sum())
                if slack == 0.0:                     # every affected weight is 0: Delta64 is 0 too
                    assert delta[k] == 0
                    continue
                over = (float(delta[k]) - min_gain) / slack
                worst = max(worst, over)
                if over > 1.0:
                    violations.append((int(e), int(i), int(slot_r[0, k]), int(slot_q[0, k]), int(delta[k]), slack))
    return SimpleNamespace(checks=checks, left_out=left_out, worst=worst, violations=violations)

"""What the power-ascent tests share (test_ascent_cpu.py, test_gpu_ascent.py): the cases (the seeded states of power_control_util
under an adjustable set, floors and a start), the sequential float64 restatement `ascent_ref` on the oracle's step
(oracle/d2d_oracle.py), the exact host loop `ascent_by_evaluate` over env.evaluate(), and the fixed-point check `reference_check`.

The statement (include/d2d_ascent.h).  A link is on an RB iff 0 <= rb < R; the group of RB r is the set of links on r in ascending
link index.  A turn of the adjustable link i at the power vector p: for every level q of i's alphabet, T(q) is the sequential
double sum over the group of the members' capacities under p with p[i] = q; q is admissible iff q == p[i] or every member with a
floor above -inf has sinr(q) >= floor or sinr(p[i]) < floor; best is the lowest admissible level whose T is maximal among the
admissible ones (a NaN T is never chosen); the link moves iff T(best) - T(p[i]) > min_gain.  The adjustable links take turns in
ascending link index; a round that moves nobody ends the ascent, and so do max_rounds rounds that each moved a link.

WHY THE FLOAT64 RESTATEMENT IS NO TRAJECTORY YARDSTICK.  T is flat in the level near an interior optimum: in most envs some decision
has a runner-up within 1e-5 relative of the winner, which float32 capacities may legitimately rank the other way, and the runs then
part.  The restatement checks properties of the outcome; the path is checked word for word against `ascent_by_evaluate`, whose
every capacity is a float32 value evaluate() produces.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import power_control_util as pcu
from gym_d2d_amd.power_ascent import STARTS          # the names of `start` are the module's
from oracle import d2d_oracle as orc

W, CAP, BAR = pcu.W, pcu.CAP, pcu.BAR
NEG = -np.inf
FLOORS = {'cue': 0.0, 'due': 5.0}

# name: (case of power_control_util, envs, every: adjustable = the agent links j with j % every == 0)
CASES = {
    'n37_r5': ('n37_r5', 16, 1),                 # mixed group sizes; N no multiple of the wave
    'n20_r64': ('n20_r64', 16, 1),               # empty RBs; links alone; the cap
    'n96_r1': ('n96_r1', 2, 1),                  # one group: one wave does all the work
    'n50_r6_hata': ('n50_r6_hata', 8, 1),        # the pow-k law
    'n50_r6_ld35': ('n50_r6_ld35', 8, 1),
    'n50_r6_no_rb': ('n50_r6_no_rb', 8, 1),      # a link on no RB
    'n300_r7': ('n300_r7', 4, 5),                # more links than threads
    'n1000_r64_ld35': ('n1000_r64_ld35', 2, 16),  # past 64 KiB of LDS
}
MIXED = ('n50_r6_mixed', 8, 1)                   # the general power law: no oracle model, exact checks only


def floor_vector(floor, cues, dues):
    """float32 [N]: None is -inf everywhere."""
    if floor is None:
        return np.full(cues + dues, NEG, dtype=np.float32)
    return pcu.target_vector(floor, cues, dues).astype(np.float32)


def adjustable_mask(n, every):
    return np.arange(n) % every == 0


def start_powers(pwr, on, adj, p_min, p_max, start):
    """The vector the ascent begins at: held, p_min or p_max for the adjustable links on an RB, held for every other link."""
    assert start in STARTS, start
    pwr = np.asarray(pwr, dtype=np.int64)
    take = on & adj[None, :]
    if start == 'held':
        return pwr.copy()
    return np.where(take, np.asarray(p_min if start == 'min' else p_max)[None, :], pwr)


def sequential_sum(a, axis=-1):
    """The double sum of `a` along `axis` in index order (np.sum adds pairwise)."""
    a = np.asarray(a, dtype=np.float64)
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis) if a.shape[axis] else np.zeros(np.delete(a.shape, axis))


def choose(total, sinr, cur, floor):
    """One turn's choice.  total [L] double; sinr [L, G] (the members' sinr_db at every level, in the precision of the caller);
    cur: the index of the current level; floor [G] in the same precision.  Returns (best index or None, admissible bool [L])."""
    with np.errstate(invalid='ignore'):
        held = (sinr >= floor[None, :]) | (sinr[cur] < floor)[None, :] | ~(floor > NEG)[None, :]
    adm = held.all(axis=1)
    adm[cur] = True
    ok = adm & ~np.isnan(total)
    if not ok.any():
        return None, adm
    top = total[ok].max()
    return int(np.nonzero(ok & (total == top))[0][0]), adm


# ------------------------------------------------------------------------------------------ the float64 restatement
_tables = {}


def _table_spec(c, e):
    """The oracle's path loss of env e between every two devices, evaluated once by the oracle's own formula on the oracle's own
    distance and handed back to its step as a 'table' spec: a turn then gathers instead of taking G^2 L logarithms again."""
    key = (c.name, int(e))
    if key not in _tables:
        pos = c.pos[e].astype(np.float64)
        d = pos[:, None, :] - pos[None, :, :]
        dist = (d[..., 0] ** 2 + d[..., 1] ** 2) ** 0.5
        with np.errstate(divide='ignore', invalid='ignore'):
            tab = orc.path_loss_db(c.spec, dist, c.cols.ant_h_m[:, None], c.cols.ant_h_m[None, :])
        _tables[key] = orc.PathLossSpec('table', table_db=tab)
    return _tables[key]


def group_tables(c, e, members, p, i_local, levels):
    """The oracle's step for the group `members` of env e under p with member i_local at every level: (sinr_db, capacity_mbps)
    float64 [L, G]."""
    lv, g = len(levels), len(members)
    pw = np.repeat(np.asarray(p, dtype=np.float64)[members][None, :], lv, axis=0)
    pw[:, i_local] = levels
    pos = np.broadcast_to(c.pos[e].astype(np.float64), (lv,) + c.pos[e].shape)
    out = orc.step(pos, np.asarray(c.tx)[members], np.asarray(c.rx)[members], np.zeros((lv, g), dtype=np.int64), pw, c.cols,
                   _table_spec(c, e), chunk=lv)
    return out['sinr_db'], out['capacity_mbps']


def ascent_ref(c, envs, adjustable=None, floor=None, start='held', min_gain=0.0, max_rounds=16):
    """The sequential statement in float64 on the oracle's step, env by env.  Returns a namespace: power_dbm int [E, N], rounds,
    moves int [E], converged bool [E], raised: list of (env, link, T before, T after) per move, floor_changed bool [E] (some turn's
    choice differs from what it would have been without floors), start int [E, N]."""
    envs = np.asarray(envs)
    n, r = c.n, c.r
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    adj_all = np.ones(n, bool) if adjustable is None else np.asarray(adjustable, dtype=bool)
    rb = np.asarray(c.rb)[envs]
    on = (rb >= 0) & (rb < r)
    p0 = start_powers(np.asarray(c.pwr)[envs], on, adj_all, c.p_min, c.p_max, start)
    power = p0.copy()
    rounds, moves = np.zeros(len(envs), dtype=np.int64), np.zeros(len(envs), dtype=np.int64)
    conv, changed, raised = np.zeros(len(envs), dtype=bool), np.zeros(len(envs), dtype=bool), []
    for x, e in enumerate(envs):
        p = power[x]
        turns = [i for i in range(n) if adj_all[i] and on[x, i]]
        groups = {i: np.nonzero(on[x] & (rb[x] == rb[x, i]))[0] for i in turns}
        for _ in range(max_rounds):
            moved = False
            for i in turns:
                members = groups[i]
                levels = np.arange(c.p_min[i], c.p_max[i] + 1)
                sinr, cap = group_tables(c, e, members, p, int(np.searchsorted(members, i)), levels)
                total = sequential_sum(cap, axis=1)
                cur = int(p[i] - c.p_min[i])
                best, _ = choose(total, sinr, cur, fl[members])
                free, _ = choose(total, sinr, cur, np.full(len(members), NEG))
                changed[x] |= best != free
                if best is not None and total[best] - total[cur] > min_gain:
                    raised.append((int(e), i, float(total[cur]), float(total[best])))
                    p[i] = levels[best]
                    moved = True
                    moves[x] += 1
            if not moved:
                conv[x] = True
                break
            rounds[x] += 1
    return SimpleNamespace(power_dbm=power, rounds=rounds, moves=moves, converged=conv, raised=raised, floor_changed=changed, start=p0,
                           on_rb=on)


@lru_cache(maxsize=None)
def reference(name, floors=False, start='held'):
    """ascent_ref of a row of CASES on its envs, computed once."""
    case, b, every = CASES[name]
    c = pcu.make_case(case)
    return ascent_ref(c, np.arange(b), adjustable_mask(c.n, every), FLOORS if floors else None, start)


def reference_check(c, envs, power, converged, adjustable=None, floor=None, min_gain=0.0, start_power=None):
    """The fixed-point inequality of the float64 oracle at the powers `power` [E, N] (of the envs `envs`), for the envs `converged`
    marks.  For every adjustable link i on an RB and every level q that the float64 floor test admits:

        T64(q) - T64(cur) <= min_gain + 2 BAR (max(T64(q), T64(cur)) + G)

    G the group's size: what a per-capacity deviation of BAR max(|ref|, 1) allows on two group sums.  A (link, level) check is left
    out iff some member's float64 SINR lies within W of its floor or of its receiver sensitivity, at q or at the current level.
    Returns a namespace: checks, left_out (counts), worst (the largest left side less min_gain, over the bound's slack term: <= 1
    passes), violations (list), and floors_kept: every link that clears its floor by more than W at start_power is at or above
    floor - W at `power` (None without start_power)."""
    envs = np.asarray(envs)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    adj_all = np.ones(c.n, bool) if adjustable is None else np.asarray(adjustable, dtype=bool)
    sens_all = c.cols.sens_dbm[np.asarray(c.rx)]
    checks = left_out = 0
    worst, violations, kept = -np.inf, [], None
    for x, e in enumerate(envs):
        if not converged[x]:
            continue
        rb = np.asarray(c.rb)[e]
        on = (rb >= 0) & (rb < c.r)
        p = np.asarray(power[x], dtype=np.int64)
        for i in np.nonzero(adj_all & on)[0]:
            members = np.nonzero(on & (rb == rb[i]))[0]
            levels = np.arange(c.p_min[i], c.p_max[i] + 1)
            sinr, cap = group_tables(c, e, members, p, int(np.searchsorted(members, i)), levels)
            total = sequential_sum(cap, axis=1)
            cur = int(p[i] - c.p_min[i])
            f, sens = fl[members], sens_all[members]
            _, adm = choose(total, sinr, cur, f)
            near = (np.abs(sinr - sens[None, :]) < W) | ((f > NEG)[None, :] & (np.abs(sinr - f[None, :]) < W))
            near = near.any(axis=1)
            near = near | near[cur]
            for q in range(len(levels)):
                if q == cur or not adm[q]:
                    continue
                checks += 1
                if near[q]:
                    left_out += 1
                    continue
                slack = 2 * BAR * (max(total[q], total[cur]) + len(members))
                over = (total[q] - total[cur] - min_gain) / slack
                worst = max(worst, over)
                if over > 1.0:
                    violations.append((int(e), int(i), int(levels[q]), float(total[q]), float(total[cur])))
    if start_power is not None:
        kept = True
        for x, e in enumerate(envs):
            rb = np.asarray(c.rb)[e]
            on = (rb >= 0) & (rb < c.r)
            rb_eff = np.where(on, rb, c.r + np.arange(c.n))
            s0, s1 = (orc.step(c.pos[e][None], c.tx, c.rx, rb_eff[None], np.asarray(v[x])[None], c.cols, c.spec)['sinr_db'][0]
                      for v in (start_power, power))
            clear = on & (fl > NEG) & (s0 > fl + W)
            kept = kept and bool((s1[clear] >= fl[clear] - W).all())
    return SimpleNamespace(checks=checks, left_out=left_out, worst=worst, violations=violations, floors_kept=kept)


# ------------------------------------------------------------------------------------------ the exact host loop over evaluate()
def ascent_by_evaluate(env, adjustable=None, floor=None, start='held', min_gain=0.0, max_rounds=16):
    """The statement as a host loop: one env.evaluate() call per link turn with K = the link's levels candidates (every env takes
    link i's turn in the same call), T the sequential double sum of the float32 capacity plane over the group, the floor
    comparisons in float32 on the sinr_db plane.  Returns host arrays (power_dbm int32, sinr_db, capacity_mbps float32 [B, N],
    rounds, moves int32 [B], converged uint8 [B]) and the number of evaluate() calls."""
    import torch
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    rb = env._t['rb'].cpu().numpy().astype(np.int64)
    held = env._t['pwr'].cpu().numpy().astype(np.int64)
    p_min, p_max = (np.asarray(a, dtype=np.int64) for a in env._class_bounds())
    adj = np.arange(n) >= n - env.num_agents
    if adjustable is not None:
        adj = adj & np.asarray(adjustable.cpu() if torch.is_tensor(adjustable) else adjustable, dtype=bool)
    fl = floor_vector(floor, env.num_cues, n - env.num_cues)
    on = (rb >= 0) & (rb < r)
    p = start_powers(held, on, adj, p_min, p_max, start)
    rb_dev = torch.as_tensor(rb.astype(np.int32), device=env.device)
    rounds, moves = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32)
    conv, live, calls = np.zeros(b, dtype=np.uint8), np.ones(b, dtype=bool), 0
    for _ in range(max_rounds):
        moved = np.zeros(b, dtype=bool)
        for i in np.nonzero(adj)[0]:
            turn = live & on[:, i]
            if not turn.any():
                continue
            levels = np.arange(p_min[i], p_max[i] + 1)
            cand = np.repeat(p[:, None, :], len(levels), axis=1)
            cand[:, :, i] = levels[None, :]
            res = env.evaluate(rb_dev[:, None, :].expand(b, len(levels), n).contiguous(),
                               torch.as_tensor(cand.astype(np.int32), device=env.device))
            calls += 1
            sinr, cap = res['sinr_db'].cpu().numpy(), res['capacity_mbps'].cpu().numpy()
            assert sinr.dtype == cap.dtype == np.float32
            for e in np.nonzero(turn)[0]:
                members = np.nonzero(on[e] & (rb[e] == rb[e, i]))[0]
                total = sequential_sum(cap[e][:, members], axis=1)
                cur = int(p[e, i] - p_min[i])
                best, _ = choose(total, sinr[e][:, members], cur, fl[members])
                if best is not None and total[best] - total[cur] > min_gain:
                    p[e, i] = levels[best]
                    moved[e] = True
                    moves[e] += 1
        conv[live & ~moved] = 1
        rounds[live & moved] += 1
        live &= moved
        if not live.any():
            break
    res = env.evaluate(rb_dev[:, None, :].contiguous(), torch.as_tensor(p[:, None, :].astype(np.int32), device=env.device))
    sinr, cap = res['sinr_db'].cpu().numpy()[:, 0].copy(), res['capacity_mbps'].cpu().numpy()[:, 0].copy()
    return (p.astype(np.int32), sinr, cap, rounds, moves, conv), calls + 1

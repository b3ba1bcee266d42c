"""What the table RB-ascent tests share (test_table_rb_ascent_cpu.py, test_gpu_table_rb_ascent.py): the cases (drawn tables of
table_evaluate_util.draw_table with seeded start planes), the exact host loop `table_rb_ascent_by_evaluate` over
env.evaluate_table(), the sequential float64 restatement `rb_ascent_ref` and the fixed-point check `reference_check`, both on the
oracle's step formulas on a table by link pair (table_route_util.table_step_ref).

The statement is rb_ascent_util's (include/d2d_rbascent.h) with one substitution: the planes of (rb^r, pwr) are evaluate_table()'s on
the table (include/d2d_tabascent.h).  The turn itself - `decide`, `candidates`, `presence`, `sets` - is rb_ascent_util's, unchanged:
the exact loop feeds it evaluate_table()'s float32 planes, the restatement the float64 ones.  As there, the float64 restatement is no
trajectory yardstick: it checks properties of the outcome; the path is checked word for word against the host loop.

The tables are drawn per (env, j, i), every entry on its own: not symmetric, so a transposed or mis-pitched gain block shows.  A
float32 case holds the float32 rounding of its draw and the reference reads the rounded values.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import power_control_util as pcu
import rb_ascent_util as ru
import table_evaluate_util as teu
import table_route_util as tru
from oracle import d2d_oracle as orc

W, CAP, BAR = ru.W, ru.CAP, ru.BAR
NEG = ru.NEG
FLOORS = ru.FLOORS
NAMES = ('rb', 'sinr_db', 'capacity_mbps', 'rounds', 'moves', 'converged', 'domain')
sequential_sum, floor_vector = ru.sequential_sum, ru.floor_vector
decide, candidates, presence, sets = ru.decide, ru.candidates, ru.presence, ru.sets

# name: (cues, due pairs, R, envs, every: movable = the agent links j with j % every == 0, entry type, rows per env beyond N (1: the
# live layout, whose last row is NaN and never read), links on no RB: one at -1 and one at R)
CASES = {
    'n3_r1': (1, 2, 1, 3, 1, 'float64', 0, False),             # no candidate: zero moves, converged
    'n37_r5': (12, 25, 5, 16, 1, 'float64', 1, False),         # the basic case
    'n37_r5_f32': (12, 25, 5, 16, 1, 'float32', 0, False),
    'n20_r64': (6, 14, 64, 4, 1, 'float32', 0, False),         # more RBs than links
    'n20_r300': (6, 14, 300, 3, 1, 'float64', 0, False),       # more RBs than threads; the last allowed word partly filled
    'n96_r2': (32, 64, 2, 2, 1, 'float32', 1, False),          # two groups near 48
    'n300_r7': (100, 200, 7, 2, 5, 'float64', 1, False),       # more links than threads; ten bitset words
    'n50_r6_no_rb': (20, 30, 6, 4, 1, 'float32', 1, True),     # one link at rb -1 and one at R
    'n1000_r320': (300, 700, 320, 2, 25, 'float32', 0, False),  # past 64 KiB of LDS by the header's formula
}
NO_RB = (7, 11)                                  # the links of a no_rb case at rb = -1 and rb = R, in every env


def lds_bytes(n, r, allowed=False):
    """The formula of include/d2d_tabascent.h."""
    r16 = lambda x: (x + 15) & ~15
    n4 = (n + 3) & ~3
    return 16 * n + 2 * r16(4 * n) + 8 * n4 + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 112


@lru_cache(maxsize=None)
def make_case(name):
    """The seeded case: table (what the kernel reads: [B, N + extra, N] of the entry type, a NaN last row when extra), pl (what the
    references read: the entries as float64), the start planes rb / pwr int32 [B, N], the link list and the oracle's columns."""
    cues, dues, r, b, every, dtype, extra, no_rb = CASES[name]
    n = cues + dues
    rng = np.random.default_rng([sum(map(ord, name)), n, r, b])
    draw = teu.draw_table(rng, b, n)
    table = np.full((b, n + extra, n), np.nan, dtype=dtype)
    table[:, :n] = draw
    _, _, levels = pcu.bounds(cues, dues)
    rb = rng.integers(0, r, (b, n)).astype(np.int32)
    pwr = rng.integers(0, levels, (b, n)).astype(np.int32)
    if no_rb:
        rb[:, NO_RB[0]], rb[:, NO_RB[1]] = -1, r
    tx, rx, _ = tru.orc_links(cues, dues)
    c = SimpleNamespace(name=name, cues=cues, dues=dues, n=n, r=r, b=b, every=every, dtype=dtype, extra=extra, table=table,
                        pl=table[:, :n].astype(np.float64), rb=rb, pwr=pwr, tx=tx, rx=rx,
                        cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))
    for v in (c.table, c.pl, c.rb, c.pwr):
        v.setflags(write=False)
    return c


def movable_mask(c):
    return None if c.every == 1 else ru.movable_mask(c.n, c.every)


def domain_of(table, n):
    """int32 [B]: 1 iff an entry [j, i], j, i < n, of the env's block fails x > -inf."""
    with np.errstate(invalid='ignore'):
        return (~(np.asarray(table)[:, :n, :n] > NEG)).any(axis=(1, 2)).astype(np.int32)


# ------------------------------------------------------------------------------------------ the float64 restatement
def oracle_planes(c, e, rb_rows, pwr):
    """The float64 (sinr_db, capacity_mbps) [K, N] of env e for the assignments rb_rows [K, N] by the oracle's step formulas on the
    env's table (table_route_util.table_step_ref); a link on no RB shares its pseudo RB with nobody."""
    rb_rows = np.asarray(rb_rows, dtype=np.int64)
    k, n = rb_rows.shape
    on = (rb_rows >= 0) & (rb_rows < c.r)
    rb_eff = np.where(on, rb_rows, c.r + np.arange(n)[None, :])
    with np.errstate(divide='ignore', invalid='ignore'):
        out = tru.table_step_ref(c.pl[e][None], None, rb_eff, np.repeat(np.asarray(pwr, dtype=np.float64)[None, :], k, axis=0), c.cols,
                                 c.tx, c.rx)
    return out['sinr_db'], out['capacity_mbps']


def rb_ascent_ref(c, envs, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """rb_ascent_util.rb_ascent_ref with the planes of oracle_planes: the sequential statement in float64, env by env.  Returns a
    namespace: rb int [E, N], rounds, moves int [E], converged bool [E], raised: list of (env, link, the env's oracle total before,
    after) per move, kept: list of (env, link moved, bool: every member of the RB it left or joined that met its floor before the
    move meets it after), start int [E, N]."""
    envs = np.asarray(envs)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    rb0 = np.asarray(c.rb)[envs].astype(np.int64)
    rb_all = rb0.copy()
    rounds, moves = np.zeros(len(envs), dtype=np.int64), np.zeros(len(envs), dtype=np.int64)
    conv, raised, kept = np.zeros(len(envs), dtype=bool), [], []
    every = np.ones(c.r, bool)
    for x, e in enumerate(envs):
        rb = rb_all[x]
        turns = ru._turns(c, rb, allowed, movable)
        for _ in range(max_rounds):
            moved = False
            for i in turns:
                sinr, cap = oracle_planes(c, e, candidates(rb, i, c.r), c.pwr[e])
                to, _, _, _ = decide(sinr, cap, rb, i, every if allowed is None else allowed[i], fl, min_gain)
                if to is not None:
                    cur = int(rb[i])
                    raised.append((int(e), i, float(sequential_sum(cap[cur])), float(sequential_sum(cap[to]))))
                    met = (fl > NEG) & (sinr[cur] >= fl) & ((rb == to) | (np.arange(c.n) == i))
                    kept.append((int(e), i, bool((sinr[to][met] >= fl[met]).all())))
                    rb[i] = to
                    moved = True
                    moves[x] += 1
            if not moved:
                conv[x] = True
                break
            rounds[x] += 1
    return SimpleNamespace(rb=rb_all, rounds=rounds, moves=moves, converged=conv, raised=raised, kept=kept, start=rb0)


@lru_cache(maxsize=None)
def reference(name, floors=False, max_rounds=16):
    """rb_ascent_ref of a case on all its envs, computed once."""
    c = make_case(name)
    return rb_ascent_ref(c, np.arange(c.b), None, movable_mask(c), FLOORS if floors else None, 0.0, max_rounds)


def reference_check(c, envs, rb_final, converged, allowed=None, movable=None, floor=None, min_gain=0.0):
    """rb_ascent_util.reference_check with the planes of oracle_planes: the fixed-point inequality of the float64 reference at the
    RBs `rb_final` [E, N], for the envs `converged` marks.  For every movable link i on RB c and every candidate r that the float64
    floor test admits:

        D64(r) - D64(c) <= min_gain + BAR * sum(T64 + group size)

    over the four group sums involved (With(r), Without(r), With(c), Without(c)).  A check is left out iff some member's float64
    SINR lies within W of its floor or of its receiver sensitivity in either state.  Returns a namespace: checks, left_out (counts),
    worst (the largest left side less min_gain, over the bound's slack term: <= 1 passes), violations (list)."""
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
        for i in ru._turns(c, rb, allowed, movable):
            cur = int(rb[i])
            sinr, cap = oracle_planes(c, e, candidates(rb, i, c.r), c.pwr[e])
            _, d, cand, _ = decide(sinr, cap, rb, i, every if allowed is None else allowed[i], fl, min_gain)
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


# ------------------------------------------------------------------------------------------ the exact host loop over evaluate_table()
def table_rb_ascent_by_evaluate(env, table, rb, pwr, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """rb_ascent_util.rb_ascent_by_evaluate over env.evaluate_table(..., table=): one call per link turn with K = R candidates
    (candidate r has rb[i] = r; every env takes link i's turn in the same call), the sums sequential double sums of the float32
    capacity plane over the member sets the statement names, the floor comparisons in float32 on the sinr_db plane.  table: the device
    tensor (or None: the live table); rb, pwr: the start planes, device tensors int32 [B, N].  Returns host arrays (rb int32, sinr_db,
    capacity_mbps float32 [B, N], rounds, moves int32 [B], converged uint8 [B], domain int32 [B]) and the number of evaluate_table()
    calls."""
    import torch
    from gym_d2d_amd import table_evaluate
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    rb = rb.cpu().numpy().astype(np.int64)
    pwr = pwr.contiguous()
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
            res = env.evaluate_table(torch.as_tensor(cand.astype(np.int32), device=env.device), pwr_k, table=table)
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
    res = env.evaluate_table(torch.as_tensor(rb[:, None, :].astype(np.int32), device=env.device), pwr[:, None, :].contiguous(), table=table)
    sinr, cap = res['sinr_db'].cpu().numpy()[:, 0].copy(), res['capacity_mbps'].cpu().numpy()[:, 0].copy()
    tab = table_evaluate.live_table(env.simulator) if table is None else table
    return (rb.astype(np.int32), sinr, cap, rounds, moves, conv, domain_of(tab.cpu().numpy(), n)), calls + 1

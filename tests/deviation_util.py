"""What the deviation tests share (test_deviation_cpu.py, test_gpu_deviation.py): the case table, `lds_bytes`, the NumPy restatement
of include/d2d_deviate.h on evaluate()-style planes of any precision, and the two ways to fill those planes - `by_evaluate` from
env.evaluate() launches (float32, the exact yardstick) and `by_oracle` from the float64 oracle (oracle/d2d_oracle.py).

The statement.  For a selected link i on RB c at power p, an RB r and a level l (power q = p_min[i] + l): s^(r,q) is the held state
with rb[i] = r, pwr[i] = q.  With(r,q) is the sequential double sum of cap(s^(r,q)) over group(r) u {i}, Without(r) the one over
group(r) \\ {i} with i on no RB, D = With - Without, gain(r,q) = D(r,q) - D(c,p).  (r,q) is admissible iff it is (c,p) or every m
of group(r) u {i} with a floor above -inf has sinr_m(s^(r,q)) >= floor or sinr_m(s) < floor.  An entry is open iff l < L_i,
allowed[i][r] or r == c, it is admissible and link i is on an RB.  The table holds -inf where closed, else gain rounded once to
float32.  best is the open entry other than (c,p) of maximal double gain, ties to the lowest power, then the lowest RB, a NaN never
chosen; it is taken iff gain(best) > min_gain, else the held action with 0.0; regret is the largest gain of the env, leader the
lowest link that has it, -1 when nobody would move.

The planes of one selected link are the K = R Lmax + 1 single-link variants of the state: row r Lmax + l is s^(r, p_min + min(l,
L_i - 1)) (the columns behind L_i repeat the last level and are closed), the last row is link i on rb -1, which gives Without.  The
held state s is the row (c, p - p_min): the envs hold a power inside the alphabet.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import ascent_util as au
import power_control_util as pcu
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

BAR = pcu.BAR                                        # the project's bar: |d| <= BAR max(|ref|, 1)
THRESHOLD_DB = 1e-4                                  # evaluate_util's / assignpwr_util's: an SINR this close to a sensitivity or a floor
MARK_CAP = 0.01                                      # ... marks the entry; at most this share of a case's entries
NEG = -np.inf
FLOOR_SETTINGS = {'none': None, 'cue0': {'cue': 0.0, 'due': NEG}, 'below': {'cue': 0.0, 'due': 5.0}}
sequential_sum = au.sequential_sum
floor_vector = au.floor_vector

# name: cues, dues, R, law, cell radius m, envs, links put on no RB, CUE max dBm, DUE max dBm (levels = max + 1), and what the
# float64 side takes of it: `oracle` = (envs, every: the selected links j % every == 0 of the agents) - an oracle launch is K N^2
CASES = {
    'd6_r4': dict(cues=3, dues=3, r=4, law='ld2', cell=500.0, b=4, no_rb=0, cue_max=23, due_max=20, oracle=(4, 1)),          # fewer entries than a wave
    'd50_r25': dict(cues=25, dues=25, r=25, law='urban', cell=500.0, b=4, no_rb=1, cue_max=23, due_max=20, oracle=(2, 7)),   # config 2's shape; a link on no RB
    'd130_r70': dict(cues=65, dues=65, r=70, law='ld2', cell=500.0, b=3, no_rb=0, cue_max=23, due_max=20, oracle=(1, 31)),   # several waves and chunks; 3 allowed words
    'd40_r1': dict(cues=16, dues=24, r=1, law='mixed', cell=500.0, b=2, no_rb=0, cue_max=23, due_max=20, oracle=None),       # no RB candidates; one 40-member group
    'd40_r2': dict(cues=16, dues=24, r=2, law='ld35', cell=120.0, b=2, no_rb=0, cue_max=23, due_max=20, oracle=(2, 5)),      # groups past 32 members
    'd16_r8_lv': dict(cues=8, dues=8, r=8, law='mixed', cell=500.0, b=2, no_rb=0, cue_max=63, due_max=0, oracle=None),       # 64 levels and 1 level: padding
    'd300_r8': dict(cues=100, dues=200, r=8, law='ld2', cell=500.0, b=2, no_rb=0, cue_max=23, due_max=20, oracle=(1, 37)),   # several workgroups per env; long groups
}
SUBSET_CASE = 'd130_r70'                             # the GPU test selects a non-contiguous subset of its links
LAWS = {'ld2': 0, 'mixed': 1, 'urban': 2, 'ld35': 2}  # the kernel's law id


def lds_bytes(n, r, allowed=False):
    """The header's formula, restated: 80 n + has_allowed round16(4 n ceil(r / 32)) + round16(4 ceil(n / 32) r) + 5216."""
    r16 = lambda x: (x + 15) // 16 * 16
    return 80 * n + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 5216


def build_case(name, k):
    """The seeded state of the case dict `k` (a CASES entry, or one in its form) under the seed its name gives, in
    power_control_util's form, with the case's own alphabets."""
    cues, dues, r = k['cues'], k['dues'], k['r']
    n = cues + dues
    levels = np.array([k['cue_max'] + 1] * cues + [k['due_max'] + 1] * dues)
    rng = np.random.default_rng(sum(map(ord, name)))
    pos = random_layout(rng, k['b'], cues, dues, cell_radius=k['cell'])
    raw = rng.integers(0, r * levels, (k['b'], n))
    if name == 'd40_r2':                             # 35 of the 40 links on RB 0: a group past 32 members
        raw[:, :35] %= levels[:35]
    if k['no_rb']:
        raw[:, n - k['no_rb']:] = r * levels[n - k['no_rb']:] + rng.integers(0, levels[n - k['no_rb']:], (k['b'], k['no_rb']))
    rb, pwr = orc.decode_actions(raw, levels)
    tx, rx, _ = default_links(cues, dues)
    spec = pcu.models()[k['law']][1]
    cfgs = orc.device_configs(cues, dues, cue_max_tx_power_dBm=k['cue_max'], due_max_tx_power_dBm=k['due_max'])
    return SimpleNamespace(name=name, cues=cues, dues=dues, n=n, r=r, law=k['law'], cell=k['cell'], b=k['b'], pos=pos,
                           raw=raw.astype(np.int32), rb=rb.astype(np.int32), pwr=pwr.astype(np.int32), tx=tx, rx=rx,
                           p_min=np.zeros_like(levels), p_max=levels - 1, levels=levels, spec=spec, cols=orc.device_columns(*cfgs[1:]),
                           cue_max=k['cue_max'], due_max=k['due_max'])


@lru_cache(maxsize=None)
def make_case(name):
    """build_case of a CASES entry, computed once."""
    return build_case(name, CASES[name])


def env_config(c):
    """The env_config of a case."""
    return {'num_rbs': c.r, 'num_cues': c.cues, 'num_due_pairs': c.dues, 'path_loss_model': pcu.models()[c.law][0],
            'cue_max_tx_power_dBm': c.cue_max, 'due_max_tx_power_dBm': c.due_max}


def oracle_links(name):
    """(envs, links) the float64 side takes of a case; None where the law has no oracle model."""
    if CASES[name]['oracle'] is None:
        return None
    envs, every = CASES[name]['oracle']
    return np.arange(envs), np.arange(CASES[name]['cues'] + CASES[name]['dues'])[::every]


def allowed_mask(n, r, seed, rb=None):
    """A random bool [N, R]: a fifth of the rows all zero, and, with rb [N], every third link's own RB excluded."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, r)) < 0.6
    mask[rng.random(n) < 0.2] = False
    if rb is not None:
        for i in range(0, n, 3):
            if 0 <= rb[i] < r:
                mask[i, rb[i]] = False
    return mask


# ------------------------------------------------------------------------------------------ the variants of one link
def variants(rb, pwr, i, r_count, lo, lv, lmax):
    """(rb_rows, pwr_rows) int [E, K, N], K = R Lmax + 1, of link i for the states rb, pwr int [E, N]: row r Lmax + l has rb[i] =
    r, pwr[i] = lo + min(l, lv - 1); the last row has link i on rb -1."""
    e, n = rb.shape
    k = r_count * lmax + 1
    rb_rows, pwr_rows = np.repeat(rb[:, None, :], k, axis=1), np.repeat(pwr[:, None, :], k, axis=1)
    rb_rows[:, :k - 1, i] = np.repeat(np.arange(r_count), lmax)[None, :]
    pwr_rows[:, :k - 1, i] = (lo + np.minimum(np.tile(np.arange(lmax), r_count), lv - 1))[None, :]
    rb_rows[:, k - 1, i] = -1
    return rb_rows, pwr_rows


# ------------------------------------------------------------------------------------------ the restatement, one env and one link
def link_row(sinr, cap, rb, pwr, i, r_count, lo, lv, lmax, allowed_i, floor):
    """One link of one env on the planes sinr, cap [K, N] of `variants` (any precision; floor [N] in the planes').  Returns a
    namespace: with_, gain float64 [R, Lmax], without float64 [R], open, adm bool [R, Lmax], held (r, l) or None, on bool."""
    c, p = int(rb[i]), int(pwr[i])
    k = r_count * lmax + 1
    on = 0 <= c < r_count
    ns = SimpleNamespace(on=on, held=None, with_=np.zeros((r_count, lmax)), without=np.zeros(r_count), gain=np.zeros((r_count, lmax)),
                         open=np.zeros((r_count, lmax), bool), adm=np.zeros((r_count, lmax), bool))
    if not on:
        return ns
    assert lo <= p < lo + lv, 'the held power lies inside the alphabet'
    m = rb[None, :] == np.arange(r_count)[:, None]                       # group(r) \ {i}
    m[:, i] = False
    w = m.copy()                                                         # group(r) u {i}
    w[:, i] = True
    cap64 = np.asarray(cap, dtype=np.float64)
    planes = cap64[:k - 1].reshape(r_count, lmax, -1)
    ns.with_ = sequential_sum(np.where(w[:, None, :], planes, 0.0), axis=2)          # a link outside the set adds 0.0
    ns.without = sequential_sum(np.where(m, cap64[k - 1][None, :], 0.0), axis=1)
    ns.held = (c, p - lo)
    with np.errstate(invalid='ignore'):
        d = ns.with_ - ns.without[:, None]
        ns.gain = d - d[ns.held]
        s = sinr[:k - 1].reshape(r_count, lmax, -1)
        now = sinr[c * lmax + (p - lo)]                                  # sinr_m(s)
        f = floor[None, None, :]
        ok = ~(f > NEG) | (s >= f) | (now[None, None, :] < f)
    ns.adm = (ok | ~w[:, None, :]).all(axis=2)
    ns.adm[ns.held] = True
    may = np.ones(r_count, bool) if allowed_i is None else np.asarray(allowed_i, dtype=bool).copy()
    may[c] = True
    ns.open = ns.adm & may[:, None] & (np.arange(lmax) < lv)[None, :]
    return ns


def best_of(ns, min_gain):
    """(r, l, gain) of the best deviation of a link_row, or None where the link stays."""
    if not ns.on:
        return None
    cand = ns.open & ~np.isnan(ns.gain)
    cand[ns.held] = False
    if not cand.any():
        return None
    top = ns.gain[cand].max()
    rr, ll = np.nonzero(cand & (ns.gain == top))
    x = np.lexsort((rr, ll))[0]                                          # the lowest power, then the lowest RB
    return (int(rr[x]), int(ll[x]), float(top)) if top > min_gain else None


def restate(fill, rb, pwr, links, r_count, p_min, p_max, settings, dtype=np.float32):
    """The statement on the planes `fill(i, rb_rows, pwr_rows)` -> (sinr, cap) [E, K, N] gives for link i's variants, under every
    setting (allowed bool [N, R] or None, floor [N], min_gain) of `settings`: the planes are filled once per link and serve them
    all.  rb, pwr int [E, N].  Returns one namespace per setting: table float32 [E, M, R, Lmax], gain float64 [E, M, R, Lmax], open
    bool [E, M, R, Lmax], rb_out, pwr_out int32 [E, N], gain_link float64 [E, N], regret float64 [E], leader int32 [E], rows (the
    link_row namespaces, [E][M]), lmax, links."""
    rb, pwr = np.asarray(rb, dtype=np.int64), np.asarray(pwr, dtype=np.int64)
    e_count, n = rb.shape
    links = np.asarray(links, dtype=np.int64)
    lv_all = (np.asarray(p_max, dtype=np.int64) - np.asarray(p_min, dtype=np.int64) + 1)
    lmax = int(lv_all[links].max())
    shape = (e_count, len(links), r_count, lmax)
    out = [SimpleNamespace(table=np.full(shape, NEG, dtype=np.float32), gain=np.zeros(shape), open=np.zeros(shape, bool),
                           rb_out=rb.astype(np.int32).copy(), pwr_out=pwr.astype(np.int32).copy(), gain_link=np.zeros((e_count, n)),
                           rows=[[None] * len(links) for _ in range(e_count)], lmax=lmax, links=links) for _ in settings]
    for a, i in enumerate(links):
        lo, lv = int(p_min[i]), int(lv_all[i])
        rb_rows, pwr_rows = variants(rb, pwr, i, r_count, lo, lv, lmax)
        sinr, cap = fill(int(i), rb_rows, pwr_rows)
        assert sinr.dtype == cap.dtype == dtype and sinr.shape == rb_rows.shape
        for o, (allowed, floor, min_gain) in zip(out, settings):
            fl = np.asarray(floor).astype(dtype)
            for e in range(e_count):
                ns = link_row(sinr[e], cap[e], rb[e], pwr[e], i, r_count, lo, lv, lmax, None if allowed is None else allowed[i], fl)
                o.rows[e][a] = ns
                o.gain[e, a], o.open[e, a] = ns.gain, ns.open
                with np.errstate(over='ignore', invalid='ignore'):
                    o.table[e, a] = np.where(ns.open, ns.gain.astype(np.float32), np.float32(NEG))
                best = best_of(ns, min_gain)
                if best is not None:
                    o.rb_out[e, i], o.pwr_out[e, i], o.gain_link[e, i] = best[0], lo + best[1], best[2]
    for o in out:
        o.regret = o.gain_link.max(axis=1)
        o.leader = np.where(o.regret > 0.0, o.gain_link.argmax(axis=1), -1).astype(np.int32)    # argmax: the lowest link that has it
    return out


# ------------------------------------------------------------------------------------------ the planes from evaluate()
def by_evaluate(env, links=None, settings=((None, None, 0.0),), one_launch=False):
    """The statement on env.evaluate()'s float32 planes: one launch per selected link with K = R Lmax + 1 candidates, or
    (one_launch) one launch for all links.  settings: (allowed bool [N, R] or None, floor as floor_sinr_db takes it, min_gain) each.
    Returns restate()'s namespaces, one per setting, and the number of evaluate() calls."""
    import torch
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    rb = env._t['rb'].cpu().numpy().astype(np.int64)
    pwr = env._t['pwr'].cpu().numpy().astype(np.int64)
    p_min, p_max = (np.asarray(a, dtype=np.int64) for a in env._class_bounds())
    links = np.arange(n - env.num_agents, n) if links is None else np.asarray(links)
    host = lambda al: None if al is None else np.asarray(al.cpu() if torch.is_tensor(al) else al, dtype=bool)
    settings = [(host(al), floor_vector(fl, env.num_cues, n - env.num_cues), mg) for al, fl, mg in settings]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a.astype(np.int32)), device=env.device)
    calls = [0]
    planes = {}

    def launch(rb_rows, pwr_rows):
        res = env.evaluate(dev(rb_rows), dev(pwr_rows))
        calls[0] += 1
        return res['sinr_db'].cpu().numpy().copy(), res['capacity_mbps'].cpu().numpy().copy()

    if one_launch:
        lv = p_max - p_min + 1
        lmax = int(lv[links].max())
        rows = [variants(rb, pwr, i, r, int(p_min[i]), int(lv[i]), lmax) for i in links]
        sinr, cap = launch(np.concatenate([x[0] for x in rows], axis=1), np.concatenate([x[1] for x in rows], axis=1))
        k = r * lmax + 1
        for a, i in enumerate(links):
            planes[int(i)] = (sinr[:, a * k:(a + 1) * k], cap[:, a * k:(a + 1) * k])
    fill = (lambda i, rb_rows, pwr_rows: planes[i]) if one_launch else (lambda i, rb_rows, pwr_rows: launch(rb_rows, pwr_rows))
    return restate(fill, rb, pwr, links, r, p_min, p_max, settings, np.float32), calls[0]


# ------------------------------------------------------------------------------------------ the planes from the float64 oracle
def oracle_planes(c, e, rb_rows, pwr_rows):
    """The oracle's float64 (sinr_db, capacity_mbps) [K, N] of env e for the states (rb_rows, pwr_rows) [K, N]; a link on no RB shares
    its pseudo RB with nobody (goodput_ascent_util.oracle_planes)."""
    rb_rows = np.asarray(rb_rows, dtype=np.int64)
    k, n = rb_rows.shape
    on = (rb_rows >= 0) & (rb_rows < c.r)
    rb_eff = np.where(on, rb_rows, c.r + np.arange(n)[None, :])
    pos = np.broadcast_to(c.pos[e].astype(np.float64), (k,) + c.pos[e].shape)
    out = orc.step(pos, c.tx, c.rx, rb_eff, np.asarray(pwr_rows, dtype=np.float64), c.cols, au._table_spec(c, e), chunk=64)
    return out['sinr_db'], out['capacity_mbps']


def by_oracle(c, envs, links, allowed=None, floor=None, min_gain=0.0, rb=None, pwr=None, planes=None):
    """The statement on the float64 oracle's planes for the envs `envs` and the links `links` of a case, under one setting; `planes(c,
    e, i, rb_rows, pwr_rows)` fills link i's planes of env e in oracle_planes' place (deviation_large_util.restricted_planes).  Returns
    restate()'s namespace with three more fields: near bool [E, M, R, Lmax] (some member of group(r) u {i} has a float64 SINR within
    THRESHOLD_DB of its sensitivity or of its floor in the entry's state, in the held state or with i gone), delta float64 [E, M, R,
    Lmax] (the env's oracle total at s^(r,q) less the total at s, summed over ALL links) and total float64 [E] (the total at s)."""
    envs = np.asarray(envs)
    rb = (np.asarray(c.rb)[envs] if rb is None else np.asarray(rb)).astype(np.int64)
    pwr = (np.asarray(c.pwr)[envs] if pwr is None else np.asarray(pwr)).astype(np.int64)
    fl = floor_vector(floor, c.cues, c.dues).astype(np.float64)
    sens = c.cols.sens_dbm[np.asarray(c.rx)]
    kept = {}

    def fill(i, rb_rows, pwr_rows):
        both = [oracle_planes(c, e, rb_rows[x], pwr_rows[x]) if planes is None else planes(c, e, i, rb_rows[x], pwr_rows[x])
                for x, e in enumerate(envs)]
        kept[i] = (np.stack([s for s, _ in both]), np.stack([k for _, k in both]))
        return kept[i]

    res = restate(fill, rb, pwr, links, c.r, c.p_min, c.p_max, [(allowed, fl, min_gain)], np.float64)[0]
    lmax = res.lmax
    near, delta = np.zeros(res.open.shape, bool), np.zeros(res.open.shape)
    total = np.zeros(len(envs))
    for a, i in enumerate(res.links):
        sinr, cap = kept[int(i)]
        for x in range(len(envs)):
            ns = res.rows[x][a]
            if not ns.on:
                continue
            held = ns.held[0] * lmax + ns.held[1]
            with np.errstate(invalid='ignore'):
                close = (np.abs(sinr[x] - sens[None, :]) <= THRESHOLD_DB) | ((fl > NEG)[None, :] & (np.abs(sinr[x] - fl[None, :]) <= THRESHOLD_DB))
            w = rb[x][None, :] == np.arange(c.r)[:, None]
            w[:, i] = True
            involved = np.repeat(w, lmax, axis=0)                        # [R Lmax, N]: group(r) u {i}
            k = c.r * lmax
            mark = ((close[:k] | close[held][None, :] | close[k][None, :]) & involved).any(axis=1)
            mark |= (close[held] & w[ns.held[0]]).any() | (close[k] & w[ns.held[0]]).any()       # D(c,p) enters every entry
            near[x, a] = mark.reshape(c.r, lmax)
            tot = sequential_sum(cap[x], axis=1)
            delta[x, a] = (tot[:k] - tot[held]).reshape(c.r, lmax)
            total[x] = tot[held]
    res.near, res.delta, res.total = near, delta, total
    return res


@lru_cache(maxsize=None)
def oracle_side(name, floors='none'):
    """by_oracle of a case on its oracle envs and links under a floor setting, computed once."""
    c = make_case(name)
    envs, links = oracle_links(name)
    return by_oracle(c, envs, links, None, FLOOR_SETTINGS[floors])

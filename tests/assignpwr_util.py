"""What the joint RB and power matching tests share (test_assignpwr_cpu.py, test_gpu_assignpwr.py): the float64 reference of the
per-level planes - own, harm, admissibility under SINR floors and the near-threshold marks - on read_side_util's received powers,
stated the way assign_util.weights_ref states one level; brute force over placements x powers through evaluate_util.evaluate_ref;
and the seeded cases, alphabets and floor settings of the direct launches of csrc/d2d_assignpwr.hip."""
import itertools
from functools import lru_cache

import numpy as np

import assign_util as asu
import evaluate_util as evu
import read_side_util as rsu

BAR, THRESHOLD_DB, THRESHOLD_CAP, B = asu.BAR, asu.THRESHOLD_DB, asu.THRESHOLD_CAP, asu.B
NO_POWER = -32768
MAX_LEVELS, CHUNK = 64, 8

# (cues, due pairs, RBs, law) -> (p_min, p_max) of every link in the bit-for-bit test: 1, 7, 8, 9, 21 and 47 levels, one below, one
# at and one past the chunk of 8, p_min != 0 and negative.  The movable links are the DUE links.
EXACT_CASES = {
    (1, 2, 4, 'ld35'): (5, 5),
    (13, 50, 64, 'mixed'): (-3, 3),
    (57, 200, 259, 'ld35'): (0, 8),
    (100, 200, 1, 'ld2'): (0, 20),
    (60, 200, 4000, 'mixed'): (2, 9),
    (300, 700, 8, 'mixed'): (-10, 36),
}
SCATTERED = asu.SCATTERED
SCATTERED_BOUNDS = {'cue': (0, 23), 'due': (-5, 12)}        # the scattered movable set: CUE and DUE ranges differ (24 and 18 levels)
# the floor comparison: levels 0 .. 20 throughout
FLOOR_CASES = ((1, 2, 4, 'ld35'), (13, 50, 64, 'mixed'), (57, 200, 259, 'ld35'), (100, 200, 1, 'ld2'), (60, 200, 4000, 'mixed'),
               (300, 700, 8, 'mixed'))
# the movable links of a floor case: every DUE link, or every STRIDE-th of them where the float64 planes [B, M, R, P] of all of them
# would take half a gigabyte - the other DUE links then stay in the background, on the RBs the case gives them
FLOOR_STRIDE = {(60, 200, 4000, 'mixed'): 8}
FLOOR_LEVELS = (0, 20)
FLOOR_SETTINGS = ((5.0, 0.0), (15.0, 10.0))                 # (cue, due) dB
# the small cases of the optimality proof against brute force
SMALL_CASES = ((2, 3, 3, 'ld35'), (3, 2, 3, 'ld2'), (2, 3, 4, 'mixed'))
SMALL_FLOORS = (None, (5.0, 0.0), (10.0, 5.0), (0.0, 10.0))
SMALL_LEVELS = (0, 4, 8, 12, 16, 20)


def lds_bytes(n, r, power_law):
    """The dynamic LDS a launch asks for, by the layout written in csrc/d2d_assignpwr.hip."""
    r16 = lambda x: (x + 15) & ~15
    n4 = (n + 3) & ~3
    return 16 * n + (r16(8 * n) if power_law else 0) + 32 * n + r16(8 * n4) + 3 * r16(4 * n) + r16(4 * (r + 1))


def class_floors(c, cues, pair):
    """float64 [N]: pair = (cue, due) dB by link class; None: no floors (-inf)."""
    if pair is None:
        return np.full(c['n'], -np.inf)
    return np.r_[np.full(cues, float(pair[0])), np.full(c['n'] - cues, float(pair[1]))]


def uniform_bounds(c, lo, hi):
    return np.full(c['n'], lo, dtype=np.int32), np.full(c['n'], hi, dtype=np.int32)


def scattered_bounds(c, cues=13):
    lo = np.r_[np.full(cues, SCATTERED_BOUNDS['cue'][0]), np.full(c['n'] - cues, SCATTERED_BOUNDS['due'][0])].astype(np.int32)
    hi = np.r_[np.full(cues, SCATTERED_BOUNDS['cue'][1]), np.full(c['n'] - cues, SCATTERED_BOUNDS['due'][1])].astype(np.int32)
    return lo, hi


# ------------------------------------------------------------------------------------------ the per-level planes, float64
def level_ref(c, links, power, floor, pl=None):
    """One level: (own, harm, admissible, near) [B, M, R], float64 / float64 / bool / bool, with movable link links[a] at power[a]
    dBm.  own, harm and the sensitivity part of near are assign_util.weights_ref's on the case whose power plane holds `power` for
    the movable links - the same expressions in the same order.  floor: float64 [N], -inf: none for that link.  (a, r) is admissible
    iff link a's SINR there is >= floor[a] and no background member k of r with background-only SINR >= floor[k] has SINR < floor[k]
    with a present.  near: the SINR of link a on r, or of any member of r with a present, lies within THRESHOLD_DB of its sensitivity
    or of its floor - or a member's background-only SINR lies that close to its floor (whether it constrains is then undecided)."""
    pwr = np.array(c['pwr'])
    pwr[:, np.asarray(links)] = np.asarray(power)[None, :]
    c = dict(c, pwr=pwr)
    pl = rsu.pair_pl_db(c) if pl is None else pl
    mw, _ = rsu._received_mw(c, pl)                                       # [b, j, i], zero diagonal
    sig, noise_dbm = rsu.signal_dbm(c, pl)
    b, n, r = c['b'], c['n'], c['r']
    tx, rx = np.asarray(c['tx']), np.asarray(c['rx'])
    noise = 10.0 ** (noise_dbm / 10.0)
    bw_mhz, sens = 1e-6 * c['ocols'].bw_hz[tx], c['ocols'].sens_dbm[rx]
    rb = np.asarray(c['rb'], dtype=np.int64)
    links = np.asarray(links, dtype=np.int64)
    floor = np.asarray(floor, dtype=np.float64)
    has = np.isfinite(floor)
    movable = np.zeros(n, bool)
    movable[links] = True
    m = len(links)

    def cap_of(sinr_db, who):
        return np.where(sinr_db > sens[who], bw_mhz[who] * np.log2(1.0 + 10.0 ** (sinr_db / 10.0)), 0.0)

    def close(sinr_db, level):
        with np.errstate(invalid='ignore'):
            return np.abs(sinr_db - level) <= THRESHOLD_DB               # an infinite level is close to nothing
    own, harm = np.zeros((b, m, r)), np.zeros((b, m, r))
    adm, near = np.ones((b, m, r), bool), np.zeros((b, m, r), bool)
    for e in range(b):
        bg = np.nonzero(~movable & (rb[e] >= 0) & (rb[e] < r))[0]        # the background links on an RB
        member = np.zeros((r, len(bg)))
        member[rb[e, bg], np.arange(len(bg))] = 1.0                        # [r, k]
        ix_own = (member @ mw[e][np.ix_(bg, links)]).T                     # [a, r]
        s_own = sig[e, links][:, None] - 10.0 * np.log10(ix_own + noise[links][:, None])
        own[e] = cap_of(s_own, links[:, None])
        near[e] = close(s_own, sens[links][:, None]) | close(s_own, floor[links][:, None])
        adm[e] = ~has[links][:, None] | (s_own >= floor[links][:, None])
        if not len(bg):
            continue
        same = rb[e, bg][:, None] == rb[e, bg][None, :]
        ix_bg = (mw[e][np.ix_(bg, bg)] * same).sum(axis=0)                 # [k]; the diagonal of mw is 0
        s_without = sig[e, bg] - 10.0 * np.log10(ix_bg + noise[bg])
        s_with = sig[e, bg][None, :] - 10.0 * np.log10(ix_bg[None, :] + mw[e][np.ix_(links, bg)] + noise[bg][None, :])   # [a, k]
        loss = cap_of(s_without, bg)[None, :] - cap_of(s_with, bg[None, :])
        harm[e] = loss @ member.T
        bound = has[bg] & (s_without >= floor[bg])                         # [k]: the background alone keeps its floor
        broken = bound[None, :] & (s_with < floor[bg][None, :])
        adm[e] &= ~((broken.astype(np.float64) @ member.T) > 0)
        undecided = close(s_with, sens[bg][None, :]) | close(s_with, floor[bg][None, :]) | close(s_without, floor[bg])[None, :]
        near[e] |= (undecided.astype(np.float64) @ member.T) > 0
    return own, harm, adm, near


def weights_power_ref(c, links, p_min, p_max, floor=None, floors=None):
    """The per-level planes of a case: (w float64 [B, M, R, P], valid bool [M, P], [(admissible, near) bool [B, M, R, P] per floor
    setting]).  Level l of movable link a is the power p_min[links[a]] + l, valid while <= p_max[links[a]]; P is the longest
    alphabet.  w = own - harm.  floors: a list of float64 [N] settings (floor: one of them; the list is then of length 1)."""
    settings = [floor if floor is not None else np.full(c['n'], -np.inf)] if floors is None else list(floors)
    links = np.asarray(links, dtype=np.int64)
    lo, hi = np.asarray(p_min, dtype=np.int64)[links], np.asarray(p_max, dtype=np.int64)[links]
    levels = int((hi - lo).max()) + 1
    pl = rsu.pair_pl_db(c)
    shape = (c['b'], len(links), c['r'], levels)
    w = np.zeros(shape)
    valid = (lo[:, None] + np.arange(levels)[None, :]) <= hi[:, None]
    marks = [(np.zeros(shape, bool), np.zeros(shape, bool)) for _ in settings]
    for l in range(levels):
        power = np.minimum(lo + l, hi)
        for q, f in enumerate(settings):
            own, harm, adm, near = level_ref(c, links, power, f, pl)
            marks[q][0][..., l], marks[q][1][..., l] = adm & valid[None, :, None, l], near & valid[None, :, None, l]
        w[..., l] = own - harm
    return w, valid, marks


def best_power(w, valid, adm):
    """(weights float64 [B, M, R], level int [B, M, R]; -inf / -1 where no level is admissible): the maximum of w over the admissible
    levels, equal values to the lowest."""
    masked = np.where(adm & valid[None, :, None, :], w, -np.inf)
    level = masked.argmax(axis=3)
    best = np.take_along_axis(masked, level[..., None], axis=3)[..., 0]
    return best, np.where(np.isfinite(best), level, -1)


def floor_links(c, cues, dues, r, law):
    return asu.due_links(c, cues)[::FLOOR_STRIDE.get((cues, dues, r, law), 1)]


@lru_cache(maxsize=2)
def floor_case_ref(cues, dues, r, law):
    """weights_power_ref of a FLOOR_CASES entry, floor_links() movable, levels FLOOR_LEVELS, under no floors and every FLOOR_SETTINGS
    entry: (w, valid, [(adm, near)] in the order (None, *FLOOR_SETTINGS)).  Computed once and left unchanged."""
    c = asu.case(cues, dues, r, law)
    lo, hi = uniform_bounds(c, *FLOOR_LEVELS)
    settings = [class_floors(c, cues, pair) for pair in (None,) + FLOOR_SETTINGS]
    return weights_power_ref(c, floor_links(c, cues, dues, r, law), lo, hi, floors=settings)


@lru_cache(maxsize=1)
def scattered_floor_ref():
    """The SCATTERED movable set (CUE and DUE links, alphabets of 24 and 18 levels) under every FLOOR_SETTINGS entry:
    (w, valid, [(adm, near)] in the order (None, *FLOOR_SETTINGS)).  `allowed` plays no part in the reference."""
    c = asu.case(*SCATTERED)
    links, _ = asu.scattered_movable(c)
    lo, hi = scattered_bounds(c)
    settings = [class_floors(c, 13, pair) for pair in (None,) + FLOOR_SETTINGS]
    return weights_power_ref(c, links, lo, hi, floors=settings)


# ------------------------------------------------------------------------------------------ brute force on complete assignments
def brute_force(c, links, powers, floor):
    """The largest total capacity (Mbps, float64, per env) over every one-to-one placement of the movable links x every choice of
    one power of `powers` per movable link that keeps the floors, minus the background's capacity - None for an env where nothing
    does.  Everything is judged on the COMPLETE assignment by evaluate_util.evaluate_ref: a movable link needs sinr_db >= its
    floor; a background link whose sinr_db in the background-only assignment is >= its floor must keep it."""
    links = np.asarray(links)
    m, r, n, b = len(links), c['r'], c['n'], c['b']
    floor = np.asarray(floor, dtype=np.float64)
    cand_rb, cand_pw = [asu.background_candidate(c, links)], [np.array(c['pwr'], dtype=np.int32)]
    for cols in itertools.permutations(range(r), m):
        for pw in itertools.product(powers, repeat=m):
            cand_rb.append(asu.placement_candidate(c, links, np.asarray(cols)))
            p = np.array(c['pwr'], dtype=np.int32)
            p[:, links] = np.asarray(pw)
            cand_pw.append(p)
    rb, pwr = np.stack(cand_rb, axis=1), np.stack(cand_pw, axis=1)
    sinr, cap, total = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rb, pwr, c, r)
    is_bg = np.ones(n, bool)
    is_bg[links] = False
    on = (rb[:, 0] >= 0) & (rb[:, 0] < r)                                 # [b, n]: the background links on an RB
    with np.errstate(invalid='ignore'):
        bound = is_bg[None, :] & on & np.isfinite(floor)[None, :] & (sinr[:, 0] >= floor[None, :])
        kept = ~bound[:, None, :] | (sinr >= floor[None, None, :])
        own_ok = ~np.isfinite(floor)[None, None, links] | (sinr[:, :, links] >= floor[None, None, links])
    feasible = kept.all(axis=2) & own_ok.all(axis=2)
    background = cap[:, 0][:, is_bg].sum(axis=1)
    out = []
    for e in range(b):
        ok = feasible[e, 1:]
        out.append(float(total[e, 1:][ok].max() - background[e]) if ok.any() else None)
    return out

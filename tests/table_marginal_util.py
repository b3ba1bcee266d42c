"""What the table difference-reward tests share (test_table_marginal_cpu.py, test_gpu_table_marginal.py): the case table of the
direct launches of csrc/d2d_tabmarg.hip, the float64 reference on them, the planted cases and the LDS layout restated.

The data is table_evaluate_util's: make_case with K = 1 draws the table (every entry on its own: not symmetric, so a transposed or
mis-pitched index shows), the planes (some links at rb -1 and R) and the columns.  The reference, marginal_ref, is the direct
leave-one-out: every link's capacity from the statement's formulas, then for every link i the capacities of its RB's other members
with row i of the same-RB interference taken out, all in float64 on 'pl' (what the kernel reads, as float64)."""
from functools import lru_cache

import numpy as np

import table_evaluate_util as teu

BAR = teu.BAR                                # the project's bar: |d| <= BAR max(|ref|, 1) on harm_mbps and difference_mbps (Mbps)
THRESHOLD_DB, THRESHOLD_CAP = teu.THRESHOLD_DB, teu.THRESHOLD_CAP
THREADS = 256                                # csrc/d2d_tabmarg.hip: TM_THREADS

# (links, RBs, envs, entry type, rows per env beyond N): the path it forces.  Both entry widths; the table as [B, N, N] (0) and in
# the live layout [B, N+1, N] (1), whose last row is NaN: never read
CASES = (
    (1, 1, 1, 'float64', 0),                 # no interferer
    (3, 1, 5, 'float32', 1),                 # all links share the one RB
    (50, 6, 5, 'float64', 1),                # one wave, not full
    (130, 70, 5, 'float32', 1),              # three waves, the last with two lanes; mostly small groups
    (300, 2, 1, 'float64', 0),               # groups of about 150 and more links than threads: the second pass of the loops
    (300, 2, 5, 'float32', 1),
)
LEFT_OUT = (0, 0, 0, 0, 0, 0)                # undecided links per case, of 1, 15, 250, 650, 300 and 1500: a reference run on the draws
PLANT = (50, 6, 5, 'float64', 1)             # the case the planted entries go into
PLANT_ENV, PLANT_RB = 1, 5


def lds_bytes(n, r):
    """The dynamic LDS a launch asks for, by the layout written in csrc/d2d_tabmarg.hip: v1 float4[N] | txl float2[N] | acc
    double[N rounded up to 4] | noise float[N] | cap float[N] | srb int[N] | start int[R + 1] | wdom u32[4], each rounded up to 16."""
    r16 = lambda x: (x + 15) & ~15
    n4 = (n + 3) & ~3
    return 16 * n + r16(8 * n) + 8 * n4 + 3 * r16(4 * n) + r16(4 * (r + 1)) + 16


@lru_cache(maxsize=None)
def make_case(n, r, b, dtype, extra):
    """The seeded case of a CASES entry: table_evaluate_util.make_case with one candidate, rb and pwr as [B, N]."""
    base = teu.make_case(n, r, 1, b, dtype, extra)
    c = dict(base, rb=np.ascontiguousarray(base['rb'][:, 0]), pwr=np.ascontiguousarray(base['pwr'][:, 0]))
    del c['k']
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def link_budget(c):
    """(eirp_off_db [N] at the transmitters, rx_off_db, noise_mw, sens_db [N] at the receivers, bw_mhz [N] at the transmitters)."""
    o, tx, rx = c['ocols'], np.asarray(c['tx']), np.asarray(c['rx'])
    return o.eirp_off_db[tx], o.rx_off_db[rx], 10.0 ** (o.noise_dbm[rx] / 10.0), o.sens_dbm[rx], 1e-6 * o.bw_hz[tx]


def marginal_ref(c, rb=None, pwr=None, pl=None):
    """The float64 leave-one-out on the case's table (or pl) for its planes (or rb / pwr, [B, N]): a dict of
    harm, difference, capacity, sinr_db [B, N]; decided bool [B, N] - False where the link's own reference SINR, or a same-RB
    victim's with or without the link, lies within THRESHOLD_DB of the sensitivity; lifted int [B, N] - the victims whose capacity
    is 0 with the link and positive without it."""
    rb = np.asarray(c['rb'] if rb is None else rb, dtype=np.int64)
    pwr = np.asarray(c['pwr'] if pwr is None else pwr, dtype=np.int64)
    pl = np.asarray(c['pl'] if pl is None else pl, dtype=np.float64)
    b, n = rb.shape
    r = c['r']
    eirp_off, rx_off, noise, sens, bw_mhz = link_budget(c)
    idx = np.arange(n)
    out = {k: np.zeros((b, n)) for k in ('harm', 'difference', 'capacity', 'sinr_db')}
    out['decided'], out['lifted'] = np.ones((b, n), dtype=bool), np.zeros((b, n), dtype=np.int64)

    def planes(sig_db, ix):
        s = sig_db - 10.0 * np.log10(ix + noise)
        return s, np.where(s > sens, bw_mhz * np.log2(1.0 + 10.0 ** (s / 10.0)), 0.0)

    with np.errstate(all='ignore'):
        for e in range(b):
            eirp = pwr[e] + eirp_off                                                         # [j]
            on = (rb[e] >= 0) & (rb[e] < r)
            same = (rb[e][:, None] == rb[e][None, :]) & on[:, None] & on[None, :]
            same[idx, idx] = False
            ms = np.where(same, 10.0 ** ((eirp[:, None] - pl[e]) / 10.0), 0.0)               # [j, i]: what j puts into i's receiver
            sig_db = eirp - pl[e][idx, idx] + rx_off
            s_with, cap = planes(sig_db, ms.sum(axis=0))
            near = np.abs(s_with - sens) <= THRESHOLD_DB
            out['sinr_db'][e], out['capacity'][e] = s_with, cap
            for i in range(n):
                victims = same[i]
                if victims.any():
                    wo = ms.copy()
                    wo[i] = 0.0                                                              # link i off the air
                    s_wo, cap_wo = planes(sig_db, wo.sum(axis=0))
                    out['harm'][e, i] = (cap_wo - cap)[victims].sum()
                    out['lifted'][e, i] = int(((cap == 0.0) & (cap_wo > 0.0) & victims).sum())
                    if (near | (np.abs(s_wo - sens) <= THRESHOLD_DB))[victims].any():
                        out['decided'][e, i] = False
            out['decided'][e] &= ~near
    out['difference'] = out['capacity'] - out['harm']
    return out


@lru_cache(maxsize=None)
def case_ref(n, r, b, dtype, extra):
    """marginal_ref of a CASES entry, computed once and left unchanged."""
    out = marginal_ref(make_case(n, r, b, dtype, extra))
    for v in out.values():
        v.setflags(write=False)
    return out


def same_rb(rb, r):
    """bool [B, j, i]: links j != i of one env on one RB - the pairs whose entries [j, i] a launch reads."""
    rb = np.asarray(rb)
    on = (rb >= 0) & (rb < r)
    same = (rb[:, :, None] == rb[:, None, :]) & on[:, :, None] & on[:, None, :]
    same[:, np.arange(rb.shape[1]), np.arange(rb.shape[1])] = False
    return same


@lru_cache(maxsize=None)
def planted_lifted():
    """The PLANT case with one pair (p, q) alone on RB PLANT_RB of env PLANT_ENV and entry [p, q] set so that q lies 3 dB under its
    sensitivity with p on the air: (case, p, q).  Without p, q is alone: harm[p] is q's whole capacity, its SNR's."""
    c = make_case(*PLANT)
    e, r = PLANT_ENV, PLANT_RB
    rb, table = c['rb'].copy(), c['table'].copy()
    members = np.flatnonzero(rb[e] == r)
    rb[e, members] = 0                                                   # clear the RB, then seat the pair
    alive = [j for j in range(c['n']) if j != teu.DEAD_LINK]
    p, q = alive[5], alive[17]
    rb[e, [p, q]] = r
    eirp_off, rx_off, noise, sens, _ = link_budget(c)
    sig_db = c['pwr'][e, q] + eirp_off[q] - c['pl'][e, q, q] + rx_off[q]
    assert sig_db - 10.0 * np.log10(noise[q]) > sens[q] + 6.0            # q clears its threshold alone, with room
    ix = 10.0 ** ((sig_db - (sens[q] - 3.0)) / 10.0) - noise[q]          # the interference that puts q 3 dB under
    table[e, p, q] = c['pwr'][e, p] + eirp_off[p] - 10.0 * np.log10(ix)
    out = dict(c, rb=rb, table=table, pl=table[:, :c['n']].astype(np.float64))
    for v in (rb, table, out['pl']):
        v.setflags(write=False)
    return out, p, q

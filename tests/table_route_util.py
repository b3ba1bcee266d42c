"""The step kernel's path-loss table modes at every launch shape (test_table_route_cpu.py, test_gpu_table_route.py): the case table -
one row per `step_kernel<M, LPT, FULL, 0, OPT>` instantiation of launch_step, M in {PL_TABLE = 2, PL_TABLE_DB = 5} -, seeded synthetic
tables that are NOT made from positions, seeded actions with the envs in which a launch changes its path, and a float64 reference of
the step on a table by (tx link, rx link).

A table made from distances is symmetric, and a link table gathered from a device table holds one value for every CUE receiver column
of a row (all CUEs are received by device 0), so most index mistakes cannot show on it.  `pairs` draws every (env, j, i) on its own;
`devices` draws every (env, tx device, rx device) on its own and is NaN wherever no link reads it."""
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace
from typing import Optional

import numpy as np

from oracle import d2d_oracle as orc

THRESHOLD_DB = 1e-4          # evaluate_util's: a link whose reference SINR lies this close to its sensitivity may fall on either side
TOL = 1e-5                   # the project's bar: |d| <= TOL * max(|ref|, 1)
P_CUE, P_DUE = 24, 21        # power levels of the default config (0..23 dBm, 0..20 dBm): raw action = rb * P + pwr
LIST_SLOTS = 8               # csrc/d2d_step_device.h: links per RB a member list holds
N_FIXED = 5                  # the fixed-action case: CUE links 0..4 are driven by set_fixed_actions
# own-link entries: alive links U[40, 120) dB, dead links (below their sensitivity whatever the interference: SNR < -123.4 dB needs
# more than 276.3 dB on a CUE uplink, 223 dB on a sidelink) U[282, 298); every other entry U[60, 318).  10^-31.8 is a normal float32.
OWN_DB, DEAD_DB, OTHER_DB = (40.0, 120.0), (282.0, 298.0), (60.0, 318.0)
DEAD_CUES, DEAD_DUES = (7, 9), (2, 5, 9)            # link indices (DUEs counted from the first sidelink), the same in every env
OOR_CUE, OOR_DUE = 6, 1                             # the links of the out-of-range env: rb == R, and a negative raw action
OVERFLOW_DUES = range(10, 22)                       # the 12 sidelinks of the overflow env that all take RB 0
N_INF = 5                                           # +inf interferer entries per env: gain exactly 0, not flagged


@dataclass(frozen=True)
class Case:
    name: str
    b: int
    cues: int
    dues: int
    rbs: int
    kernel: str                      # with {m} for the mode
    geometry: tuple                  # (lpt, tpe, epw, mask_words, walk) of the plan
    path: str                        # the path the shape forces, in words
    tune: tuple = ()                 # ((key, value), ...): epw, lpt, threads - the planner's tune_<key>, the handle's TUNE_STEP_*
    walk: Optional[int] = None       # TUNE_STEP_WALK, None: auto (the test then also runs sim_util.search_variants)
    bucketing: bool = True
    reward: int = 1
    xpos: bool = False
    stepping: str = 'raw'            # 'raw' actions, 'planes' (rb= / pwr=), 'fixed' (a fixed-action CUE prefix + raw actions)
    lists: bool = False              # the launch walks member lists: env 1 overflows one
    routes: tuple = ('R1', 'R2', 'R3', 'R4')
    gpu: bool = True                 # False: planned only (d2d_create refuses more than D2D_MAX_LINKS = 2048 links)

    @property
    def n(self):
        return self.cues + self.dues

    @property
    def d(self):
        return 1 + self.cues + 2 * self.dues

    def plan_inputs(self, mode):
        words = [f'B={self.b} N={self.n} R={self.rbs} obs_mode=1 mode={mode} reward_fn={self.reward}']
        words += [f'tune_{k}={v}' for k, v in self.tune]
        if self.walk is not None:
            words.append(f'tune_walk={self.walk}')
        if not self.bucketing:
            words.append('bucketing=0')
        if self.xpos:
            words.append('xpos=1')
        if self.stepping == 'planes':
            words.append('action_mode=1')
        if self.stepping == 'fixed':
            words.append(f'n_fixed={N_FIXED}')
        return ' '.join(words)


def _cases():
    small = [
        Case('n50_masks', 7, 20, 30, 6, 'step_kernel<{m},1,false,0,0>', (1, 64, 4, 2, 0),
             '4 envs per workgroup, the last one holds 3; 2 mask words: the nested mask walk'),
        Case('n50_lists', 7, 20, 30, 16, 'step_kernel<{m},1,false,0,1>', (1, 64, 4, 2, 2),
             'member lists, 4 envs per workgroup; env 1 overflows a list: its workgroup falls back to the masks', walk=2, lists=True,
             stepping='fixed'),
        Case('n64_full', 3, 24, 40, 16, 'step_kernel<{m},1,true,0,0>', (1, 64, 1, 2, 0), 'one env per 64-thread workgroup, no predication',
             tune=(('epw', 1),)),
        Case('n64_full_lists', 3, 24, 40, 16, 'step_kernel<{m},1,true,0,1>', (1, 64, 1, 2, 2), 'the same on member lists; env 1 overflows',
             tune=(('epw', 1),), walk=2, lists=True),
        Case('n128_full_lpt2', 3, 48, 80, 32, 'step_kernel<{m},2,true,0,0>', (2, 64, 1, 4, 0), 'two links per thread, one env per workgroup',
             tune=(('epw', 1), ('lpt', 2))),
        Case('n128_full_lpt2_lists', 3, 48, 80, 32, 'step_kernel<{m},2,true,0,1>', (2, 64, 1, 4, 2), 'the same on member lists; env 1 overflows',
             tune=(('epw', 1), ('lpt', 2)), walk=2, lists=True),
        Case('n130_lpt2', 5, 50, 80, 40, 'step_kernel<{m},2,false,0,0>', (2, 128, 2, 5, 0),
             '128 threads per env, 2 envs per workgroup, 5 mask words; links 128 and 129 are second links of lanes 0 and 1',
             tune=(('lpt', 2),), stepping='planes'),
        Case('n130_lpt2_lists', 5, 50, 80, 40, 'step_kernel<{m},2,false,0,1>', (2, 128, 2, 5, 2), 'the same on member lists; env 1 overflows',
             tune=(('lpt', 2),), walk=2, lists=True),
        Case('n130_strided', 5, 50, 80, 40, 'step_kernel<{m},0,false,0,0>', (0, 64, 4, 0, 0),
             'strided links, 4 envs per workgroup, no masks: the all-pairs sweep', tune=(('threads', 64),)),
    ]
    twins = []
    for c in small:
        lpt, full, hot, opt = c.kernel[len('step_kernel<{m},'):-1].split(',')
        twins.append(Case(**{**c.__dict__, 'name': c.name + '_xpos', 'xpos': True,
                             'kernel': f'step_kernel<{{m}},{lpt},{full},{hot},{int(opt) + 16}>', 'path': c.path + '; float64 positions'}))
    large = [
        Case('n1100_sweep', 2, 300, 800, 4, 'step_kernel<{m},2,false,0,0>', (2, 576, 1, 0, 0),
             '576 threads, no masks past 1024 links: the sweep, about 275 links per RB', routes=('R2', 'R3f64', 'R4f32')),
        Case('n1100_lists', 2, 300, 800, 300, 'step_kernel<{m},2,false,0,1>', (2, 576, 1, 0, 2),
             'the auto walk takes the lists; env 1 overflows one and falls back to the sweep', lists=True, routes=('R2', 'R3f64', 'R4f32')),
        Case('n2100_strided', 2, 600, 1500, 600, 'step_kernel<{m},0,false,0,0>', (0, 1024, 1, 0, 0),
             'strided at 1024 threads; planned only: more links than d2d_create takes', gpu=False, routes=()),
        Case('n2048_strided', 2, 600, 1448, 600, 'step_kernel<{m},0,false,0,0>', (0, 512, 1, 0, 0),
             'strided at 512 threads, 4 links per thread: the largest strided env the library takes', tune=(('threads', 512),),
             routes=('R3f32shared', 'R4f32')),
    ]
    special = [
        Case('n50_reward3', 7, 20, 30, 16, 'step_kernel<{m},1,false,0,0>', (1, 64, 4, 2, 0),
             'CueSinrShannon asks for the lists and is refused: the mask walk', walk=2, reward=3),
        Case('n50_no_bucketing', 7, 20, 30, 6, 'step_kernel<{m},1,false,0,0>', (1, 64, 4, 0, 0),
             'no mask words: the sweep with the links in registers', bucketing=False),
    ]
    return small + twins + large + special


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
GPU_CASES = [c for c in CASES if c.gpu]
# the domain flags of the live table: LPT 1, 2 and 0, the walks of sim_util.search_variants where the case leaves them open, real lists
FLAG_CASES = ('n50_masks', 'n50_lists', 'n130_lpt2', 'n130_lpt2_lists', 'n130_strided')


def links(case):
    """(link_tx, link_rx, link_type): all CUE uplinks, then all DUE sidelinks - Simulator.default_link_keys()."""
    return orc_links(case.cues, case.dues)


def orc_links(cues, dues):
    tx = list(range(1, 1 + cues)) + [1 + cues + 2 * p for p in range(dues)]
    rx = [0] * cues + [2 + cues + 2 * p for p in range(dues)]
    ty = [orc.UPLINK] * cues + [orc.SIDELINK] * dues
    return np.array(tx), np.array(rx), np.array(ty)


def dead_links(case):
    return np.array(list(DEAD_CUES) + [case.cues + k for k in DEAD_DUES])


def special_envs(case):
    """(overflow env or None, out-of-range env): env 1 overflows a list in the list cases; the out-of-range env is env 2, or env 0
    where there are only two."""
    return (1 if case.lists else None), (2 if case.b >= 3 else 0)


def _seed(case, what):
    return [sum(map(ord, case.name)), case.n, case.rbs, what]


def actions(case):
    """rb, pwr [B, N] as the step decodes them, and what reaches the handle: raw [B, N - n_fixed] and the fixed links' (idx, rb, pwr).
    Even envs keep every dead CUE alone with other CUEs on RB R - 1 (no -1 under SystemCapacity); odd envs put dead CUE 7 on the RB of
    the first sidelink (-1 for the env).  Every other link takes a balanced random RB: at most ceil(N / (R - 1)) + 1 links per RB."""
    rng = np.random.default_rng(_seed(case, 1))
    b, n, r, c = case.b, case.n, case.rbs, case.cues
    levels = np.array([P_CUE] * c + [P_DUE] * case.dues)
    pwr = rng.integers(0, levels[None, :], (b, n))
    rb = np.empty((b, n), dtype=np.int64)
    dead_cues = np.array(DEAD_CUES)
    for e in range(b):
        rb[e] = rng.permutation(n) % (r - 1)
        if e % 2 == 0:
            alive_cues = np.setdiff1d(np.arange(c), dead_cues)
            rb[e, alive_cues[::7][:3]] = r - 1                  # three alive CUEs there too: RB R - 1 is a row like any other
            rb[e, dead_cues] = r - 1
        else:
            rb[e, dead_cues[0]] = rb[e, c]
    overflow, oor = special_envs(case)
    if overflow is not None:
        rb[overflow, [c + k for k in OVERFLOW_DUES]] = 0
    fixed = None
    if case.stepping == 'fixed':
        idx = np.arange(N_FIXED)
        fixed = (idx, idx % r, 3 + 4 * idx)
        rb[:, idx], pwr[:, idx] = fixed[1][None], fixed[2][None]
    raw = rb * levels[None] + pwr
    # the out-of-range env: rb == R on a CUE; a negative raw action on a sidelink, decoded with Python's floor (d2d_env.py:93-96)
    raw[oor, OOR_CUE] = r * P_CUE + 3
    raw[oor, c + OOR_DUE] = -4
    rb, pwr = orc.decode_actions(raw, levels[None])
    if fixed is not None:
        raw = raw[:, N_FIXED:]
    return SimpleNamespace(rb=rb, pwr=pwr, raw=raw.astype(np.int32), fixed=fixed, levels=levels)


def _draw(rng, shape, own_mask, dead_mask):
    """Independent dB values: own entries from the lower ranges, every other entry from OTHER_DB."""
    t = rng.uniform(*OTHER_DB, shape)
    own = rng.uniform(*OWN_DB, shape)
    dead = rng.uniform(*DEAD_DB, shape)
    t = np.where(own_mask, own, t)
    return np.where(dead_mask, dead, t)


def pairs(case, shared=False):
    """[B, N, N] (shared: [N, N]) float64 dB by (tx link j, rx link i), every entry drawn on its own; N_INF interferer entries per env
    are +inf."""
    rng = np.random.default_rng(_seed(case, 3 if shared else 2))
    n, envs = case.n, 1 if shared else case.b
    eye = np.eye(n, dtype=bool)
    dead = np.zeros(n, dtype=bool)
    dead[dead_links(case)] = True
    t = _draw(rng, (envs, n, n), eye[None], (eye & dead[None, :])[None])
    rb = actions(case).rb
    for e in range(envs):
        # pairs on one RB in this env (shared: in env 0), so that the step reads them; distinct transmitters
        j = rng.choice(n, N_INF, replace=False)
        for jj in j:
            mates = np.flatnonzero((rb[e] == rb[e, jj]) & (np.arange(n) != jj))
            t[e, jj, rng.choice(mates) if len(mates) else (jj + 1) % n] = np.inf
    return t[0] if shared else t


def snr_row(case):
    """[B, N] float64 dB: the SNR's own evaluation of every link's path (row N of the live table), drawn on its own."""
    return np.random.default_rng(_seed(case, 4)).uniform(*OWN_DB, (case.b, case.n))


def devices(case, shared=False):
    """[B, D, D] (shared: [D, D]) float64 dB by (tx device, rx device), every pair drawn on its own; NaN where no link reads it."""
    rng = np.random.default_rng(_seed(case, 6 if shared else 5))
    tx, rx, _ = links(case)
    d, envs = case.d, 1 if shared else case.b
    own = np.zeros((d, d), dtype=bool)
    own[tx, rx] = True
    dead = np.zeros((d, d), dtype=bool)
    k = dead_links(case)
    dead[tx[k], rx[k]] = True
    t = _draw(rng, (envs, d, d), own[None], dead[None])
    read = np.zeros((d, d), dtype=bool)
    read[np.ix_(tx, rx)] = True
    t = np.where(read[None], t, np.nan)
    return t[0] if shared else t


def gather(case, dev_table):
    """The link table a device table stands for: [..., N, N] by (tx link, rx link)."""
    tx, rx, _ = links(case)
    return np.ascontiguousarray(dev_table[..., tx[:, None], rx[None, :]])


def columns(case):
    return orc.device_columns(*orc.device_configs(case.cues, case.dues)[1:])


def positions(case):
    """[B, D, 2]: float32 numbers, or (xpos) float64 numbers that are not - the tables do not depend on them."""
    from sim_util import random_layout
    pos = random_layout(np.random.default_rng(_seed(case, 7)), case.b, case.cues, case.dues)
    if not case.xpos:
        return pos
    pos = pos.astype(np.float64) * (1.0 + 2.0 ** -30)
    pos[:, 0] = 0.0
    return pos


def table_step_ref(pl, snr_pl, rb, pwr, cols, link_tx, link_rx):
    """oracle.d2d_oracle.step's formulas (simulator.py:77-154) on a table by LINK pair: pl [B | 1, N, N] dB from the tx of link j to
    the rx of link i, snr_pl [B, N] the SNR's own evaluation of link i's path or None (then pl's diagonal), rb / pwr [B, N].
    float64 sinr_db, snr_db, rate_bps, capacity_mbps [B, N]."""
    pl = np.asarray(pl, dtype=np.float64)
    rb = np.asarray(rb); pwr = np.asarray(pwr, dtype=np.float64)
    b, n = rb.shape
    out = {k: np.empty((b, n)) for k in ('sinr_db', 'snr_db', 'rate_bps', 'capacity_mbps')}
    noise = cols.noise_dbm[link_rx]
    eye = np.eye(n, dtype=bool)
    for e in range(b):
        t = pl[e if pl.shape[0] > 1 else 0]
        eirp = pwr[e] + cols.eirp_off_db[link_tx]                                 # device.py:60
        sig = eirp - np.diagonal(t) + cols.rx_off_db[link_rx]                     # simulator.py:93
        sig_snr = sig if snr_pl is None else eirp - snr_pl[e] + cols.rx_off_db[link_rx]      # simulator.py:114
        same = (rb[e][:, None] == rb[e][None, :]) & ~eye                          # [j, i]: simulator.py:95
        with np.errstate(invalid='ignore'):
            ix_mw = np.where(same, orc.db_to_linear(eirp[:, None] - t), 0.0)      # simulator.py:97-101
        sinr = sig - orc.linear_to_db(ix_mw.sum(axis=0) + orc.db_to_linear(noise))            # simulator.py:106-107
        ok = sinr > cols.sens_dbm[link_rx]                                        # simulator.py:123,149
        shannon = np.log2(1 + orc.db_to_linear(sinr))
        out['sinr_db'][e] = sinr
        out['snr_db'][e] = sig_snr - noise                                        # simulator.py:115
        out['rate_bps'][e] = np.where(ok, shannon, 0.0)
        out['capacity_mbps'][e] = np.where(ok, 1e-6 * cols.bw_hz[link_tx] * shannon, 0.0)
    return out


REWARD_PARAM = {1: 0.0, 3: 0.0}          # SystemCapacity's min capacity; CueSinrShannon's SINR threshold in dB


def reference(case, pl, snr_pl=None):
    """table_step_ref on the case's actions, its reward from orc.reward_* as [B, N], and what lies too close to a threshold to
    compare: near [B, N] (rate, capacity), near_env [B] (the reward)."""
    a = actions(case)
    tx, rx, ty = links(case)
    cols = columns(case)
    pl = np.asarray(pl, dtype=np.float64)
    ref = table_step_ref(pl[None] if pl.ndim == 2 else pl, snr_pl, a.rb, a.pwr, cols, tx, rx)
    near = np.abs(ref['sinr_db'] - cols.sens_dbm[rx][None]) <= THRESHOLD_DB
    if case.reward == 1:
        reward = np.repeat(orc.reward_system_capacity(ref['capacity_mbps'], a.rb, ty, REWARD_PARAM[1])[:, None], case.n, 1)
        near_env = near.any(axis=1)
    else:
        reward = orc.reward_cue_sinr_shannon(ref['sinr_db'], a.rb, ty, REWARD_PARAM[3])
        near_env = (np.abs(ref['sinr_db'] - REWARD_PARAM[3]) <= THRESHOLD_DB).any(axis=1)
    ref.update(reward=reward, near=near, near_env=near_env, sens=cols.sens_dbm[rx])
    return ref


@lru_cache(maxsize=4)
def inputs(name):
    """The case's tables and references that more than one test reads, built once and left unchanged."""
    case = BY_NAME[name]
    out = SimpleNamespace(case=case, pairs=pairs(case), snr=snr_row(case))
    for v in (out.pairs, out.snr):
        v.setflags(write=False)
    out.ref_pairs = reference(case, out.pairs)                       # R2, R3: the SNR reads the diagonal
    return out


def rel_err(got, ref, keep=None):
    """max |got - ref| / max(|ref|, 1) over the entries `keep` selects."""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    err = np.where(np.isnan(err), np.inf, err)
    if keep is not None:
        err = err[keep]
    return float(err.max()) if err.size else 0.0

"""The rollout kernel's rare paths in each of its 48 instantiations (test_rollout_route_cpu.py, test_gpu_rollout_route.py): the case
table - one row per `rollout_kernel<MODE, OPT, LPT>` of launch_rollout and two more per mode with more RBs than pass 0 clears in its
two unrolled rounds -, the eight seeded and edited envs every row steps, a second batch with coincident devices, the float64
reference of each (oracle.d2d_oracle) and a float64 classification of every link into the arm of csrc/d2d_rollout.hip that sums
its interference.

The classification restates the kernel's thresholds from its comments and imports nothing from it: a link on an RB outside [0, R)
sweeps all pairs; up to eight links on an RB are summed in arrival order while the largest and the smallest of the lane's terms (its
own among them: the sum opens at minus the own term and adds all eight slots) lie within 2^25 of each other, and re-summed in sorted
order otherwise; from nine links on the row is full and the rest sits in the overflow pool, the own term is left out, the window is
53 - 24 - bits(members) bits (25 at 9 .. 15 members, 24 at 16 .. 31, 23 at 32 .. 63), and a lane outside it takes its terms by
selection up to 32 members and by the sweep beyond.  The kernel compares raw float bits and is conservative by less than a binade,
so a link witnesses an arm only if the ratio of its largest to its smallest term is a factor CLEARANCE = 4 away from the boundary."""
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from oracle import d2d_oracle as orc

THRESHOLD_DB = 1e-4          # evaluate_util's: a link whose reference SINR lies this close to a threshold may fall on either side
TOL = 1e-5                   # the project's bar: |d| <= TOL * max(|ref|, 1)
B = 8                        # envs per batch
N_FIXED = 40                 # the fixed-action rows: links 0 .. 39 (of 64 CUE links: a wave holds fixed and free links)
SLOTS = 8                    # links per RB the row of a member list holds
CLEARANCE = 4.0
MODELS = {0: ('inv2',), 4: ('ple35', 'ple30'), 1: ('hata',)}         # d2d::PlMode -> the path-loss models that make refresh_tables choose it
# why refresh_tables derives the mode: every exponent 2 -> PL_INV_SQUARE; one log-distance exponent 3.5 / 3.0 -> within 1/2 of k = 4 / 3
# -> PL_POWK with pow_k 4 (the copy without tests on k) / 3 (the general copy, odd: the v_rsq step); COST-Hata with the base
# station 60 m up and the CUE links as downlinks -> the transmitters' exponents are 3.325 (base station) and 4.375 (UEs at 1.5 m),
# further than 1/2 from 3 and from 4 respectively -> PL_POWER, while every class of 64 (128) links keeps one record
MIN_CAPACITY = 0.18 * float(np.log2(1.0 + 1e-5))     # SystemCapacity's min_capacity_mbps of every reward-1 row: 180 kHz at an SINR of -50 dB
ROLE_MARGIN_DB = 10.0        # CueSinrShannon's threshold of the twelve role steps lies this far below the eleven at 20 dBm, and 10.4 dB above the one at 0 dBm
ARMS = ('common', 're_sorted', 'pool_order_free', 'pool_selection', 'pool_sweep', 'oor_sweep')       # + 'divided', a decode arm

# the links the envs are built from (indices into the link list: CUE links 0 .. cues - 1, then the sidelinks; every one beyond the
# fixed prefix) and the RBs they crowd (beyond the fixed links' RBs 0 .. 39; R - 1 and R - 2: the last rows of the slot region)
FAR_CUE, VICTIM_DUE, NEAR_DUE = 41, 5, 9
ENV1_CUES, ENV2_CUES, ENV2_DUES = range(42, 51), range(42, 64), range(10, 25)
ENV4_DUES = range(20, 29)
CROWD_A, CROWD_B, CROWD_A_DUE = range(42, 53), range(53, 64), {5: 40, 6: 41}
ROLE_CUES = range(42, 54)
OOR_CUE, OOR_DUE, NEG_CUE = 45, 20, 50
ENV6_FIXED_LINK, ENV6_FIXED_FREE_CUES, ENV6_DUES = 7, range(54, 62), range(30, 40)


@dataclass(frozen=True)
class Row:
    name: str
    opt: int                         # OPT_SREC 2 | OPT_NT 4 | OPT_PAD 8 | OPT_XPOS 16
    lpt: int
    cues: int
    dues: int
    rbs: int = 64
    reward: int = 1                  # 1 SystemCapacity, 2 Shannon, 3 CueSinrShannon
    per_env: bool = False            # D2D_REWARD_PER_ENV
    fixed: bool = False              # a fixed-action prefix of N_FIXED CUE links (records then differ within the first group of 64)
    override: bool = False           # one sidelink transmitter with its own antenna gain: records differ within its group of 64
    obs: str = 'table'               # 'table' | 'none' | 'linear'
    export: bool = True              # the decoded (rb, pwr) planes
    xpos: bool = False               # a float64 layout with non-zero low parts
    tune: tuple = ()                 # ((key, value), ...): the planner's tune_<key>, the handle's TUNE_STEP_<TUNE_KEYS[key]>

    @property
    def n(self):
        return self.cues + self.dues

    @property
    def rec_uniform(self):
        """What refresh_tables derives: identical records within every aligned group of 64 links."""
        return int(self.n % 64 == 0 and not self.fixed and not self.override)

    @property
    def rec_uniform128(self):
        return int(self.rec_uniform and self.cues % 128 == 0 and self.n % 128 == 0)

    def kernel(self, mode):
        return f'rollout_kernel<{mode},{self.opt},{self.lpt}>'

    def threads(self):
        return -(-(-(-self.n // self.lpt)) // 64) * 64

    def plan_inputs(self, mode):
        words = [f'B={B} N={self.n} R={self.rbs} obs_mode={("none", "table", "linear").index(self.obs)} mode={mode} reward_fn={self.reward}',
                 f'rec_uniform={self.rec_uniform} rec_uniform128={self.rec_uniform128} xpos={int(self.xpos)}']
        if self.fixed:
            words.append(f'n_fixed={N_FIXED}')
        words += [f'tune_{k}={v}' for k, v in self.tune]
        return ' '.join(words)


TUNE_KEYS = {'srec': 'TUNE_STEP_SCALAR_RECORDS', 'nt': 'TUNE_STEP_NT_RESULTS', 'lpt': 'TUNE_STEP_LPT'}


def _rows():
    def t(**kw):
        return tuple(kw.items())
    return [
        # a multiple of 64 links, float32 positions
        Row('o0_l1', 0, 1, 64, 64, reward=3, tune=t(srec=0, nt=0)),
        Row('o2_l1', 2, 1, 64, 64, obs='none', export=False, tune=t(nt=0)),
        Row('o4_l1', 4, 1, 64, 64, reward=3, fixed=True),
        Row('o6_l1', 6, 1, 64, 64, reward=2),
        Row('o0_l2', 0, 2, 64, 64, per_env=True, export=False, tune=t(lpt=2, nt=0)),          # classes of 64: per-lane records
        Row('o4_l2', 4, 2, 64, 64, reward=2, obs='none', tune=t(lpt=2)),
        Row('o2_l2', 2, 2, 128, 128, obs='linear', tune=t(lpt=2, nt=0)),                      # classes of 128: one scalar load per wave
        Row('o6_l2', 6, 2, 128, 128, per_env=True, obs='none', export=False, tune=t(lpt=2)),  # the benchmark's learner configuration
        # padded: 62 shadow threads in the third wave
        Row('o8_l1', 8, 1, 64, 66, fixed=True, obs='linear', tune=t(nt=0)),
        Row('o12_l1', 12, 1, 64, 66, reward=3, export=False),
        # exact positions
        Row('o16_l1', 16, 1, 64, 64, fixed=True, xpos=True, tune=t(nt=0)),
        Row('o18_l1', 18, 1, 64, 64, reward=2, obs='none', xpos=True, tune=t(nt=0)),
        Row('o20_l1', 20, 1, 64, 64, reward=3, override=True, xpos=True),
        Row('o22_l1', 22, 1, 64, 64, per_env=True, obs='none', export=False, xpos=True),
        Row('o24_l1', 24, 1, 64, 66, reward=2, xpos=True, tune=t(nt=0)),
        Row('o28_l1', 28, 1, 64, 66, obs='none', xpos=True),
        # R + 1 + (R + 1) / 4 = 377 sixteen-byte units of slots and counters against 2 x 64 and 2 x 128 threads: further rounds of pass 0
        Row('r300_l2', 4, 2, 64, 64, rbs=300, tune=t(lpt=2)),
        Row('r300_l1', 6, 1, 64, 64, rbs=300),
    ]


ROWS = _rows()
BY_NAME = {r.name: r for r in ROWS}
CASES = [(r.name, model) for r in ROWS for models in MODELS.values() for model in models]


def pass0_rounds(row):
    """Rounds of pass 0: ceil((R + 1 + ceil((R + 1) / 4)) / threads); the first two are unrolled, the others the workgroup-uniform loop."""
    rows = row.rbs + 1
    return -(-(rows + (rows + 3) // 4) // row.threads())


# ---- the shape: links, devices, path loss
def links(row, model):
    """(link_tx, link_rx, link_type): the CUE links - uplinks, under 'hata' downlinks -, then the sidelinks."""
    c, p = row.cues, row.dues
    cue_dev = np.arange(1, 1 + c)
    due_tx = 1 + c + 2 * np.arange(p)
    if model == 'hata':
        tx, rx, ty = np.zeros(c, dtype=np.int64), cue_dev, [orc.DOWNLINK] * c
    else:
        tx, rx, ty = cue_dev, np.zeros(c, dtype=np.int64), [orc.UPLINK] * c
    return np.concatenate([tx, due_tx]), np.concatenate([rx, due_tx + 1]), np.array(ty + [orc.SIDELINK] * p)


def device_overrides(row, model):
    """The device_config_file of the row, parsed: {} for most."""
    out = {}
    if model == 'hata':
        out['mbs'] = {'position': [0.0, 0.0], 'config': {'antenna_height_m': 60.0}}
    if row.override:
        out['due06'] = {'config': {'tx_antenna_gain_dBi': 3.5}}                    # the transmitter of sidelink 3
    return out


def columns(row, model):
    _, cfgs, is_bs = orc.device_configs(row.cues, row.dues, overrides=device_overrides(row, model))
    return orc.device_columns(cfgs, is_bs)


def spec(model):
    if model == 'hata':
        return orc.PathLossSpec('cost_hata', 2.1, area='suburban')
    return orc.PathLossSpec('log_distance', 2.1, ple={'inv2': 2.0, 'ple35': 3.5, 'ple30': 3.0}[model])


def levels(row, model):
    return orc.pwr_levels_for(links(row, model)[2])


# ---- the envs
def _seed(row, model, what, attempt):
    return [sum(map(ord, row.name)), sum(map(ord, model)), what, attempt]


def _layout(rng, row):
    from sim_util import random_layout
    return random_layout(rng, B, row.cues, row.dues).astype(np.float64)


def _exact(row, pos):
    """float32 numbers, or (xpos) float64 numbers with non-zero low parts - the same layout scaled by 1 + 2^-30."""
    if not row.xpos:
        return pos.astype(np.float32)
    pos = pos.astype(np.float32).astype(np.float64) * (1.0 + 2.0 ** -30)
    pos[:, 0] = 0.0
    return pos


class _Edit:
    """The edits of one batch: raw [B, N] actions of all links and positions [B, D, 2]."""

    def __init__(self, row, model, rng):
        self.row, self.lv = row, levels(row, model)
        self.pos = _layout(rng, row)
        self.raw = rng.integers(0, row.rbs * self.lv[None, :], (B, row.n))
        self.fixed = None
        if row.fixed:
            idx = np.arange(N_FIXED)
            self.fixed = (idx, idx % row.rbs, 3 + idx % 20)
            self.raw[:, idx] = (self.fixed[1] * self.lv[idx] + self.fixed[2])[None]
        self.free = np.ones(row.n, dtype=bool)
        self.free[:N_FIXED if row.fixed else 0] = False

    def due(self, p):
        return self.row.cues + p

    def due_tx(self, p):
        return 1 + self.row.cues + 2 * p

    def due_rx(self, p):
        return 2 + self.row.cues + 2 * p

    def crowd(self, env, rb, members, pwr=10):
        """Every other free link off `rb`, then `members` onto it."""
        cur = self.raw[env] // self.lv
        move = (cur == rb) & self.free
        self.raw[env] = np.where(move, ((rb + 1) % self.row.rbs) * self.lv + self.raw[env] % self.lv, self.raw[env])
        for l in members:
            assert self.free[l], l
            self.raw[env, l] = rb * self.lv[l] + min(pwr, int(self.lv[l]) - 1)

    def power(self, env, link, pwr):
        self.raw[env, link] = self.raw[env, link] // self.lv[link] * self.lv[link] + pwr

    def near_far(self, env, rb):
        """The victim sidelink at the cell's western edge, the near sidelink's transmitter 0.3 m from the victim's receiver at 20 dBm,
        the far CUE link at 0 dBm: its transmitter 930 m away at the eastern edge, or (downlinks) the base station 450 m away."""
        v, q = VICTIM_DUE, NEAR_DUE
        self.pos[env, self.due_rx(v)] = (-450.0, 30.0)
        self.pos[env, self.due_tx(v)] = (-444.0, 38.0)
        self.pos[env, self.due_tx(q)] = (-449.7, 30.0)
        self.pos[env, self.due_rx(q)] = (-446.7, 34.0)
        self.pos[env, 1 + FAR_CUE] = (480.0, 3.0)
        self.raw[env, self.due(q)] = rb * self.lv[self.due(q)] + 20
        self.raw[env, FAR_CUE] = rb * self.lv[FAR_CUE] + 0

    def ring(self, env, devices, radius, phase=0.0):
        k = np.arange(len(devices))
        a = phase + 2 * np.pi * k / len(devices)
        self.pos[env, list(devices)] = np.stack([radius * np.cos(a), radius * np.sin(a)], axis=1)


def _main_batch(row, model, attempt):
    ed = _Edit(row, model, np.random.default_rng(_seed(row, model, 1, attempt)))
    r, c = row.rbs, row.cues
    trio = [ed.due(VICTIM_DUE), ed.due(NEAR_DUE), FAR_CUE]
    # env 0: three on one RB, the near / far pair -> re-sorted
    ed.crowd(0, 47, trio); ed.near_far(0, 47)
    # env 1: twelve on RB R - 1 with the pair -> pool, selection
    ed.crowd(1, r - 1, trio + list(ENV1_CUES)); ed.near_far(1, r - 1)
    # env 2: forty on one RB with the pair -> pool, sweep
    ed.crowd(2, 44, trio + list(ENV2_CUES) + [ed.due(p) for p in ENV2_DUES]); ed.near_far(2, 44)
    # env 3: two links on the same out-of-range RB (rb == R: they interfere with each other, d2d_env.py:94-96), a negative action.
    # With two links per thread the partners of OOR_CUE (odd) and of the sidelink (even) are ordinary links of the same thread.
    ed.raw[3, OOR_CUE] = r * ed.lv[OOR_CUE] + 5
    ed.raw[3, ed.due(OOR_DUE)] = r * ed.lv[ed.due(OOR_DUE)] + 5
    ed.raw[3, NEG_CUE] = -7
    # env 4: nine sidelinks on RB R - 2, their transmitters on a ring of 200 m (neighbours 137 m apart, the farthest 394 m), all at
    # 10 dBm: the pool, every term well inside the window.  And the crowd without a sidelink (below), in an env at the mean.
    ed.crowd(4, r - 2, [ed.due(p) for p in ENV4_DUES])
    ed.ring(4, [ed.due_tx(p) for p in ENV4_DUES], 200.0, 0.05)
    for p in ENV4_DUES:
        ed.pos[4, ed.due_rx(p)] = ed.pos[4, ed.due_tx(p)] + (6.0, 8.0)
    # env 5: the reward's second look.  A CROWD: eleven CUE links at their top level (23 dBm; downlinks 46 dBm) but one at 0 dBm.
    # Uplinks: the strong ten 5 m from the base station, the weak one 480 m away (-23 - 10 - 39.6 dB and the receiver's 17.5 dBi,
    # which the signal alone gets: -55 dB under 1 / d^2, less under the steeper laws); downlinks: all from the base station
    # (-56 dB).  The weak link's capacity is below MIN_CAPACITY (-50 dB).
    top = int(ed.lv[0]) - 1

    def crowd(env, rb, cues, extra=()):
        ed.crowd(env, rb, list(cues) + list(extra), pwr=top)
        ed.power(env, cues[0], 0)
        ed.ring(env, [1 + k for k in cues], 5.0, 0.1 + 0.2 * (rb == 53))
        ed.pos[env, 1 + cues[0]] = (-480.0, -20.0) if rb == 51 else (-20.0, 480.0)
    # env 4 holds a crowd without a sidelink on RB 53: a second overflowing RB in one env (the pool holds two RBs' entries), and
    # under SystemCapacity no -1 from it - env 4 stays at the mean
    crowd(4, 53, CROWD_B)
    if row.reward == 3:
        # twelve CUE links on one RB at 20 dBm, their devices on a ring of 300 m: equal gains, so SINR = P_i / sum P_j.  A role step
        # (inputs().roles) takes one of them to 0 dBm
        ed.crowd(5, 51, list(ROLE_CUES), pwr=20)
        ed.ring(5, [1 + k for k in ROLE_CUES], 300.0, 0.1)
    else:
        # env 5: a crowd with exactly one sidelink on RB 51, and the crowd without one on RB 53; env 6: the first again, so that
        # two envs end at -1 - with an odd sidelink, which two links per thread enter into the list behind the eleven (a thread's
        # second links follow all first links of its wave), so that the sidelink sits in the pool
        crowd(5, 51, CROWD_A, [ed.due(CROWD_A_DUE[5])])
        crowd(5, 53, CROWD_B)
        crowd(6, 51, CROWD_A, [ed.due(CROWD_A_DUE[6])])
    # env 6: the row's edge links
    if row.n % 64:                   # the shadowed link N - 1 and link N - 2 on a crowded RB with a pool
        ed.crowd(6, 55, [row.n - 1, row.n - 2] + [ed.due(p) for p in ENV6_DUES][:8])
    elif row.lpt == 2:               # the two links of one thread on the same crowded RB
        ed.crowd(6, 55, [ed.due(p) for p in ENV6_DUES])
    if row.fixed:                    # a fixed link among the crowd: the free links come to its RB
        ed.crowd(6, ENV6_FIXED_LINK % r, list(ENV6_FIXED_FREE_CUES) + [ed.due(p) for p in ENV6_DUES][8:])
    # env 7: untouched
    return ed


def _zero_batch(row, model, attempt):
    """Coincident devices: env 0 a sidelink whose receiver sits on its transmitter, alone on its RB; env 1 the same with company;
    env 2 a sidelink's transmitter on another sidelink's receiver, both on one RB; envs 3 .. 7 untouched."""
    ed = _Edit(row, model, np.random.default_rng(_seed(row, model, 2, attempt)))
    for env in (0, 1):
        ed.pos[env, ed.due_rx(7)] = ed.pos[env, ed.due_tx(7)]
    ed.crowd(0, 45, [ed.due(7)])
    ed.crowd(1, 45, [ed.due(7), ed.due(30), 44])
    ed.pos[2, ed.due_tx(11)] = ed.pos[2, ed.due_rx(3)]
    ed.crowd(2, 49, [ed.due(3), ed.due(11)])
    return ed


ZERO_LINKS = ((0, 7), (1, 7), (2, 3))            # (env, sidelink) whose SINR is not finite


# ---- the reference
def reference(row, model, pos, raw, param):
    """orc.step on the decoded actions and the row's reward: float64 sinr_db, snr_db, rate_bps, capacity_mbps [B, N], rb, pwr,
    reward ([B] under SystemCapacity, else [B, N])."""
    tx, rx, ty = links(row, model)
    cols = columns(row, model)
    rb, pwr = orc.decode_actions(raw, levels(row, model)[None, :])
    ref = orc.step(np.asarray(pos, dtype=np.float64), tx, rx, rb, pwr, cols, spec(model), chunk=B)
    ref.update(rb=rb, pwr=pwr, sens=cols.sens_dbm[rx])
    if row.reward == 1:
        ref['reward'] = orc.reward_system_capacity(ref['capacity_mbps'], rb, ty, param)
    elif row.reward == 2:
        ref['reward'] = orc.reward_shannon(ref['sinr_db'], param)
    else:
        ref['reward'] = orc.reward_cue_sinr_shannon(ref['sinr_db'], rb, ty, param)
    return ref


def capacity_threshold_db(row, model, min_capacity):
    """[N]: the SINR at which a link's capacity equals min_capacity (simulator.py:150-151)."""
    tx = links(row, model)[0]
    bw_mhz = 1e-6 * columns(row, model).bw_hz[tx]
    return orc.linear_to_db(2.0 ** (min_capacity / bw_mhz) - 1.0)


def reward_param(row, ref_sinr, ty):
    """The reward's parameter, from the reference alone (the SINRs do not depend on it): SystemCapacity MIN_CAPACITY; Shannon the 30th
    percentile of all SINRs and CueSinrShannon the median of the non-D2D links', rounded to a dB and moved off it by 0.37 dB."""
    if row.reward == 1:
        return MIN_CAPACITY
    if row.reward == 2:
        return float(np.round(np.percentile(ref_sinr, 30.0))) + 0.37
    return float(np.round(np.median(ref_sinr[:, ty != orc.SIDELINK]))) + 0.37


def near(row, model, ref, param):
    """How many links of the reference lie within THRESHOLD_DB of a threshold that decides an output."""
    ty = links(row, model)[2]
    count = int((np.abs(ref['sinr_db'] - ref['sens'][None]) <= THRESHOLD_DB).sum())
    if row.reward == 1:
        thr = capacity_threshold_db(row, model, param)
        count += int((np.abs(ref['sinr_db'] - thr[None]) <= THRESHOLD_DB)[:, ty != orc.SIDELINK].sum())
    else:
        count += int((np.abs(ref['sinr_db'] - param) <= THRESHOLD_DB).sum())
    return count


def _role_raw(row, model, raw, k):
    """The raw actions of role step k: member k of env 5's twelve at 0 dBm, the others as they are (20 dBm)."""
    lv = levels(row, model)
    out = raw.copy()
    l = ROLE_CUES[k]
    out[5, l] = out[5, l] // lv[l] * lv[l]
    return out


@lru_cache(maxsize=None)
def inputs(name, model):
    """Everything a test reads of a case, built once and left unchanged: re-seeded until no link of any step lies within THRESHOLD_DB
    of a threshold (`attempt` says how often), so that the GPU comparison leaves nothing out."""
    row = BY_NAME[name]
    tx, rx, ty = links(row, model)
    for attempt in range(32):
        ed = _main_batch(row, model, attempt)
        pos = _exact(row, ed.pos)
        ref0 = reference(row, model, pos, ed.raw, 0.0)
        param = reward_param(row, ref0['sinr_db'], ty)
        ref = reference(row, model, pos, ed.raw, param)
        roles = []
        if row.reward == 3:
            # the twelve sit on a ring: equal gains, so the eleven share one SINR (the main step's, within 0.04 dB) and the low member
            # lies 20.4 dB below it, whatever the path-loss law and the receiver's gain and noise
            role_param = float(np.round(np.median(ref['sinr_db'][5, list(ROLE_CUES)]))) - ROLE_MARGIN_DB + 0.37
            for k in range(len(ROLE_CUES)):
                raw_k = _role_raw(row, model, ed.raw, k)
                roles.append(SimpleNamespace(raw=raw_k, param=role_param, ref=reference(row, model, pos, raw_k, role_param)))
        if near(row, model, ref, param) + sum(near(row, model, s.ref, s.param) for s in roles) == 0:
            break
    else:
        raise AssertionError(f'{name} {model}: no seed keeps every link {THRESHOLD_DB} dB off the thresholds')
    zed = _zero_batch(row, model, attempt)
    out = SimpleNamespace(row=row, model=model, attempt=attempt, tx=tx, rx=rx, ty=ty, levels=levels(row, model), fixed=ed.fixed,
                          pos=pos, raw=ed.raw, param=param, ref=ref, roles=roles, zero_pos=_exact(row, zed.pos), zero_raw=zed.raw)
    for v in (out.pos, out.raw, out.zero_pos, out.zero_raw, *ref.values(), *(s.raw for s in roles)):
        v.setflags(write=False)
    return out


def handle_actions(inp, raw):
    """What reaches the handle: the columns of the links without a fixed action, int32."""
    return np.ascontiguousarray(raw[:, N_FIXED if inp.row.fixed else 0:], dtype=np.int32)


# ---- the arms
def terms(inp, raw=None):
    """[B, j, i] float64 mW: what the transmitter of link j adds at the receiver of link i (simulator.py:97-101), from the oracle's own
    path loss; the diagonal is the own term."""
    row, model = inp.row, inp.model
    cols = columns(row, model)
    _, pwr = orc.decode_actions(inp.raw if raw is None else raw, inp.levels[None, :])
    pl = orc.pair_path_loss_db(spec(model), np.asarray(inp.pos, dtype=np.float64), inp.tx, inp.rx, cols)
    return orc.db_to_linear((pwr + cols.eirp_off_db[inp.tx][None, :])[:, :, None] - pl)


def decode_bound(row, levels_):
    """[N]: the largest action the multiply-high decode takes (refresh_tables): min(2^32 / P, 2^24 - 1, R P - 1)."""
    p = levels_.astype(np.int64)
    return np.minimum(np.minimum(0xFFFFFFFF // p, (1 << 24) - 1), row.rbs * p - 1)


def classify(inp):
    """(arm [B, N] of ARMS, clear [B, N] bool: CLEARANCE away from the arm's boundary, divided [B, N] bool: decoded by division)."""
    row = inp.row
    t = terms(inp)
    rb = inp.ref['rb']
    arm = np.empty((B, row.n), dtype=object)
    clear = np.ones((B, row.n), dtype=bool)
    for e in range(B):
        for i in range(row.n):
            if not 0 <= rb[e, i] < row.rbs:
                arm[e, i] = 'oor_sweep'
                continue
            members = np.flatnonzero(rb[e] == rb[e, i])
            m = len(members)
            if m <= SLOTS:
                v = t[e, members, i]                              # the own term among them
                bound = 2.0 ** 25
            else:
                v = t[e, members[members != i], i]                # the own entry is left out
                bound = 2.0 ** (53 - 24 - int(m).bit_length())
            ratio = v.max() / v.min()
            exact = ratio < bound
            clear[e, i] = ratio * CLEARANCE <= bound or ratio >= bound * CLEARANCE
            if m <= SLOTS:
                arm[e, i] = 'common' if exact else 're_sorted'
            else:
                arm[e, i] = 'pool_order_free' if exact else ('pool_selection' if m <= 32 else 'pool_sweep')
    divided = (inp.raw < 0) | (inp.raw > decode_bound(row, inp.levels)[None, :])
    if row.fixed:
        divided[:, :N_FIXED] = True
    return arm, clear, divided


def arm_counts(inp):
    """{arm: links that witness it (clear of its boundary)} and 'divided', 'band' (links inside a boundary's band: witnesses of nothing)."""
    arm, clear, divided = classify(inp)
    out = {a: int(((arm == a) & clear).sum()) for a in ARMS}
    out['divided'] = int(divided.sum())
    out['band'] = int((~clear).sum())
    return out


def rel_err(got, ref):
    """max |got - ref| / max(|ref|, 1); a NaN counts as infinite."""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    err = np.where(np.isnan(err), np.inf, err)
    return float(err.max()) if err.size else 0.0

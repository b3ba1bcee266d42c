"""What the large read-side tests share (test_read_side_cpu.py, test_gpu_read_side_large.py): the seeded cases of the direct launches of
csrc/d2d_marginal.hip, d2d_graph.hip and d2d_sense.hip past 256 links, and float64 references that need no oracle spec and no
[b, j, r] one-hot: the pair path loss for any law columns, the per-RB interference sums, the leave-one-out capacities from RB member
lists, and the coupling matrix.  test_read_side_cpu.py ties each of them to the oracle where the oracle has the law.

Index order: pair_pl_db is [b, j, i] (transmitter link j first, as orc.pair_path_loss_db); everything else is receiver first."""
from functools import lru_cache

import numpy as np

import best_rb_util as bru
import neighbors_util as nbu
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

BAR = bru.BAR
# links: (cues, due pairs) - best_rb_util.SHAPES and the shapes that are new here
#   259: N % 4 != 0 above 256, a second receiver block of 3 rows (sense), a third of 3 rows (coupling)
#   260: N % 4 == 0 with ONE float4 group behind column 256
#   1000: marginal above 64 KiB with a power law, N % 64 != 0
SHAPES = {**bru.SHAPES, 259: (59, 200), 260: (60, 200), 1000: (300, 700)}
CELL_40 = bru.ORACLE_CELL_M

# ---- the GPU cases; test_read_side_cpu.py checks the caps below on the references of these very seeds
# (links, RBs, law, envs, cell radius): the path it forces | undecided share measured on the float64 reference (cap 1 %)
MARGINAL_CASES = (
    (259, 33, 'ld35', 2, 500.0),      # N % 4 != 0, sorted slots >= 256 in both phase loops, 18.4 KiB                  | 0.00 %
    (1000, 8, 'mixed', 2, 500.0),     # 70.4 KiB: the first shape of the MaxDynamicSharedMemorySize branch; j up to 999     | 0.00 %
    (1000, 8, 'ld2', 2, 500.0),       # 62.6 KiB: the same shape just below the branch                                  | 0.00 %
    (2048, 64, 'ld35', 2, 500.0),     # 144 KiB, j >= 1024 in the key rb << 11 | j                                      | 0.00 %
    (2048, 64, 'ld2', 2, 500.0),      # 128 KiB                                                                         | 0.00 %
    (300, 1, 'urban', 2, CELL_40),    # 300-member sums: every link harms 299 others                                    | 0.00 %
    (2048, 3, 'ld35', 1, CELL_40),    # about 680 members per RB: acc - td over hundreds of terms                       | 0.00 %
)
MARGINAL_RELAUNCH = (259, 33, 'ld35', 2, 500.0)
MARGINAL_WIDE_R = 4000                # the 1000-link 'mixed' case once more on 4000 RBs: 86 KiB with a 16 KiB start array
# (links, law, envs)
COUPLING_CASES = (
    (259, 'ld2', 2),                  # non-VEC by shape; second c0 trip with 3 live columns; third receiver block of 3 rows
    (1000, 'mixed', 2),               # four c0 trips, the last with 232 columns; eight receiver blocks, the last of 104 rows
    (2048, 'ld35', 1),                # 16 receiver blocks, 8 column trips
    (260, 'ld2', 2),                  # VEC with a last group of one float4 at c0 = 256
)
# (links, law, envs, downlink): near-tie share left out at k = 1 / 8 / 64 on the float64 reference (cap neighbors_util.CAP = 5 %)
NEIGHBOR_CASES = (
    (259, 'ld35', 2, False),          # 5 keys per lane, N % 64 = 3, win_j >= 256                                   | 0 / 0.31 / 2.57 %
    (259, 'ld2', 2, True),            # downlink: 59 links share the BS as transmitter - 91 % of the gaps exact ties   | 0 / 0.00 / 0.01 %
    (1000, 'mixed', 2, False),        # 16 keys per lane, 39 KiB                                                     | 0 / 0.24 / 2.72 %
    (2048, 'ld35', 1, False),         # 80 KiB: the MaxDynamicSharedMemorySize branch; 32 keys per lane; j >= 1024   | 0 / 0.24 / 3.64 %
    (2048, 'ld2', 1, False),          # 64 KiB exactly: NOT above the branch (lds > 64 KiB is false)                 | 0 / 0.29 / 3.79 %
)
KS = (1, 8, 64)
# (links, RBs, law, envs)
SENSE_CASES = (
    (259, 37, 'ld35', 2),             # R % 4 != 0: scalar stores, two tiles (32 + 5), second receiver block of 3 rows
    (259, 44, 'ld2', 2),              # ragged vector tile cw = 12
    (41, 330, 'mixed', 2),            # eleven tiles, the last a scalar tail of 10 (R % 4 == 2)
    (2048, 5, 'mixed', 2),            # 80.5 KiB: the MaxDynamicSharedMemorySize branch; eight receiver blocks
    (2048, 64, 'ld2', 1),             # two full vector tiles at the link limit; 64.8 KiB: the branch under the inverse-square law
)


def law_columns(law, cues, dues):
    """The per-device law columns {'a_tx_db', 'a_rx_db', 'exponent'} of a case, float64 - what best_rb_util.make_case folds."""
    from gym_d2d_amd.envs.env_config import EnvConfig
    from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss, LogDistancePathLoss
    from gym_d2d_amd.simulator import create_devices
    d = 1 + cues + 2 * dues
    if law == 'mixed':
        k = np.arange(d)
        return {'a_tx_db': 40.0 + (k % 3), 'a_rx_db': 1.5 * (k % 2), 'exponent': np.where(k % 2 == 1, 3.7, 2.2)}
    model = {'ld2': lambda: LogDistancePathLoss(2.1), 'ld35': lambda: LogDistancePathLoss(2.1, ple=3.5),
             'urban': lambda: CostHataPathLoss(2.1, AreaType.URBAN), 'suburban': lambda: CostHataPathLoss(2.1, AreaType.SUBURBAN)}[law]
    devs = list(create_devices(EnvConfig(num_cues=cues, num_due_pairs=dues)).values())
    return {k: np.asarray(v, dtype=np.float64) for k, v in model().power_law_columns(devs).items()}


def oracle_spec(law):
    return {'ld2': orc.PathLossSpec('log_distance', 2.1, ple=2.0), 'ld35': orc.PathLossSpec('log_distance', 2.1, ple=3.5),
            'urban': orc.PathLossSpec('cost_hata', 2.1, area='urban'), 'suburban': orc.PathLossSpec('cost_hata', 2.1, area='suburban'),
            'mixed': None}[law]


@lru_cache(maxsize=None)
def build_case(cues, dues, r, law, b=2, cell_radius=500.0, downlink=False):
    """best_rb_util.make_case's recipe for any (cues, due pairs): seeded float32 positions from random_layout, rb with about a tenth
    outside [0, R), tx power levels, the folded columns.  downlink: the CUE links run from device 0 to the CUE, as
    DownlinkTrafficModel builds them.  Beyond make_case's fields: law_cols, cap_cols (d2d_marginal_capacity's) and law."""
    from gym_d2d_amd.sensing import fold_columns
    n, d = cues + dues, 1 + cues + 2 * dues
    rng = np.random.default_rng(1000 * n + 10 * r + sum(map(ord, law)) + int(cell_radius) + (7 if downlink else 0))
    pos = random_layout(rng, b, cues, dues, cell_radius=cell_radius)
    tx, rx, _ = default_links(cues, dues)
    if downlink:
        tx, rx = tx.copy(), rx.copy()
        tx[:cues], rx[:cues] = 0, np.arange(1, 1 + cues)
    rb = rng.integers(0, r, (b, n)).astype(np.int32)
    bad = rng.random((b, n)) < 0.1
    bad[0, 0] = True
    rb[bad] = rng.choice([-1, -7, r, r + 1, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    pwr = rng.integers(0, 20, (b, n)).astype(np.int32)
    ocols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    law_cols = law_columns(law, cues, dues)
    budget = {'eirp_off_db': ocols.eirp_off_db, 'rx_off_db': ocols.rx_off_db, 'noise_dbm': ocols.noise_dbm}
    cols, kind, pow_k = fold_columns(budget, law_cols, tx)
    return _finish(dict(b=b, n=n, d=d, r=r, pos=pos, tx=tx.astype(np.int32), rx=rx.astype(np.int32), rb=rb, pwr=pwr, bad=bad, cols=cols,
                        kind=kind, pow_k=pow_k, ocols=ocols, spec=oracle_spec(law)), law, law_cols)


def _finish(c, law, law_cols):
    from gym_d2d_amd.marginal import fold_capacity_columns
    c['law'], c['law_cols'] = law, law_cols
    c['cap_cols'] = fold_capacity_columns({'bw_hz': c['ocols'].bw_hz, 'sens_dbm': c['ocols'].sens_dbm})
    return c


@lru_cache(maxsize=None)
def make_case(n, r, law, b=2, cell_radius=500.0, downlink=False):
    """The case of a link count: best_rb_util.make_case itself where its SHAPES has the count (uplink), build_case otherwise."""
    cues, dues = SHAPES[n]
    if n in bru.SHAPES and not downlink:
        return _finish(dict(bru.make_case(n, r, law, b=b, cell_radius=cell_radius)), law, law_columns(law, cues, dues))
    return build_case(cues, dues, r, law, b=b, cell_radius=cell_radius, downlink=downlink)


def lds_bytes(kernel, n, r=1, power_law=False):
    """The dynamic LDS a launch asks for, by the layouts written in the kernels' sources: which side of the 64 KiB branch a case is on."""
    r16 = lambda x: (x + 15) & ~15
    n4, hh = (n + 3) & ~3, r16(8 * n) if power_law else 0
    if kernel == 'marginal':
        return 16 * n + hh + 32 * n + r16(8 * n4) + 2 * r16(4 * n) + r16(4 * (r + 1))
    if kernel == 'neighbors':
        return 16 * n + hh + 4 * 4 * ((n + 63) & ~63)
    assert kernel == 'sense'
    return 16 * n + hh + r16(4 * (r + 1)) + max(4 * n4 + 4 * n, 4 * 32 * 65 * 4)


def with_rb(c, rb, r=None):
    """The case on another rb plane (and RB count); nothing else changes."""
    rb = np.ascontiguousarray(rb, dtype=np.int32)
    r = c['r'] if r is None else int(r)
    return dict(c, rb=rb, r=r, bad=(rb < 0) | (rb >= r))


# ------------------------------------------------------------------------------------------ float64 references
def pair_pl_db(c):
    """PL[b, j, i] in dB from the transmitter of link j to the receiver of link i, float64, for ANY law columns: the power law
    sensing.fold_columns lowers, a_tx_db[tx_j] + a_rx_db[rx_i] + 10 exponent[tx_j] log10(d) - LogDistancePathLoss with a_tx the
    path-loss constant, CostHataPathLoss with its slope / 10 as the exponent and log10(d_km) folded into a_tx (path_loss.py)."""
    pos = np.asarray(c['pos'], dtype=np.float64)
    tx, rx = np.asarray(c['tx'], dtype=np.int64), np.asarray(c['rx'], dtype=np.int64)
    t, r = pos[:, tx], pos[:, rx]
    dx = t[:, :, None, 0] - r[:, None, :, 0]
    dy = t[:, :, None, 1] - r[:, None, :, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    law = c['law_cols']
    a_tx, a_rx, expo = (np.asarray(law[k], dtype=np.float64) for k in ('a_tx_db', 'a_rx_db', 'exponent'))
    with np.errstate(divide='ignore'):
        return a_tx[tx][None, :, None] + a_rx[rx][None, None, :] + 10.0 * expo[tx][None, :, None] * np.log10(dist)


def _received_mw(c, pl=None):
    """mw[b, j, i]: what the receiver of link i takes in from the transmitter of link j before its own rx offset (simulator.py:97-101),
    the diagonal set to 0; and eirp[b, j]."""
    pl = pair_pl_db(c) if pl is None else pl
    n = c['n']
    eirp = np.asarray(c['pwr'], dtype=np.float64) + c['ocols'].eirp_off_db[np.asarray(c['tx'])][None, :]
    mw = 10.0 ** ((eirp[:, :, None] - pl) / 10.0)
    mw[:, np.arange(n), np.arange(n)] = 0.0
    return mw, eirp


def interference_per_rb(c, pl=None):
    """I[b, i, r] in mW, float64: the sum over the links j != i on RB r of their received power at i.  Scattered by RB with np.add.at
    - no [b, j, r] one-hot, which at 330 RBs x 2048 links does not fit."""
    mw, _ = _received_mw(c, pl)
    b, n, r = c['b'], c['n'], c['r']
    rb = np.asarray(c['rb'], dtype=np.int64)
    out = np.zeros((b, r, n))
    for e in range(b):
        on = np.nonzero((rb[e] >= 0) & (rb[e] < r))[0]
        np.add.at(out[e], rb[e, on], mw[e, on, :])
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def signal_dbm(c, pl=None):
    """sig[b, i] = eirp_i - PL_ii + rx_off (simulator.py:93) and the receivers' noise in dBm [N]."""
    pl = pair_pl_db(c) if pl is None else pl
    n = c['n']
    tx, rx = np.asarray(c['tx']), np.asarray(c['rx'])
    eirp = np.asarray(c['pwr'], dtype=np.float64) + c['ocols'].eirp_off_db[tx][None, :]
    return eirp - pl[:, np.arange(n), np.arange(n)] + c['ocols'].rx_off_db[rx][None, :], c['ocols'].noise_dbm[rx]


def sinr_per_rb(c, ix_mw, pl=None):
    """sinr_db[b, i, r] = sig_i - dB(I + lin(noise_i)): rb_sensing_util.sinr_from_interference on pair_pl_db."""
    sig, noise = signal_dbm(c, pl)
    return sig[:, :, None] - 10.0 * np.log10(ix_mw + (10.0 ** (noise / 10.0))[None, :, None])


def leave_one_out_direct(c, bar=BAR, pl=None):
    """(difference_mbps, harm_mbps, capacity_mbps, decided), [B, N] each, float64 and bool, from the member lists of the RBs.

    Per env and RB with members M: G[j, i] the received power of j at i, W[k, i] = sum over j in M, j != i, j != k of G[j, i] - formed
    as a product with a 0 / 1 matrix, a sum of non-negative terms with no cancellation - so that W[i, i] is the interference the
    step sees at i and W[k, i] what is left without link k.  The simulator's definitions (simulator.py:123,149-151): sinr_db > sens
    -> bw_mhz log2(1 + sinr), else 0.  harm[k] = sum over i != k of cap(W[k, i]) - cap(W[i, i]); difference = capacity - harm.
    A link whose rb is outside [0, R) is alone.

    decided[b, k]: neither k's own SINR nor, for any victim i on its RB, i's SINR with or without k lies within
    2 bar max(|sinr|, 1) dB of that receiver's sensitivity - a victim on the threshold flips a whole capacity.

    pl: the pair path loss [b, j, i] to use instead of pair_pl_db(c) (a case that has an oracle spec and no law columns)."""
    pl = pair_pl_db(c) if pl is None else pl
    mw, _ = _received_mw(c, pl)
    sig, noise_dbm = signal_dbm(c, pl)
    b, n, r = c['b'], c['n'], c['r']
    tx, rx = np.asarray(c['tx']), np.asarray(c['rx'])
    noise = 10.0 ** (noise_dbm / 10.0)
    bw_mhz, sens = 1e-6 * c['ocols'].bw_hz[tx], c['ocols'].sens_dbm[rx]
    rb = np.asarray(c['rb'], dtype=np.int64)

    def cap_of(sinr_db, members):
        return np.where(sinr_db > sens[members], bw_mhz[members] * np.log2(1.0 + 10.0 ** (sinr_db / 10.0)), 0.0)

    def near(sinr_db, members):
        return np.abs(sinr_db - sens[members]) <= 2.0 * bar * np.maximum(np.abs(sinr_db), 1.0)
    cap, harm, decided = np.zeros((b, n)), np.zeros((b, n)), np.ones((b, n), bool)
    for e in range(b):
        on = (rb[e] >= 0) & (rb[e] < r)
        groups = [np.nonzero(on & (rb[e] == q))[0] for q in np.unique(rb[e][on])] + [np.array([j]) for j in np.nonzero(~on)[0]]
        for m in groups:
            g = mw[e][np.ix_(m, m)]                                        # [j, i], zero diagonal
            w = (1.0 - np.eye(len(m))) @ g                                 # [k, i]
            sinr = sig[e, m][None, :] - 10.0 * np.log10(w + noise[m][None, :])
            caps = cap_of(sinr, m[None, :])
            base = np.diagonal(caps)
            gain = caps - base[None, :]
            np.fill_diagonal(gain, 0.0)
            cap[e, m], harm[e, m] = base, gain.sum(axis=1)
            close = near(sinr, m[None, :])
            own = np.diagonal(close)
            decided[e, m] = ~(close.any(axis=1) | own.any())
    return cap - harm, harm, cap, decided


def coupling_ref(c, pl=None):
    """ref[b, i, j] = eirp_off_db[tx_j] - PL(tx_j -> rx_i): neighbors_util.coupling_ref on pair_pl_db."""
    pl = pair_pl_db(c) if pl is None else pl
    return np.ascontiguousarray((c['ocols'].eirp_off_db[np.asarray(c['tx'])][None, :, None] - pl).transpose(0, 2, 1))


@lru_cache(maxsize=None)
def neighbor_case(n, law, b, downlink):
    """(case, ref [B, N, N]) of a NEIGHBOR_CASES entry; the rb plane is not used (one RB)."""
    c = make_case(n, 1, law, b=b, downlink=downlink)
    return c, coupling_ref(c)


@lru_cache(maxsize=None)
def neighbor_ranked(n, law, b, downlink, k):
    return nbu.ranked(neighbor_case(n, law, b, downlink)[1], k)


@lru_cache(maxsize=None)
def wide_r_case():
    """The 1000-link 'mixed' case on ONE rb plane under two RB counts, (on 8 RBs, on MARGINAL_WIDE_R RBs): the plane of the 8-RB case
    with its off-RB values 8 and 9 moved out of both ranges, so that every link stands where it stood and both launches must give the
    harm of the 8-RB case."""
    c = make_case(1000, 8, 'mixed')
    rb = c['rb'].copy()
    rb[c['rb'] == 8], rb[c['rb'] == 9] = MARGINAL_WIDE_R, MARGINAL_WIDE_R + 1
    return with_rb(c, rb), with_rb(c, rb, MARGINAL_WIDE_R)


@lru_cache(maxsize=None)
def marginal_ref(n, r, law, b, cell_radius):
    """leave_one_out_direct of a MARGINAL_CASES entry (or of the wide-R case), computed once and left unchanged."""
    c = wide_r_case()[1] if r == MARGINAL_WIDE_R else make_case(n, r, law, b=b, cell_radius=cell_radius)
    return leave_one_out_direct(c)

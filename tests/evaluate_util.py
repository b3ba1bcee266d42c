"""What the what-if evaluation tests share (test_evaluate_cpu.py, test_gpu_evaluate.py): a float64 reference that takes explicit
positions, link lists, candidate planes and columns, and the seeded cases of the direct launches of csrc/d2d_evaluate.hip.

The reference is the simulator's definition (simulator.py:93-151) on read_side_util.pair_pl_db: per candidate, the interference at a
link's receiver is the sum over the OTHER links of its RB, sinr_db = signal - dB(I + noise), capacity = bw_mhz log2(1 + sinr) where
sinr_db > sensitivity, else 0, total = the sum of the capacities.  A link whose rb is outside [0, R) shares with nobody.
test_evaluate_cpu.py ties it to the oracle's step where the oracle has the law."""
from functools import lru_cache

import numpy as np

import read_side_util as rsu

BAR = rsu.BAR                                # the project's bar: |d| <= BAR max(|ref|, 1) on sinr_db (dB) and capacity_mbps (Mbps)
THRESHOLD_DB = 1e-4                          # links whose reference sinr_db lies this close to the sensitivity: capacity not compared
THRESHOLD_CAP = 0.01                         # ... at most this share of a case
B = 3
CHUNK = 8                                    # include/d2d_evaluate.h: D2D_EVALUATE_CHUNK
P_LOW, P_HIGH = 0, 23                        # the lowest and the highest power level a default CUE has (dBm)

# links: (cues, due pairs)
SHAPES = {1: (1, 0), 3: (1, 2), 63: (13, 50), 65: (15, 50), 257: (57, 200), 260: (60, 200), 300: (100, 200), 1000: (300, 700)}
# (links, RBs, law, K): the path it forces.  laws: 'ld2' inverse square, 'ld35' an exponent of 3.5 (PL_POWK), 'mixed' per-device
# exponents that force the general split (PL_POWER)
CASES = (
    (1, 3, 'ld2', 1),                # no interferer; one candidate
    (3, 1, 'ld35', 2),               # all links share the one RB
    (63, 5, 'mixed', CHUNK),         # one wave, not full; exactly one chunk
    (65, 5, 'ld2', CHUNK + 1),       # one lane of a second wave; a second workgroup with ONE candidate
    (257, 7, 'ld35', 33),            # second pass of the 256-thread loops; five chunks, the last with one candidate
    (300, 1, 'ld2', 2),              # 299-term sums
    (260, 4000, 'mixed', 2),         # mostly empty RBs, a 16 KiB start[]
    (1000, 8, 'mixed', 2),           # 80 KiB of LDS: the MaxDynamicSharedMemorySize branch
)
KIND = {'ld2': 0, 'mixed': 1, 'ld35': 2}     # the law id sensing.fold_columns gives each


def lds_bytes(n, r, power_law):
    """The dynamic LDS a launch asks for, by the layout written in csrc/d2d_evaluate.hip."""
    r16 = lambda x: (x + 15) & ~15
    n4, hh = (n + 3) & ~3, r16(8 * n) if power_law else 0
    return 16 * n + 16 * n + r16(8 * n) + hh + 16 * n + hh + 4 * n4 + r16(4 * n) + r16(4 * (r + 1)) + 32


@lru_cache(maxsize=None)
def make_case(n, r, law, k, b=B, cell_radius=500.0):
    """The seeded case of a CASES entry: read_side_util.build_case's layout and columns, and K candidate planes rb / pwr int32
    [B, K, N] of its own: rb uniform over the RBs, powers uniform over P_LOW .. P_HIGH with a third of the links at each end."""
    cues, dues = SHAPES[n]
    c = dict(rsu.build_case(cues, dues, r, law, b=b, cell_radius=cell_radius))
    rng = np.random.default_rng(77 + 1000 * n + 10 * r + k + sum(map(ord, law)))
    rb = rng.integers(0, r, (b, k, n)).astype(np.int32)
    pwr = rng.integers(P_LOW, P_HIGH + 1, (b, k, n)).astype(np.int32)
    end = rng.random((b, k, n))
    pwr[end < 1 / 3], pwr[end > 2 / 3] = P_LOW, P_HIGH
    pwr[0, 0, 0], pwr[-1, -1, -1] = P_LOW, P_HIGH                        # both ends at one link and one candidate too
    c.update(k=k, rb=rb, pwr=pwr, bad=np.zeros_like(rb, bool))
    return c


def contrast_planes(c, k=33):
    """K candidates for the case's layout in which consecutive candidates differ maximally: everyone on one RB, then everyone
    spread out (link j on RB j mod R), alternating, with powers that flip between the ends as well."""
    b, n, r = c['b'], c['n'], c['r']
    rb = np.empty((b, k, n), dtype=np.int32)
    pwr = np.empty((b, k, n), dtype=np.int32)
    for q in range(k):
        rb[:, q] = (q // 2) % r if q % 2 == 0 else (np.arange(n) + q) % r
        pwr[:, q] = P_HIGH if q % 4 < 2 else np.where(np.arange(n) % 2 == 0, P_LOW, P_HIGH)
    return rb, pwr


def evaluate_ref(pos, link_tx, link_rx, rb, pwr, columns, num_rbs):
    """(sinr_db, capacity_mbps [B, K, N], total_mbps [B, K]), float64.  pos [B, D, 2]; rb, pwr int [B, K, N] (or [K, N] with B = 1);
    columns: {'ocols': the oracle's device columns, 'law_cols': {'a_tx_db', 'a_rx_db', 'exponent'} per device} or, in their place,
    'pl': the pair path loss [B, j, i] in dB (a case that has an oracle spec and no law columns)."""
    pos = np.asarray(pos, dtype=np.float64)
    rb, pwr = np.asarray(rb, dtype=np.int64), np.asarray(pwr, dtype=np.int64)
    if rb.ndim == 2:
        rb, pwr = rb[None], pwr[None]
    b, k, n = rb.shape
    tx, rx = np.asarray(link_tx, dtype=np.int64), np.asarray(link_rx, dtype=np.int64)
    ocols = columns['ocols']
    base = dict(b=b, n=n, r=int(num_rbs), pos=pos, tx=tx, rx=rx, ocols=ocols, law_cols=columns.get('law_cols'))
    pl = columns['pl'] if 'pl' in columns else rsu.pair_pl_db(base)                           # [b, j, i]
    noise = 10.0 ** (ocols.noise_dbm[rx] / 10.0)
    bw_mhz, sens = 1e-6 * ocols.bw_hz[tx], ocols.sens_dbm[rx]
    idx = np.arange(n)
    sinr, cap = np.empty((b, k, n)), np.empty((b, k, n))
    for q in range(k):
        eirp = pwr[:, q] + ocols.eirp_off_db[tx][None, :]                                      # [b, j]
        mw = 10.0 ** ((eirp[:, :, None] - pl) / 10.0)                                          # [b, j, i]
        on = (rb[:, q] >= 0) & (rb[:, q] < num_rbs)
        same = (rb[:, q, :, None] == rb[:, q, None, :]) & on[:, :, None] & on[:, None, :]
        same[:, idx, idx] = False
        ix = (mw * same).sum(axis=1)                                                           # [b, i]
        sig = eirp - pl[:, idx, idx] + ocols.rx_off_db[rx][None, :]
        s = sig - 10.0 * np.log10(ix + noise[None, :])
        sinr[:, q] = s
        cap[:, q] = np.where(s > sens[None, :], bw_mhz[None, :] * np.log2(1.0 + 10.0 ** (s / 10.0)), 0.0)
    return sinr, cap, cap.sum(axis=2)


@lru_cache(maxsize=None)
def case_ref(n, r, law, k):
    """evaluate_ref of a CASES entry and the links left out of its capacity comparison, computed once and left unchanged:
    (sinr_db, capacity_mbps, total_mbps, decided bool [B, K, N])."""
    c = make_case(n, r, law, k)
    sinr, cap, total = evaluate_ref(c['pos'], c['tx'], c['rx'], c['rb'], c['pwr'], c, r)
    sens = c['ocols'].sens_dbm[np.asarray(c['rx'])]
    return sinr, cap, total, np.abs(sinr - sens[None, None, :]) > THRESHOLD_DB


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max()) if ref.size else 0.0

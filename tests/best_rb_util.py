"""What the best-response RB tests share: the seeded cases of the direct launches, the lowering of their models to the kernel's
columns, and the oracle's side of the comparison (expected best RB per link, and which links are near-ties)."""
from functools import lru_cache

import numpy as np

import rb_sensing_util as rbs
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

BAR = 1e-5                                   # the project's bar on dB quantities: |d| <= BAR max(|ref|, 1)
SHAPES = {7: (3, 4), 41: (11, 30), 131: (31, 100), 300: (100, 200), 2048: (512, 1536)}     # links: (cues, due pairs)
DIRECT_N, DIRECT_R = (7, 131, 300), (1, 3, 33, 70)
# the direct launches past those: (links, R, law, envs)
#   2048 links at a small R: EIGHT receiver blocks (grid.y; 2 at most up to 300 links), link index 2047 in the sort key rb << 11 | j,
#   and with a power law more than 64 KiB of LDS in d2d_bestrb.hip - the MaxDynamicSharedMemorySize branch, which d2d_sense.hip takes
#   for the reference block of the same case as well
#   41 links on 330 RBs: an allowed mask of ELEVEN words with a ragged tail of 10 bits (R = 70 has three)
DIRECT_LARGE = ((2048, 3, 'ld35', 2), (2048, 3, 'mixed', 2), (2048, 5, 'ld2', 2), (41, 330, 'ld2', 3))
# the oracle comparison at 2048 links: one env, these links on every RB (nine oracle envs of 2048 x 2048 pairs each)
LARGE_ORACLE = (2048, 3, 'ld35', (0, 1024, 2047))
LAWS = ('ld2', 'ld35', 'urban')              # the models the oracle knows; 'mixed' below has per-device exponents (the general law)
# the oracle comparison: every R at 7 links, the two R either side of the 32-RB grouping at 41 (B0 * N * R oracle envs each)
# ... in a 40 m cell: at the default 500 m most interferers under the steeper laws arrive far below the noise floor, so an occupied RB
# sits within twice the bar of the link's SNR and almost every link is a near-tie between an occupied and an empty RB, which no
# bar-limited comparison can decide.  In a compact cell every interferer counts and the oracle decides every link
# (test_best_rb_cpu.py checks the share that is left out on the oracle alone).  The bit-for-bit cases keep the 500 m cell.
ORACLE_CELL_M = 40.0
ORACLE_CASES = [(7, r, law) for r in DIRECT_R for law in LAWS] + [(41, r, law) for r in (3, 33) for law in LAWS]


def _model(law):
    from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss, LogDistancePathLoss
    return {'ld2': (lambda: LogDistancePathLoss(2.1), orc.PathLossSpec('log_distance', 2.1, ple=2.0)),
            'ld35': (lambda: LogDistancePathLoss(2.1, ple=3.5), orc.PathLossSpec('log_distance', 2.1, ple=3.5)),
            'urban': (lambda: CostHataPathLoss(2.1, AreaType.URBAN), orc.PathLossSpec('cost_hata', 2.1, area='urban'))}[law]


@lru_cache(maxsize=None)
def make_case(n, r, law, b=3, cell_radius=500.0):
    """One seeded state for a direct launch: float32 positions, the default link list, rb with about a tenth outside [0, R), tx
    power levels, the folded columns with their law id, and the oracle's columns and spec (None for 'mixed')."""
    from gym_d2d_amd.envs.env_config import EnvConfig
    from gym_d2d_amd.sensing import fold_columns
    from gym_d2d_amd.simulator import create_devices
    cues, dues = SHAPES[n]
    rng = np.random.default_rng(1000 * n + 10 * r + sum(map(ord, law)) + int(cell_radius))
    d = 1 + cues + 2 * dues
    pos = random_layout(rng, b, cues, dues, cell_radius=cell_radius)
    tx, rx, _ = default_links(cues, dues)
    rb = rng.integers(0, r, (b, n)).astype(np.int32)
    bad = rng.random((b, n)) < 0.1
    bad[0, 0] = True                                                    # at least one, also at 7 links
    rb[bad] = rng.choice([-1, -7, r, r + 1, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    pwr = rng.integers(0, 20, (b, n)).astype(np.int32)
    ocols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    budget = {'eirp_off_db': ocols.eirp_off_db, 'rx_off_db': ocols.rx_off_db, 'noise_dbm': ocols.noise_dbm}
    if law == 'mixed':
        k = np.arange(d)
        law_cols, spec = {'a_tx_db': 40.0 + (k % 3), 'a_rx_db': 1.5 * (k % 2), 'exponent': np.where(k % 2 == 1, 3.7, 2.2)}, None
    else:
        model, spec = _model(law)
        devs = list(create_devices(EnvConfig(num_cues=cues, num_due_pairs=dues)).values())
        law_cols = model().power_law_columns(devs)
    cols, kind, pow_k = fold_columns(budget, law_cols, tx)
    return dict(b=b, n=n, d=d, r=r, pos=pos, tx=tx.astype(np.int32), rx=rx.astype(np.int32), rb=rb, pwr=pwr, bad=bad, cols=cols,
                kind=kind, pow_k=pow_k, ocols=ocols, spec=spec)


def occupied(rb, r):
    """[B, N, R] bool: some OTHER link of the env sits on RB r."""
    onehot = rb[:, :, None] == np.arange(r)[None, None, :]              # [b, j, r]
    return (onehot.sum(axis=1, keepdims=True) - onehot) > 0


@lru_cache(maxsize=None)
def oracle_side(n, r, law):
    """(ref float64 [B, N, R], expect int [B, N], decided bool [B, N]) of a case.  expect is the oracle's argmax; a link is decided
    when that argmax is safe from the bar: either no other RB comes within twice the bar of the top value, or every RB that does
    is one nobody else uses - those tie exactly (sinr == snr on each of them) and must resolve to the lowest r.  Every other link
    is a near-tie that involves an occupied RB and is left out."""
    c = make_case(n, r, law, cell_radius=ORACLE_CELL_M)
    ref = rbs.counterfactual(c['pos'], c['tx'], c['rx'], c['rb'], c['pwr'], c['ocols'], c['spec'], r)
    top = ref.max(axis=-1)
    cand = ref >= (top - 2.0 * BAR * np.maximum(np.abs(top), 1.0))[:, :, None]
    only_empty = ~(cand & occupied(c['rb'], r)).any(axis=-1)
    assert (np.where(cand, ref, top[:, :, None])[only_empty] == top[only_empty][:, None]).all()       # exact ties, not near ones
    decided = (cand.sum(axis=-1) == 1) | only_empty
    return ref, cand.argmax(axis=-1), decided


@lru_cache(maxsize=None)
def large_oracle_side():
    """oracle_side() for LARGE_ORACLE: (case, ref float64 [1, K, R], expect int [1, K], decided bool [1, K]) of its K links in env 0."""
    n, r, law, links = LARGE_ORACLE
    c = make_case(n, r, law, b=2, cell_radius=ORACLE_CELL_M)
    links = np.asarray(links)
    ref = rbs.counterfactual(c['pos'][:1], c['tx'], c['rx'], c['rb'][:1], c['pwr'][:1], c['ocols'], c['spec'], r, links=links)
    top = ref.max(axis=-1)
    cand = ref >= (top - 2.0 * BAR * np.maximum(np.abs(top), 1.0))[:, :, None]
    only_empty = ~(cand & occupied(c['rb'][:1], r)[:, links]).any(axis=-1)
    decided = (cand.sum(axis=-1) == 1) | only_empty
    return c, ref, cand.argmax(axis=-1), decided

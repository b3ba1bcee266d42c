"""The yardstick of the difference-reward tests: leave-one-out capacities from the oracle's own step."""
import json

import numpy as np

from golden_util import GOLDEN_DIR
from oracle import d2d_oracle as orc


def leave_one_out(pos, link_tx, link_rx, rb, pwr, cols, spec, num_rbs):
    """(difference_mbps, harm_mbps, capacity_mbps, g_without), float64 [B0, N] each, from ONE oracle step on the B0 * N envs in
    which link i sits on pseudo-RB R - an RB of its own, where it meets nobody: g_without[b, i] is the sum over k != i of that
    env's capacities, i.e. the total capacity of the step with link i's entry dropped.  A link whose rb is outside [0, R) is on no
    RB (as in sense()): it gets a pseudo-RB of its own in every env, the base step included.  pos [B0, D, 2], rb / pwr [B0, N]."""
    pos = np.asarray(pos, dtype=np.float64)
    rb = np.asarray(rb, dtype=np.int64).copy(); pwr = np.asarray(pwr, dtype=np.int64)
    b0, n = rb.shape
    r = int(num_rbs)
    idx = np.arange(n)
    off = (rb < 0) | (rb >= r)
    rb[off] = np.broadcast_to(r + 1 + idx, rb.shape)[off]
    base = orc.step(pos, link_tx, link_rx, rb, pwr, cols, spec)['capacity_mbps']                  # [b0, n]
    big_rb = np.broadcast_to(rb[:, None, :], (b0, n, n)).copy()
    big_rb[:, idx, idx] = r                                                # env (b, i): link i sits on pseudo-RB R
    big_pwr = np.broadcast_to(pwr[:, None, :], (b0, n, n)).reshape(b0 * n, n)
    big_pos = np.broadcast_to(pos[:, None], (b0, n) + pos.shape[1:]).reshape((b0 * n,) + pos.shape[1:])
    cap = orc.step(big_pos, link_tx, link_rx, big_rb.reshape(b0 * n, n), big_pwr, cols, spec)['capacity_mbps'].reshape(b0, n, n)
    cap[:, idx, idx] = 0.0                                                 # k != i
    g_without = cap.sum(axis=2)
    harm = g_without - (base.sum(axis=1, keepdims=True) - base)
    return base - harm, harm, base, g_without


def load_fixture(name):
    z = np.load(GOLDEN_DIR / f'{name}.npz')
    meta = json.loads(bytes(z['meta_json']).decode())
    index = {d: k for k, d in enumerate(meta['dev_ids'])}
    tx = np.asarray([index[k.split(':')[0]] for k in meta['keys']])
    rx = np.asarray([index[k.split(':')[1]] for k in meta['keys']])
    pl = meta['path_loss']
    f = meta['carrier_freq_GHz']
    spec = orc.PathLossSpec('log_distance', f, ple=pl['ple']) if pl['kind'] == 'log_distance' else \
        orc.PathLossSpec('cost_hata', f, area=pl['area'])
    cols = orc.device_columns(meta['dev_cfgs'], z['dev_is_bs'])
    return dict(meta=meta, pos=z['dev_pos'][None], link_tx=tx, link_rx=rx, rb=z['rb'][None], pwr=z['pwr'][None],
                capacity_mbps=z['capacity_mbps'], g_without=z['g_without'], cols=cols, spec=spec)

"""What the read-side GPU tests share (test_gpu_rb_sensing.py, test_gpu_neighbors.py, test_gpu_marginal.py): their case table with its
models and the read-back of an env's state, and the yardsticks of the per-RB sensing tests - the oracle-based counterfactual and the
fp64 interference sum."""
import json

import numpy as np

from golden_util import GOLDEN_DIR
from oracle import d2d_oracle as orc


def _models():
    from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss, LogDistancePathLoss

    class Ple35(LogDistancePathLoss):
        def __init__(self, f):
            super().__init__(f, ple=3.5)

    class Urban(CostHataPathLoss):
        def __init__(self, f):
            super().__init__(f, AreaType.URBAN)

    class Suburban(CostHataPathLoss):
        def __init__(self, f):
            super().__init__(f, AreaType.SUBURBAN)
    return {'ld2': (LogDistancePathLoss, orc.PathLossSpec('log_distance', 2.1, ple=2.0)),
            'ld35': (Ple35, orc.PathLossSpec('log_distance', 2.1, ple=3.5)),
            'urban': (Urban, orc.PathLossSpec('cost_hata', 2.1, area='urban')),
            'suburban': (Suburban, orc.PathLossSpec('cost_hata', 2.1, area='suburban'))}


# name: (B0, cues, due pairs, RBs, model, cue_actions, downlink traffic model)
CASES = {
    'small_ld2_agent': (3, 8, 8, 5, 'ld2', 'agent', False),
    'mid_ld35_agent': (2, 64, 96, 24, 'ld35', 'agent', False),
    'crowded_urban_traffic_up': (2, 64, 64, 8, 'urban', 'traffic', False),          # 16 links per RB
    'empty_suburban_traffic_down': (2, 6, 6, 40, 'suburban', 'traffic', True),      # 12 links on 40 RBs
    'mid_ld2_traffic_down': (2, 24, 40, 16, 'ld2', 'traffic', True),
    'small_urban_agent': (3, 8, 8, 5, 'urban', 'agent', False),
    'small_suburban_traffic_up': (3, 8, 8, 5, 'suburban', 'traffic', False),
    'case07_device_config': None,                                                    # golden case07's per-device overrides
}


def _state(env):
    import torch
    t = env._t
    torch.cuda.synchronize()
    pos = np.stack([t['pos_x'].cpu().numpy(), t['pos_y'].cpu().numpy()], axis=-1).astype(np.float64)
    return pos, t['rb'].cpu().numpy().astype(np.int64), t['pwr'].cpu().numpy().astype(np.int64)


def counterfactual(pos, link_tx, link_rx, rb, pwr, cols, spec, num_rbs, links=None):
    """sinr_db[b, i, r] of the oracle's step in the env where link i of env b alone moved to RB r: ONE oracle call on
    B0 * N * R envs.  pos [B0, D, 2], rb / pwr [B0, N].  links: the links i to do it for (None: all); the result is then
    [B0, len(links), R] - at 2048 links the oracle's [envs, N, N] pair arrays allow a few dozen envs, not B0 * N * R."""
    pos = np.asarray(pos, dtype=np.float64)
    rb = np.asarray(rb, dtype=np.int64); pwr = np.asarray(pwr, dtype=np.int64)
    b0, n = rb.shape
    r = int(num_rbs)
    idx = np.arange(n) if links is None else np.asarray(links, dtype=np.int64)
    k = len(idx)
    big_rb = np.broadcast_to(rb[:, None, None, :], (b0, k, r, n)).copy()
    big_rb[:, np.arange(k), :, idx] = np.arange(r)[None, None, :]         # env (b, i, r): link i sits on RB r
    big_pwr = np.broadcast_to(pwr[:, None, None, :], (b0, k, r, n)).reshape(b0 * k * r, n)
    big_pos = np.broadcast_to(pos[:, None, None], (b0, k, r) + pos.shape[1:]).reshape((b0 * k * r,) + pos.shape[1:])
    res = orc.step(big_pos, link_tx, link_rx, big_rb.reshape(b0 * k * r, n), big_pwr, cols, spec)
    sinr = res['sinr_db'].reshape(b0, k, r, n)
    return sinr[:, np.arange(k), :, idx].transpose(1, 0, 2)               # [b0, k, r]: entry i of env (b, i, r)


def interference_mw(pos, link_tx, link_rx, rb, pwr, cols, spec, num_rbs):
    """I[b, i, r] in mW, fp64, from orc.pair_path_loss_db (pl[b, j, i]: tx of link j -> rx of link i) and the device columns."""
    pos = np.asarray(pos, dtype=np.float64)
    rb = np.asarray(rb, dtype=np.int64)
    b0, n = rb.shape
    pl = orc.pair_path_loss_db(spec, pos, np.asarray(link_tx), np.asarray(link_rx), cols)        # [b, j, i]
    eirp = np.asarray(pwr, dtype=np.float64) + cols.eirp_off_db[np.asarray(link_tx)][None, :]   # [b, j]
    with np.errstate(over='ignore', invalid='ignore'):
        mw = orc.db_to_linear(eirp[:, :, None] - pl)                       # [b, j, i]
    mw[:, np.arange(n), np.arange(n)] = 0.0                                # j != i
    onehot = (rb[:, :, None] == np.arange(int(num_rbs))[None, None, :]).astype(np.float64)   # [b, j, r]
    return np.einsum('bji,bjr->bir', mw, onehot)


def sinr_from_interference(pos, link_tx, link_rx, pwr, cols, spec, ix_mw):
    """sinr_db[b, i, r] = sig_i - dB(I + lin(noise_i)), the definition written out in fp64."""
    pos = np.asarray(pos, dtype=np.float64)
    link_tx, link_rx = np.asarray(link_tx), np.asarray(link_rx)
    n = len(link_tx)
    pl = orc.pair_path_loss_db(spec, pos, link_tx, link_rx, cols)
    eirp = np.asarray(pwr, dtype=np.float64) + cols.eirp_off_db[link_tx][None, :]
    sig = eirp - pl[:, np.arange(n), np.arange(n)] + cols.rx_off_db[link_rx][None, :]
    noise = cols.noise_dbm[link_rx]
    return sig[:, :, None] - orc.linear_to_db(ix_mw + orc.db_to_linear(noise)[None, :, None])


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
                sinr_db=z['sinr_db'], step_sinr_db=z['step_sinr_db'], cols=cols, spec=spec)

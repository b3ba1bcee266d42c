"""The spatial channel of include/d2d_channel.h restated in float64 NumPy - the yardstick of test_gpu_channel.py, checked on its own by
test_channel_cpu.py.  Written from the header: Philox4x32-10 is the oracle's (oracle/d2d_oracle.py), the median is the oracle's own
path-loss formula, everything else is restated here."""
import math

import numpy as np

from oracle import d2d_oracle as orc

SHADOW_SEED_MIX = 0x736861646F77696E
FADING_SEED_MIX = 0x666164696E676368
_U64 = 2 ** 64 - 1
FADING = {None: 0, 'rayleigh': 1, 'rician': 2}


def stream_seeds(env_seed, seed=None):
    base = int(seed) if seed is not None else int(env_seed)
    return (base ^ SHADOW_SEED_MIX) & _U64, (base ^ FADING_SEED_MIX) & _U64


def constants(shadow_std_dB=8.0, decorrelation_m=20.0, num_sinusoids=16, fading='rayleigh', rician_k_dB=6.0):
    """(M_s or 0, shadow_amp_db, wave_scale, fading id, mu, s): formed in double, the float32 ones rounded once."""
    k = 10.0 ** (rician_k_dB / 10.0)
    return (num_sinusoids if shadow_std_dB > 0 else 0, float(np.float32(shadow_std_dB * math.sqrt(2.0 / num_sinusoids))),
            1.0 / (2.0 * math.pi * decorrelation_m), FADING[fading], float(np.float32(math.sqrt(k / (k + 1.0)))),
            float(np.float32(math.sqrt(1.0 / (2.0 * (k + 1.0))))))


def _philox(c0, c1, c2, c3, seed):
    return orc.philox4x32_10(c0, c1, c2, c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def _col(x, num_envs):
    """A scalar or a per-env [B] array of clock values as uint64 [B, 1]."""
    return np.broadcast_to(np.asarray(x, dtype=np.uint64), (num_envs,)).reshape(num_envs, 1)


def wave_vectors(shadow_seed, first_env, episode, num_envs, num_sinusoids, decorrelation_m):
    """(k_tx [B, M, 2], k_rx [B, M, 2] in rad / m, phi [B, M]) of episode `episode` (a scalar or [B])."""
    g = (np.arange(num_envs, dtype=np.uint64) + np.uint64(first_env))[:, None]
    e, m = _col(episode, num_envs), np.arange(num_sinusoids, dtype=np.uint64)[None, :]
    ks = []
    for side in (0, 1):
        w = _philox(g, e, m, np.uint64(side), shadow_seed)
        u = ((w[0] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
        theta = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
        k = np.sqrt(1.0 / (1.0 - u) ** 2 - 1.0) / decorrelation_m
        ks.append(np.stack([k * np.cos(2 * np.pi * theta), k * np.sin(2 * np.pi * theta)], axis=-1))
    phi = (_philox(g, e, m, np.uint64(2), shadow_seed)[0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return ks[0], ks[1], phi


def shadow_db(p_tx, p_rx, k_tx, k_rx, phi, shadow_std_dB):
    """S [B, J, I] for transmitter positions p_tx [B, J, 2] and receiver positions p_rx [B, I, 2]."""
    m = phi.shape[1]
    alpha = np.einsum('bmc,bjc->bjm', k_tx, p_tx) + 2 * np.pi * phi[:, None, :]
    beta = np.einsum('bmc,bic->bim', k_rx, p_rx)
    amp = float(np.float32(shadow_std_dB * math.sqrt(2.0 / m)))
    return amp * np.cos(alpha[:, :, None, :] + beta[:, None, :, :]).sum(axis=-1)


def fading_h2(fading_seed, first_env, episode, t, num_envs, dev_tx, dev_rx, fading, rician_k_dB=6.0):
    """|h|^2 [B, J, I] of the device pairs (dev_tx[j], dev_rx[i]) at the clock (episode, t), each a scalar or [B]."""
    g = (np.arange(num_envs, dtype=np.uint64) + np.uint64(first_env))[:, None, None]
    e, tt = _col(episode, num_envs)[:, :, None], _col(t, num_envs)[:, :, None]
    pair = (np.asarray(dev_tx, dtype=np.uint64)[None, :, None] | (np.asarray(dev_rx, dtype=np.uint64)[None, None, :] << np.uint64(16)))
    w = _philox(g, tt, pair, e, fading_seed)
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u2 = (w[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    if fading == 'rayleigh':
        return -np.log(u1)
    assert fading == 'rician'
    _, _, _, _, mu, s = constants(fading='rician', rician_k_dB=rician_k_dB)
    r = np.sqrt(-2.0 * np.log(u1))
    return mu * mu + 2.0 * mu * s * r * np.cos(2 * np.pi * u2) + s * s * r * r


def table_db(pos, link_tx, link_rx, cols, spec, *, env_seed, first_env, episode, t, seed=None, shadow_std_dB=8.0, decorrelation_m=20.0,
             num_sinusoids=16, fading='rayleigh', rician_k_dB=6.0):
    """(table [B, N+1, N] float64 dB, |h|^2 [B, N, N] or None): the header's d2d_channel_fill for positions pos [B, D, 2] (the
    float32 planes' values), the median by the oracle's path_loss_db under `spec`; episode and t scalars or per env [B]."""
    pos = np.asarray(pos, dtype=np.float64)
    b = pos.shape[0]
    link_tx, link_rx = np.asarray(link_tx), np.asarray(link_rx)
    shadow_seed, fading_seed = stream_seeds(env_seed, seed)
    with np.errstate(divide='ignore'):
        pl = orc.pair_path_loss_db(spec, pos, link_tx, link_rx, cols)
    if shadow_std_dB > 0:
        k_tx, k_rx, phi = wave_vectors(shadow_seed, first_env, episode, b, num_sinusoids, decorrelation_m)
        pl = pl + shadow_db(pos[:, link_tx], pos[:, link_rx], k_tx, k_rx, phi, shadow_std_dB)
    h2 = None
    if fading is not None:
        h2 = fading_h2(fading_seed, first_env, episode, t, b, link_tx, link_rx, fading, rician_k_dB)
        pl = pl - 10.0 * np.log10(h2)
    n = len(link_tx)
    return np.concatenate([pl, pl[:, np.arange(n), np.arange(n)][:, None, :]], axis=1), h2


def scatter_to_devices(table, link_tx, link_rx, num_dev):
    """The link table's rows 0 .. N-1 as [B, D, D] by (tx device, rx device): well defined because the channel is keyed by device
    pair (two links with the same devices hold the same entry)."""
    b, n = table.shape[0], len(link_tx)
    out = np.full((b, num_dev, num_dev), np.nan)
    out[:, np.asarray(link_tx)[:, None], np.asarray(link_rx)[None, :]] = table[:, :n]
    return out

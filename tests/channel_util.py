"""The spatial channel of include/d2d_channel.h restated in float64 NumPy - the yardstick of test_gpu_channel.py and
test_gpu_channel_large.py, checked on its own by test_channel_cpu.py.  Written from the header: Philox4x32-10 is the oracle's (oracle/d2d_oracle.py), the median is the oracle's own
path-loss formula, everything else is restated here."""
import math

import numpy as np

from oracle import d2d_oracle as orc

SHADOW_SEED_MIX = 0x736861646F77696E
FADING_SEED_MIX = 0x666164696E676368
_U64 = 2 ** 64 - 1
FADING = {None: 0, 'rayleigh': 1, 'rician': 2}
TOL = 1e-5                      # the project's parity bar
DEEP_FADE = 1e-4                # entries whose restated |h|^2 is below this are left out ...
DEEP_FADE_CAP = 1e-3            # ... and may be this fraction of the entries at most (Exp(1) puts 1e-4 there)


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


def table_db_columns(pos, link_tx, link_rx, a_tx_db, a_rx_db, exponent, *, shadow_seed, fading_seed, first_env, episode, t,
                     shadow_std_dB=8.0, decorrelation_m=20.0, num_sinusoids=16, fading='rayleigh', rician_k_dB=6.0, chunk_elems=1 << 21):
    """(table [B, N+1, N] float64 dB, |h|^2 [B, N, N] or None): the header's d2d_channel_fill, literally, for ANY device index lists
    and per-DEVICE columns: M(u, v) = a_tx_db[u] + a_rx_db[v] + 10 exponent[u] log10 |p_u - p_v| with u = link_tx[j], v = link_rx[i],
    plus shadow_db and fading_h2 under the raw seeds.  pos [B, D, 2] (the float32 planes' values); episode and t scalars or per env
    [B]; num_sinusoids 0 or shadow_std_dB 0: no shadowing.  Evaluated in chunks of transmitter rows of about chunk_elems
    [B, rows, N, M_s] values each, so that 2048 links stay within a few hundred MB of temporaries."""
    pos = np.asarray(pos, dtype=np.float64)
    b = pos.shape[0]
    link_tx, link_rx = np.asarray(link_tx, dtype=np.int64), np.asarray(link_rx, dtype=np.int64)
    a_tx_db, a_rx_db, exponent = (np.asarray(c, dtype=np.float64) for c in (a_tx_db, a_rx_db, exponent))
    n = len(link_tx)
    shadowed = num_sinusoids > 0 and shadow_std_dB > 0
    if shadowed:
        k_tx, k_rx, phi = wave_vectors(shadow_seed, first_env, episode, b, num_sinusoids, decorrelation_m)
    p_rx = pos[:, link_rx]
    table = np.empty((b, n + 1, n))
    h2 = np.empty((b, n, n)) if fading is not None else None
    rows = max(1, chunk_elems // (b * n * max(num_sinusoids, 1)))
    for j0 in range(0, n, rows):
        j1 = min(j0 + rows, n)
        tx = link_tx[j0:j1]
        p_tx = pos[:, tx]
        dx = p_tx[:, :, None, 0] - p_rx[:, None, :, 0]
        dy = p_tx[:, :, None, 1] - p_rx[:, None, :, 1]
        with np.errstate(divide='ignore'):
            pl = a_tx_db[tx][None, :, None] + a_rx_db[link_rx][None, None, :] \
                + 10.0 * exponent[tx][None, :, None] * np.log10(np.sqrt(dx * dx + dy * dy))
        if shadowed:
            pl += shadow_db(p_tx, p_rx, k_tx, k_rx, phi, shadow_std_dB)
        if fading is not None:
            h2[:, j0:j1] = fading_h2(fading_seed, first_env, episode, t, b, tx, link_rx, fading, rician_k_dB)
            pl -= 10.0 * np.log10(h2[:, j0:j1])
        table[:, j0:j1] = pl
    table[:, n] = table[:, np.arange(n), np.arange(n)]
    return table, h2


def entry_error(got, want, h2, also_left_out=None):
    """Worst |got - want| / |want| over the entries that are not deep fades; the share of entries left out.  also_left_out: a mask
    [B, N+1, N] of entries the caller has compared by other means (a restated -inf)."""
    keep = np.ones(want.shape, dtype=bool)
    if h2 is not None:
        n = h2.shape[1]
        keep[:, :n] = h2 >= DEEP_FADE
        keep[:, n] = h2[:, np.arange(n), np.arange(n)] >= DEEP_FADE
    if also_left_out is not None:
        keep &= ~also_left_out
    assert np.isfinite(want[keep]).all()
    with np.errstate(invalid='ignore'):                              # -inf - -inf of an entry that is left out
        diff = np.abs(got - want)
    return float(np.max(diff[keep] / np.abs(want)[keep])), 1.0 - keep.mean()


def scatter_to_devices(table, link_tx, link_rx, num_dev):
    """The link table's rows 0 .. N-1 as [B, D, D] by (tx device, rx device): well defined because the channel is keyed by device
    pair (two links with the same devices hold the same entry)."""
    b, n = table.shape[0], len(link_tx)
    out = np.full((b, num_dev, num_dev), np.nan)
    out[:, np.asarray(link_tx)[:, None], np.asarray(link_rx)[None, :]] = table[:, :n]
    return out

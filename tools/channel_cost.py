#!/usr/bin/env python3
"""Cost of SpatialChannelPathLoss (csrc/d2d_channel.hip) on the GPU; one JSON line per configuration, appended to
profiles/channel_cost.jsonl with --record.

    python tools/channel_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--record]
    python tools/channel_cost.py --kernel-stats DIR/..._kernel_stats.csv --configs stress [--record]

stress: 4096 envs x 512 links x 256 RBs; config2: BASELINE config 2, 1024 x 50 links x 25 RBs.  num_sinusoids 16, Rayleigh.  In one
process, per configuration:

  fill_us        d2d_channel_fill (both launches) between two device events, median of K after W warm-up calls - for the default
                 float64 entries and for table_dtype='float32'
  table_bytes    (N + 1) N B entries of 8 or 4 bytes; store_ceiling_fraction = table_bytes / fill_us over the store-only ceiling the sensing and graph
                 costs are held against (6.69 TB/s)
  step_us        step() of an env with the model (float64 and float32 entries), of the same env with the bare median, and of the same model written as a per-step
                 ArrayPathLoss in float32 torch (the route this replaces: median, the shadow as two batched matrix products of the
                 per-link cos / sin, Exp(1) fading from torch's own generator) - K steps between two synchronisations, wall clock,
                 the envs alternating, five rounds

The kernels' own times come from a run of ONE configuration under the profiler,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/channel_cost.py --configs stress`; --kernel-stats then
reads the channel kernels' rows of the *_kernel_stats.csv that run wrote and prints (records) them as kernel_ns.
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import ArrayPathLoss, LogDistancePathLoss, SpatialChannelPathLoss, pl_constant_dB

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}
STORE_CEILING_BPS = 6.69e12
SIGMA, DC, M = 8.0, 20.0, 16


class TorchChannel(ArrayPathLoss):
    """The same model as a user would write it today: float32 torch, evaluated before every step."""
    per_step = True

    def compute(self, view):
        xp = view.xp
        b = view.tx_x.shape[0]
        g = xp.Generator(device=view.tx_x.device); g.manual_seed(1)                # the waves: per env (an episode's worth)
        u = xp.rand((2, b, 1, M), generator=g, device=view.tx_x.device)
        th = 2 * math.pi * xp.rand((2, b, 1, M), generator=g, device=view.tx_x.device)
        k = xp.sqrt(1.0 / (1.0 - u) ** 2 - 1.0) / DC
        alpha = (k[0] * xp.cos(th[0])).double() * view.tx_x.double()[..., None] + (k[0] * xp.sin(th[0])).double() * view.tx_y.double()[..., None]
        beta = (k[1] * xp.cos(th[1])).double() * view.rx_x.double()[..., None] + (k[1] * xp.sin(th[1])).double() * view.rx_y.double()[..., None]
        ca, sa, cb, sb = (f(p).float() for p in (alpha, beta) for f in (xp.cos, xp.sin))
        shadow = SIGMA * math.sqrt(2.0 / M) * (ca @ cb.transpose(1, 2) - sa @ sb.transpose(1, 2))
        dx = view.tx_x[:, :, None] - view.rx_x[:, None, :]
        dy = view.tx_y[:, :, None] - view.rx_y[:, None, :]
        median = 10.0 * xp.log10(dx * dx + dy * dy) + pl_constant_dB(self.carrier_freq_GHz, 2.0)
        fade = -10.0 * xp.log10(-xp.log(1.0 - xp.rand_like(median)))
        return median + shadow + fade


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, iters, warmup):
    cfg, b = CONFIGS[name]
    f32 = type('SpatialChannelF32', (SpatialChannelPathLoss,), {'table_dtype': 'float32'})
    models = {'channel': SpatialChannelPathLoss, 'channel_f32': f32, 'median': LogDistancePathLoss, 'torch': TorchChannel}
    envs = {k: VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, path_loss_model=v), num_envs=b) for k, v in models.items()}
    for e in envs.values():
        e.reset(seed=1)
    actions = envs['channel'].action_buffer().clone()
    for e in envs.values():
        wall_us(e, actions, warmup)
    rounds = [{k: wall_us(e, actions, iters) for k, e in envs.items()} for _ in range(5)]
    step_us = {k: round(statistics.median(r[k] for r in rounds), 2) for k in envs}
    rec = {'config': name, 'envs': b, 'links': envs['channel'].num_links, 'num_sinusoids': M, 'fading': 'rayleigh', 'step_us': step_us,
           'channel_over_median_us': round(step_us['channel'] - step_us['median'], 2),
           'torch_over_channel': round(step_us['torch'] / step_us['channel'], 2)}
    for key, dtype in (('channel', 'float64'), ('channel_f32', 'float32')):
        table = envs[key].simulator.path_loss_table
        table.set_channel_clock(1, 0, 3)
        for _ in range(warmup):
            table.channel.fill()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, c in ev:
            a.record(); table.channel.fill(); c.record()
        torch.cuda.synchronize()
        t = [a.elapsed_time(c) * 1e3 for a, c in ev]
        med, nbytes = statistics.median(t), table.live.numel() * table.live.element_size()
        rec[dtype] = {'table_bytes': nbytes, 'fill_us': {'median': round(med, 2), 'min': round(min(t), 2), 'max': round(max(t), 2)},
                      'store_ceiling_fraction': round(nbytes / (med * 1e-6) / STORE_CEILING_BPS, 4)}
    for e in envs.values():
        e.close()
    return rec


def kernel_stats(path, name):
    """The channel kernels' rows of a rocprofv3 *_kernel_stats.csv, for the one configuration that run timed."""
    import csv
    cfg, b = CONFIGS[name]
    with open(path, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'channel_' in r['Name']]
    if not rows:
        raise SystemExit(f'{path}: no row names a channel kernel')
    out = {'config': name, 'envs': b, 'source': 'rocprofv3 --kernel-trace --stats', 'kernel_ns': {}}
    for r in rows:
        kind = 'phase' if 'channel_phase_kernel' in r['Name'] else 'fill'
        out['kernel_ns'][kind] = {'calls': int(r['Calls']), 'average': round(float(r['AverageNs']), 1), 'min': float(r['MinNs']),
                                  'max': float(r['MaxNs'])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--record', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    a = ap.parse_args()
    for name in a.configs.split(','):
        if a.kernel_stats:
            line = json.dumps(dict(tool='channel_cost', **kernel_stats(a.kernel_stats, name)))
        else:
            line = json.dumps(dict(tool='channel_cost', iters=a.iters, **run(name, a.iters, a.warmup)))
        print(line, flush=True)
        if a.record:
            with (ROOT / 'profiles' / 'channel_cost.jsonl').open('a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

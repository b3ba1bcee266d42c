#!/usr/bin/env python3
"""Cost of what-if evaluation on a path-loss table (VecD2DEnv.evaluate_table, csrc/d2d_evaltab.hip) on the GPU; one JSON line per
configuration and entry type, printed and appended to profiles/table_evaluate_cost.jsonl (--out).

    python tools/table_evaluate_cost.py [--iters K] [--warmup W] [--configs config2,stress] [--dtypes float64,float32] [--out FILE]

config2: BASELINE config 2, 1024 envs x 50 links x 25 RBs; stress: 4096 x 512 links x 256 RBs.  The channel env is a
SpatialChannelPathLoss (log-distance median, 8 dB shadowing) with fading=None.  In one process, per configuration and entry type of
the live table, device events, median of K after W warm-up calls, all legs timed ALTERNATELY (one call of each per round), at
K = 1, 4 and 16 candidates per env:

  evaluate_table_us   leg 1: one evaluate_table() launch on the channel env, with both planes and totals only (planes=())
  step_us             leg 2: K calls of step() on the same env - with fading=None and nothing moving no fill is launched, so this
                      is the step alone, reading the same table (and it moves the env)
  evaluate_us         leg 3: one evaluate() launch on the native env of the same shape (log-distance, the same exponent)
  equal               evaluate_table() of the env's own planes against the last step's planes, bit for bit

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/table_evaluate_cost.py --out ''`: the kernel
is evaltab_kernel<float | double> (libd2d_evaltab.so).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from gym_d2d_amd import _native
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss

CONFIGS = {
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
}
KS = (1, 4, 16)
PLE = 3.5


class Median(LogDistancePathLoss):
    def __init__(self, f):
        super().__init__(f, ple=PLE)


def channel_model(dtype):
    return type('Channel', (SpatialChannelPathLoss,), dict(median=LogDistancePathLoss, median_kwargs={'ple': PLE}, fading=None,
                                                           num_sinusoids=8, table_dtype=dtype))


def alternating_us(fns, iters, warmup):
    """Device-event timings of several callables, one call of each per round: [(median, min, max)] in us."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(iters)]
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        t = [row[k][0].elapsed_time(row[k][1]) * 1e3 for row in ev]
        out.append({'median': round(statistics.median(t), 2), 'min': round(min(t), 2), 'max': round(max(t), 2)})
    return out


def run(name, dtype, iters, warmup):
    cfg, b = CONFIGS[name]
    chan = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, path_loss_model=channel_model(dtype)), num_envs=b)
    native = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, path_loss_model=Median), num_envs=b)
    for env in (chan, native):
        env.reset(seed=1)
    actions = chan.action_buffer().clone()
    _, _, _, info = chan.step(actions)
    n, r = chan.num_links, chan.config.num_rbs
    rec = {'config': name, 'envs': b, 'links': n, 'rbs': r, 'table_dtype': dtype, 'chunk': _native.EVALTAB_CHUNK,
           'table_bytes': int(chan.simulator.path_loss_table.live.numel() * chan.simulator.path_loss_table.live.element_size())}
    own = chan.evaluate_table(chan._t['rb'].unsqueeze(1).contiguous(), chan._t['pwr'].unsqueeze(1).contiguous())
    rec['equal'] = {'sinr_db': bool(torch.equal(own['sinr_db'][:, 0], info['sinr_db'])),
                    'capacity_mbps': bool(torch.equal(own['capacity_mbps'][:, 0], info['capacity_mbps'])),
                    'domain': int(own['domain'].sum())}
    gen = torch.Generator(device=chan.device).manual_seed(3)
    labels, fns = [], []
    fills = _native.channel_launches
    for k in KS:
        rb = torch.randint(0, r, (b, k, n), generator=gen, device=chan.device, dtype=torch.int32)
        pwr = torch.randint(0, 20, (b, k, n), generator=gen, device=chan.device, dtype=torch.int32)
        labels += [f'evaluate_table_planes_k{k}', f'evaluate_table_totals_k{k}', f'step_x{k}', f'evaluate_planes_k{k}']
        fns += [lambda rb=rb, pwr=pwr: chan.evaluate_table(rb, pwr), lambda rb=rb, pwr=pwr: chan.evaluate_table(rb, pwr, planes=()),
                lambda k=k: [chan.step(actions) for _ in range(k)], lambda rb=rb, pwr=pwr: native.evaluate(rb, pwr)]
    times = dict(zip(labels, alternating_us(fns, iters, warmup)))
    rec['fills_while_timing'] = _native.channel_launches - fills          # 0: leg 2 is the step alone
    rec['evaluate_table_us'] = {k: v for k, v in times.items() if k.startswith('evaluate_table')}
    rec['step_us'] = {k: v for k, v in times.items() if k.startswith('step')}
    rec['evaluate_us'] = {k: v for k, v in times.items() if k.startswith('evaluate_planes')}
    rec['winner'] = {f'k{k}': min((times[f'evaluate_table_planes_k{k}']['median'], 'evaluate_table'), (times[f'step_x{k}']['median'], 'step'),
                                  (times[f'evaluate_planes_k{k}']['median'], 'evaluate'))[1] for k in KS}
    for env in (chan, native):
        env.close()
    del chan, native, own, info
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--configs', default='config2,stress')
    ap.add_argument('--dtypes', default='float64,float32')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'table_evaluate_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        for dtype in a.dtypes.split(','):
            line = json.dumps(dict(tool='table_evaluate_cost', iters=a.iters, **run(name, dtype, a.iters, a.warmup)))
            print(line, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()

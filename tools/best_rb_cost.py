#!/usr/bin/env python3
"""Cost of best-response RB selection (VecD2DEnv.best_rb, csrc/d2d_bestrb.hip) on the GPU; one JSON line per configuration, printed and
appended to profiles/best_rb_cost.jsonl (--out).

    python tools/best_rb_cost.py [--iters K] [--warmup W] [--configs stress,stress_hata,config2] [--no-baseline] [--out FILE]

stress: 4096 envs x 512 links x 256 RBs, 1/d^2; stress_hata: the same with COST-Hata urban (the pow-k law); config2: BASELINE
config 2, 1024 x 50 links x 25 RBs.  In one process, per configuration:

  best_rb_us     the launch alone, device events, median of K after W warm-up calls - timed ALTERNATELY with
  sense_us       sense('sinr_db') alone (the [B, N, R] block it no longer writes) and
  sense_max_us   the thing it replaces: sense('sinr_db'), torch max(-1) over the block, the own-column gather and the subtraction
  equal          best_rb() against that formulation: best_sinr_db and gain_db bit for bit; best_rb wherever torch's max reports the
                 first maximum (its tie order is not documented: the share of links where the two indices differ is reported, and
                 on each of them the two values are equal)
  step_us        step() with BestRbObsFunction against the obs-less step() (SignalPlanesObsFunction), lockstep and autoreset (K steps
                 between two synchronisations, wall clock, alternating)

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/best_rb_cost.py --no-baseline --out ''`: the
kernel is bestrb_kernel<law> (libd2d_bestrb.so).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from gym_d2d_amd.envs import BestRbObsFunction, VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss


class UrbanHata(CostHataPathLoss):
    def __init__(self, f):
        super().__init__(f, AreaType.URBAN)


CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'stress_hata': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256, 'path_loss_model': UrbanHata}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}


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


def sense_formulation(env):
    """best_rb() the way a user had to compute it before: the sensed block, torch's max over it, the own column."""
    def run():
        blk = env.sense('sinr_db')
        val, idx = blk.max(dim=-1)
        own = torch.gather(blk, 2, env._t['rb'].long().unsqueeze(-1)).squeeze(-1)
        return idx, val, val - own
    return run


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, iters, warmup, baseline):
    cfg, b = CONFIGS[name]
    rec = {'config': name, 'envs': b}
    step_us = {}
    for mode, kw in (('lockstep', {}), ('autoreset', {'autoreset': True})):
        base = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b, **kw)
        best = VecD2DEnv(dict(cfg, obs_fn=BestRbObsFunction), num_envs=b, **kw)
        base.reset(seed=1); best.reset(seed=1)
        actions = base.action_buffer().clone()
        for e in (base, best):
            wall_us(e, actions, warmup)
        pairs = [(wall_us(base, actions, iters), wall_us(best, actions, iters)) for _ in range(5)]
        step_us[mode] = {'obs_less': round(statistics.median(p[0] for p in pairs), 2),
                         'best_rb_obs': round(statistics.median(p[1] for p in pairs), 2),
                         'added': round(statistics.median(p[1] - p[0] for p in pairs), 2)}
        base.close(); best.close()
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    k = env._best_rb_kernel()
    rec.update(links=k.n, rbs=k.r, law=k.law, out_bytes=3 * b * k.n * 4, block_bytes=b * k.n * k.r * 4)
    fns = [lambda: env.best_rb()]
    if baseline:
        fn = sense_formulation(env)
        (ri, rv, rg), (gi, gv, gg) = fn(), env.best_rb()
        differ = ri != gi.long()
        blk = env.sense('sinr_db')
        at = lambda i: torch.gather(blk, 2, i.long().unsqueeze(-1)).squeeze(-1)
        rec['equal'] = {'best_sinr_db': bool(torch.equal(rv, gv)), 'gain_db': bool(torch.equal(rg, gg)),
                        'best_rb_differs_share': round(float(differ.float().mean()), 6),
                        'values_equal_where_it_differs': bool(torch.equal(at(ri)[differ], at(gi)[differ])),
                        'kernel_index_is_lower_where_it_differs': bool((gi.long()[differ] < ri[differ]).all())}
        del ri, rv, rg, blk
        fns += [lambda: env.sense('sinr_db'), fn]
    times = alternating_us(fns, iters, warmup)
    rec['best_rb_us'] = times[0]
    if baseline:
        rec['sense_us'], rec['sense_max_us'] = times[1], times[2]
        rec['sense_max_over_best_rb'] = round(times[2]['median'] / times[0]['median'], 2)
        rec['sense_over_best_rb'] = round(times[1]['median'] / times[0]['median'], 2)
    rec['step_us'] = step_us
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,stress_hata,config2')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'best_rb_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='best_rb_cost', iters=a.iters, **run(name, a.iters, a.warmup, not a.no_baseline)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Cost of sequential best-response dynamics (VecD2DEnv.best_response_dynamics, csrc/d2d_brdyn.hip) on the GPU; one JSON line per
configuration, printed and appended to profiles/best_response_dynamics_cost.jsonl (--out).

    python tools/best_response_dynamics_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--out FILE]

Per configuration (state: reset, then one step with the reset's random actions; min_gain_db --min-gain-db, max_rounds --max-rounds):
  rounds, moves    what the kernel did per env (mean, max), and the share of envs that converged
  kernel_us        the launch alone, device events, median of K after W warm-up calls - timed ALTERNATELY with
  best_rb_us       one best_rb() launch on the same state, and with
  api_turn_us      ONE turn of the loop through the public API (best_rb(), move one link where its gain is large enough, step()):
                   what today's API pays per link and round.  The turns walk the links in ascending index from the same start.
  api_loop_us      api_turn_us x links x (the kernel's largest round count + 1, the quiet round, capped at max_rounds): the whole
                   loop for the same rounds, as the product of the measured turn - the loop itself would run for seconds per sample
                   at the stress shape
  actions_us       best_response_dynamics_actions() end to end (mask look-up, launch, encode), host clock around K calls that end
                   in a device synchronise

Every GPU step of a measuring session runs under its own `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/best_response_dynamics_cost.py --configs stress && timeout -k 10 120 python tools/best_response_dynamics_cost.py --configs config2
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
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


def run(name, iters, warmup, min_gain_db, max_rounds):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    start = env.action_buffer().clone()
    env.step(start)
    res = env.best_response_dynamics(min_gain_db=min_gain_db, max_rounds=max_rounds)
    k = env._brdyn
    rounds, moves = res.rounds.float(), res.moves.float()
    rec = {'config': name, 'envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'min_gain_db': min_gain_db, 'max_rounds': max_rounds,
           'rounds': {'mean': round(float(rounds.mean()), 2), 'max': int(rounds.max())},
           'moves': {'mean': round(float(moves.mean()), 2), 'max': int(moves.max())},
           'converged': round(float(res.converged.float().mean()), 4)}
    p = env.num_pwr_actions
    levels = torch.as_tensor(np.asarray([p[env._cue_kind]] * env.num_cues + [p['due']] * env.num_due_pairs, dtype=np.int32), device=env.device)
    turn = [0]

    def api_turn():
        i = turn[0] % k.n
        turn[0] += 1
        best, _, gain = env.best_rb()
        rb = env._t['rb'].clone()
        rb[:, i] = torch.where(gain[:, i] > min_gain_db, best[:, i], rb[:, i])
        env.step((rb * levels + env._t['pwr']).to(torch.int32))

    def kernel():
        env.best_response_dynamics(min_gain_db=min_gain_db, max_rounds=max_rounds)
    # the kernel is timed on whatever state the turns have reached: a partly settled one, as inside a training loop
    times = alternating_us([kernel, env.best_rb, api_turn], iters, warmup)
    rec['kernel_us'], rec['best_rb_us'], rec['api_turn_us'] = times
    loop_rounds = min(max_rounds, rec['rounds']['max'] + 1)
    rec['api_loop_us'] = round(times[2]['median'] * k.n * loop_rounds, 1)
    rec['api_loop_over_kernel'] = round(rec['api_loop_us'] / times[0]['median'], 1)
    rec['kernel_over_best_rb'] = round(times[0]['median'] / times[1]['median'], 2)
    env.step(start)
    fresh = alternating_us([kernel, env.best_rb], iters, warmup)         # and from the random start itself, every call
    rec['kernel_from_random_us'], rec['best_rb_from_random_us'] = fresh
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            env.best_response_dynamics_actions(min_gain_db=min_gain_db, max_rounds=max_rounds)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / iters * 1e6)
    rec['actions_us'] = round(statistics.median(walls), 2)
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--min-gain-db', type=float, default=3.0)
    ap.add_argument('--max-rounds', type=int, default=16)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'best_response_dynamics_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='best_response_dynamics_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.min_gain_db, a.max_rounds)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Wall-clock cost of VecD2DEnv(autoreset=True) against the lockstep env, on the GPU; one JSON line.

    python tools/autoreset_cost.py [--steps K] [--warmup W] [--repeats R] [--configs planes,linear]

planes: 4096 envs x 512 links (256 RBs / 256 CUEs / 256 DUE pairs), SignalPlanesObsFunction, reward_per_env=True - the obs-less
learner setup.  linear: BASELINE config 2 (1024 envs x 25 / 25 / 25, LinearObs).  Both envs live in one process and are timed
alternately, R times each, K synchronised steps per timing with the same action tensor: ms per step for each, and the overhead
(autoreset minus lockstep) per repeat with its spread.  The autoreset env starts staggered (elapsed = b % 10), so about a tenth of
its envs reset on every step - the steady state of a rollout.  For the per-kernel view run it under
`rocprofv3 --kernel-trace --stats -- python tools/autoreset_cost.py --steps 20 --warmup 5 --repeats 1 --no-stagger`: the three
kernels are reset_masked_kernel (libd2d_hip.so), merge_kernel and advance_kernel (libd2d_episode.so); with --no-stagger every env
resets on the same step, one in eleven, so a kernel's minimum is its cost in a step where no env resets.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

CONFIGS = {
    'planes': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256, 'obs_fn': SignalPlanesObsFunction}, 4096,
               {'reward_per_env': True}),
    'linear': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024, {}),
}


def timed(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run(name, steps, warmup, repeats, stagger=True):
    cfg, b, kw = CONFIGS[name]
    lock = VecD2DEnv(dict(cfg), num_envs=b, **kw)
    auto = VecD2DEnv(dict(cfg), num_envs=b, autoreset=True, **kw)
    lock.reset(seed=1)
    auto.reset(seed=1, elapsed=np.arange(b) % 10 if stagger else None)
    actions = lock.action_buffer().clone()
    timed(lock, actions, warmup)
    timed(auto, actions, warmup)
    ms = {'lockstep': [], 'autoreset': []}
    for _ in range(repeats):
        ms['lockstep'].append(timed(lock, actions, steps))
        ms['autoreset'].append(timed(auto, actions, steps))
    over = [a - l for a, l in zip(ms['autoreset'], ms['lockstep'])]
    lock.close(); auto.close()
    return {'config': name, 'staggered': stagger, 'envs': b, 'links': cfg['num_cues'] + cfg['num_due_pairs'],
            'ms_per_step': {k: round(statistics.median(v), 4) for k, v in ms.items()},
            'overhead_ms': {'median': round(statistics.median(over), 4), 'min': round(min(over), 4), 'max': round(max(over), 4)},
            'runs_ms': {k: [round(x, 4) for x in v] for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--configs', default='planes,linear')
    ap.add_argument('--no-stagger', action='store_true', help='lockstep episodes: every env resets on every 11th step only')
    a = ap.parse_args()
    out = [run(name, a.steps, a.warmup, a.repeats, not a.no_stagger) for name in a.configs.split(',')]
    print(json.dumps({'tool': 'autoreset_cost', 'steps': a.steps, 'repeats': a.repeats, 'results': out}))


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of the queue-aware goodput ascent (VecD2DEnv.goodput_ascent, csrc/d2d_goodput.hip) on the GPU against what a user had
before it on the same state: one rb_ascent() plus one power_ascent() launch (which maximise capacity, not goodput, and move one
half of the action each), and the same goodput ascent as a host loop, one evaluate() launch and one round trip per link turn; one
JSON line per configuration, printed and appended to profiles/goodput_ascent_cost.jsonl (--out).

    python tools/goodput_ascent_cost.py [--iters K] [--warmup W] [--configs config2,stress] [--out FILE]

config2: BASELINE config 2, 1024 envs x (25 + 25) links x 25 RBs; stress: 4096 envs x (256 + 256) links x 256 RBs, 1/d^2.  No floors,
no allowed mask, every link movable, min_gain_bits 0, max_rounds 16, weight 1, bits_per_mbps 1000, and a seeded demand plane of 0 ..
8000 bits per link (a quarter of the links hold nothing).  In one process, per configuration:

  goodput_us        one goodput_ascent() launch: every turn of every round of every env.  Device events, median of K after W
                    warm-up calls, timed ALTERNATELY with the two legs below (one call of each per round)
  rb_ascent_us      one rb_ascent(max_rounds=16) launch on the same state
  power_ascent_us   one power_ascent(max_rounds=16) launch on the same state
  host_loop_us      the whole host loop (tests/goodput_ascent_util.goodput_by_evaluate: the statement, stated once), ONE run, wall
                    clock, on a SUBSET of the envs, host_envs, under the round cap host_loop_max_rounds (2 at the stress shape,
                    where a round of 512 turns takes the host a minute: its figure is a LOWER bound on the loop the launch
                    replaces); its nine outputs must equal a launch's on those envs under the same cap (host_loop_equal).
                    host_loop_scaled_us is host_loop_us x envs / host_envs, a linear scaling stated as such

The stress configuration is timed on its first 256 envs first (subset_us, the median of 5 calls).  The full batch is timed only if
that extrapolates - times envs / 256, the pessimistic linear scaling - to a launch of at most --full-limit-s seconds (default 6);
otherwise the legs above are timed on the subset and the line says so (full_batch: false).  --subset-only stops behind the five
calls: the line then holds subset_us and 'not measured' for every median of 50.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
sys.path.insert(0, str(ROOT / 'tests'))
import numpy as np
import torch

from assign_cost import CONFIGS, alternating_us
from goodput_ascent_util import goodput_by_evaluate
from gym_d2d_amd import goodput_ascent
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

HOST_ENVS = {'stress': 2, 'config2': 64}
HOST_ROUNDS = {'stress': 2, 'config2': 16}      # the host loop's round cap: the large shape takes a minute per round
SUBSET = 256
MAX_ROUNDS, BPM = 16, 1000.0


def make_env(cfg, b):
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    return env


def demand_plane(b, n):
    rng = np.random.default_rng(5)
    return np.where(rng.random((b, n)) < 0.25, 0, rng.integers(1, 8001, (b, n))).astype(np.int32)


def run(name, iters, warmup, full_limit_s, subset_only=False):
    cfg, b = CONFIGS[name]
    demand_all = demand_plane(b, cfg['num_cues'] + cfg['num_due_pairs'])
    rec = {'config': name, 'envs': b, 'max_rounds': MAX_ROUNDS, 'bits_per_mbps': BPM}
    if b > SUBSET and name != 'config2':                                # the subset first: is the full batch worth a launch?
        env = make_env(cfg, SUBSET)
        dem = torch.as_tensor(demand_all[:SUBSET], device=env.device)
        sub = alternating_us([lambda: env.goodput_ascent(dem, None, BPM, max_rounds=MAX_ROUNDS)], 5, 1)[0]
        print(f'{name}: {SUBSET} envs, one launch {sub}', file=sys.stderr, flush=True)
        res = env.goodput_ascent(dem, None, BPM, max_rounds=MAX_ROUNDS)
        sub_stats = {'rounds_mean': round(float(res.rounds.float().mean()), 2), 'moves_mean': round(float(res.moves.float().mean()), 2),
                     'converged': int(res.converged.sum())}
        env.close()
        rec['subset_envs'], rec['subset_us'] = SUBSET, sub
        rec['full_extrapolated_s'] = round(sub['median'] * b / SUBSET / 1e6, 2)
        rec['full_batch'] = rec['full_extrapolated_s'] <= full_limit_s
        if subset_only:                                                 # the five-call subset figure alone: the median of 50 is not measured
            rec.update(sub_stats, subset_only=True, goodput_us='not measured', rb_ascent_us='not measured', power_ascent_us='not measured',
                       host_loop_us='not measured')
            return rec
        if not rec['full_batch']:
            b = SUBSET
    env = make_env(cfg, b)
    demand = torch.as_tensor(demand_all[:b], device=env.device)
    res = env.goodput_ascent(demand, None, BPM, max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy().copy() for t in res)
    k = env._goodput
    rec.update({'timed_envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'lds_bytes': goodput_ascent.lds_bytes(k.n, k.r),
                'rounds': {'mean': round(float(got[6].mean()), 2), 'max': int(got[6].max())},
                'moves': {'mean': round(float(got[7].mean()), 2), 'max': int(got[7].max())}, 'converged': int(got[8].sum())})
    fns = [lambda: env.goodput_ascent(demand, None, BPM, max_rounds=MAX_ROUNDS), lambda: env.rb_ascent(max_rounds=MAX_ROUNDS),
           lambda: env.power_ascent(max_rounds=MAX_ROUNDS)]
    times = alternating_us(fns, iters, warmup)
    rec['goodput_us'], rec['rb_ascent_us'], rec['power_ascent_us'] = times
    rec['goodput_over_rb_plus_power'] = round(times[0]['median'] / (times[1]['median'] + times[2]['median']), 2)
    # the host loop: one run, wall clock, on the first host_envs envs (the same seeds give the same first envs)
    hb = HOST_ENVS[name]
    small = make_env(cfg, hb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want, calls = goodput_by_evaluate(small, demand_all[:hb], None, BPM, max_rounds=HOST_ROUNDS[name])
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    same = small.goodput_ascent(torch.as_tensor(demand_all[:hb], device=small.device), None, BPM, max_rounds=HOST_ROUNDS[name])
    torch.cuda.synchronize()
    rec['host_envs'], rec['host_loop_max_rounds'], rec['host_loop_evaluate_calls'] = hb, HOST_ROUNDS[name], calls
    rec['host_loop_us'] = round(host_us, 1)
    rec['host_loop_equal'] = bool(all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(same, want)))
    rec['host_loop_scaled_us'] = round(host_us * b / hb, 1)
    rec['host_loop_over_goodput'] = round(rec['host_loop_scaled_us'] / times[0]['median'], 1)
    rec['host_loop_over_goodput_unscaled'] = round(host_us / times[0]['median'], 1)
    small.close()
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', default='config2,stress')
    ap.add_argument('--full-limit-s', type=float, default=6.0)
    ap.add_argument('--subset-only', action='store_true', help='a configuration past 256 envs: time its first 256 envs, 5 calls, and stop')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'goodput_ascent_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='goodput_ascent_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.full_limit_s, a.subset_only)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of the sum-capacity power ascent (VecD2DEnv.power_ascent, csrc/d2d_ascent.hip) on the GPU against what the env offered before
it: the same ascent as a host loop, one evaluate() launch and one round trip per link turn; one JSON line per configuration, printed
and appended to profiles/ascent_cost.jsonl (--out).

    python tools/ascent_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--out FILE]

stress: 4096 envs x (256 + 256) links x 256 RBs, 1/d^2; config2: BASELINE config 2, 1024 x (25 + 25) links x 25 RBs.  No floors,
every link adjustable, start 'held', min_gain_mbps 0, max_rounds 16.  In one process, per configuration:

  ascent_us         one power_ascent() launch: every turn of every round of every env.  Device events, median of K after W warm-up
                    calls, timed ALTERNATELY with evaluate_us (one call of each per round)
  evaluate_us       one evaluate() launch with K = 24 candidates per env: the device side of ONE link turn of the host loop
  host_loop_us      the whole host loop, ONE run, wall clock (it is host time by nature: per turn the candidate planes are made,
                    evaluate() is launched, the capacity plane is copied back and the choice is made in NumPy for every env at
                    once).  Run on host_envs envs - all of them at config2, the first 256 of the stress configuration - and its
                    powers, rounds and moves must equal the launch's on those envs (host_loop_equal).  host_loop_scaled_us is
                    host_loop_us x envs / host_envs, a linear scaling stated as such: the launches of the loop grow less than
                    linearly in the envs, the copies and the host arithmetic linearly

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/ascent_cost.py --out ''`: the kernels are
ascent_kernel<law> (libd2d_ascent.so) and evaluate_kernel<law> (libd2d_evaluate.so).
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
import numpy as np
import torch

from assign_cost import CONFIGS, alternating_us
from gym_d2d_amd import power_ascent
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

HOST_ENVS = {'stress': 256, 'config2': 1024}
MAX_ROUNDS = 16


def host_loop(env, max_rounds=MAX_ROUNDS):
    """include/d2d_ascent.h's statement over evaluate(), without floors, every env taking link i's turn in one call; returns
    (power_dbm, rounds, moves, evaluate calls)."""
    b, n, r = env.num_envs, env.num_links, env._ascent.r
    rb_dev = env._t['rb']
    rb = rb_dev.cpu().numpy()
    p = env._t['pwr'].cpu().numpy().astype(np.int32)
    p_min, p_max = env._ascent.p_min.cpu().numpy(), env._ascent.p_max.cpu().numpy()
    on = (rb >= 0) & (rb < r)
    rounds, moves, live, calls = np.zeros(b, np.int32), np.zeros(b, np.int32), np.ones(b, bool), 0
    rows = np.arange(b)
    for _ in range(max_rounds):
        moved = np.zeros(b, bool)
        for i in range(n):
            turn = live & on[:, i]
            if not turn.any():
                continue
            levels = np.arange(p_min[i], p_max[i] + 1, dtype=np.int32)
            cand = torch.as_tensor(p, device=env.device)[:, None, :].repeat(1, len(levels), 1)
            cand[:, :, i] = torch.as_tensor(levels, device=env.device)[None, :]
            cap = env.evaluate(rb_dev[:, None, :].expand(b, len(levels), n).contiguous(), cand, planes=('capacity_mbps',))['capacity_mbps']
            calls += 1
            cap = cap.cpu().numpy().astype(np.float64)
            members = on & (rb == rb[:, i:i + 1])
            total = np.add.accumulate(np.where(members[:, None, :], cap, 0.0), axis=2)[:, :, -1]      # in link order; x + 0.0 is x
            best = np.argmax(total, axis=1)                                                          # the lowest level at the maximum
            cur = p[:, i] - p_min[i]
            go = turn & (total[rows, best] - total[rows, cur] > 0.0)
            p[go, i] = levels[best[go]]
            moved |= go
            moves += go
        rounds[live & moved] += 1
        live &= moved
        if not live.any():
            break
    return p, rounds, moves, calls


def make_env(cfg, b):
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    return env


def run(name, iters, warmup):
    cfg, b = CONFIGS[name]
    env = make_env(cfg, b)
    res = env.power_ascent(max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    k = env._ascent
    rounds, moves, conv = res.rounds.cpu().numpy(), res.moves.cpu().numpy(), res.converged.cpu().numpy()
    power = res.power_dbm.cpu().numpy()
    rec = {'config': name, 'envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'max_rounds': MAX_ROUNDS,
           'lds_bytes': power_ascent.lds_bytes(k.n, k.r, k.law != 0),
           'rounds': {'mean': round(float(rounds.mean()), 2), 'max': int(rounds.max())},
           'moves': {'mean': round(float(moves.mean()), 2), 'max': int(moves.max())}, 'converged': int(conv.sum())}
    levels = int((k.p_max - k.p_min).max()) + 1
    rb_c = env._t['rb'][:, None, :].expand(b, levels, k.n).contiguous()
    pw_c = env._t['pwr'][:, None, :].expand(b, levels, k.n).contiguous()
    labels = ['ascent', 'evaluate']
    fns = [lambda: env.power_ascent(max_rounds=MAX_ROUNDS), lambda: env.evaluate(rb_c, pw_c)]
    times = dict(zip(labels, alternating_us(fns, iters, warmup)))
    rec['ascent_us'], rec['evaluate_us'], rec['evaluate_candidates'] = times['ascent'], times['evaluate'], levels
    # the host loop: one run, wall clock, on host_envs envs (the same seeds give the same first envs)
    hb = HOST_ENVS[name]
    small = env if hb == b else make_env(cfg, hb)
    if small is not env:
        small.power_ascent(max_rounds=MAX_ROUNDS)                         # opens the kernel object host_loop reads the bounds from
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hp, hr, hm, calls = host_loop(small)
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    rec['host_envs'], rec['host_loop_evaluate_calls'], rec['host_loop_us'] = hb, calls, round(host_us, 1)
    rec['host_loop_equal'] = bool(np.array_equal(hp, power[:hb]) and np.array_equal(hr, rounds[:hb]) and np.array_equal(hm, moves[:hb]))
    rec['host_loop_scaled_us'] = round(host_us * b / hb, 1)
    rec['host_loop_scaled'] = hb != b
    rec['host_loop_over_ascent'] = round(rec['host_loop_scaled_us'] / times['ascent']['median'], 1)
    if small is not env:
        small.close()
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'ascent_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='ascent_cost', iters=a.iters, **run(name, a.iters, a.warmup)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

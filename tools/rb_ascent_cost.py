#!/usr/bin/env python3
"""Cost of the sum-capacity RB ascent (VecD2DEnv.rb_ascent, csrc/d2d_rbascent.hip) on the GPU against best_response_dynamics(), the
selfish dynamics of the same shape, and against what the env offered before it: the same ascent as a host loop, one evaluate()
launch and one round trip per link turn; one JSON line per configuration, printed and appended to profiles/rb_ascent_cost.jsonl
(--out).

    python tools/rb_ascent_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--out FILE]

stress: 4096 envs x (256 + 256) links x 256 RBs, 1/d^2; config2: BASELINE config 2, 1024 x (25 + 25) links x 25 RBs.  No floors, no
allowed mask, every link movable, min_gain_mbps 0, max_rounds 16.  In one process, per configuration:

  rb_ascent_us      one rb_ascent() launch: every turn of every round of every env.  Device events, median of K after W warm-up
                    calls, timed ALTERNATELY with brdyn_us (one call of each per round)
  brdyn_us          one best_response_dynamics(min_gain_db=3, max_rounds=16) launch on the same state
  host_loop_us      the whole host loop, ONE run, wall clock (it is host time by nature: per turn the R candidate planes are made,
                    evaluate() is launched, the capacity plane is copied back and the choice is made in NumPy for every env at
                    once).  Run on a SUBSET of the envs, host_envs - the first 8 of the stress configuration, whose candidate
                    planes are R = 256 per env and turn, the first 256 of config2 - and its RBs, rounds and moves must equal the
                    launch's on those envs (host_loop_equal).  host_loop_scaled_us is host_loop_us x envs / host_envs, a linear
                    scaling stated as such: the launches of the loop grow less than linearly in the envs, the copies and the host
                    arithmetic linearly
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
from gym_d2d_amd import rb_ascent
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

HOST_ENVS = {'stress': 8, 'config2': 256}
MAX_ROUNDS = 16


def seq_sum(a):
    """The double sum along the last axis in index order; x + 0.0 is x."""
    return np.add.accumulate(a, axis=-1)[..., -1]


def host_loop(env, max_rounds=MAX_ROUNDS):
    """include/d2d_rbascent.h's statement over evaluate(), without floors or mask, every env taking link i's turn in one call;
    returns (rb, rounds, moves, evaluate calls)."""
    b, n, r = env.num_envs, env.num_links, int(env.simulator.config.num_rbs)
    rb = env._t['rb'].cpu().numpy().astype(np.int64)
    pwr = env._t['pwr'][:, None, :].expand(b, r, n).contiguous()
    on = (rb >= 0) & (rb < r)
    rounds, moves, live, calls = np.zeros(b, np.int32), np.zeros(b, np.int32), np.ones(b, bool), 0
    rows, rbs = np.arange(b), np.arange(r)
    for _ in range(max_rounds):
        moved = np.zeros(b, bool)
        for i in range(n):
            turn = live & on[:, i]
            if not turn.any() or r < 2:
                continue
            cand = np.repeat(rb[:, None, :], r, axis=1)
            cand[:, :, i] = rbs[None, :]
            cap = env.evaluate(torch.as_tensor(cand.astype(np.int32), device=env.device), pwr, planes=('capacity_mbps',))['capacity_mbps']
            calls += 1
            cap = cap.cpu().numpy().astype(np.float64)                   # [b, candidate r, link]
            c = np.where(on[:, i], rb[:, i], 0)
            m = rb[:, None, :] == rbs[None, :, None]                     # group(r) \ {i}
            m[:, :, i] = False
            w = m.copy()
            w[:, :, i] = True                                            # group(r) u {i}
            with_ = seq_sum(np.where(w, cap, 0.0))
            without = seq_sum(np.where(m, cap[rows, c][:, None, :], 0.0))
            without[rows, c] = seq_sum(np.where(m[rows, c], cap[rows, np.where(c != 0, 0, 1)], 0.0))
            d = with_ - without
            ok = (rbs[None, :] != c[:, None]) & ~np.isnan(d)
            best = np.argmax(np.where(ok, d, -np.inf), axis=1)           # the lowest RB at the maximum
            go = turn & ok[rows, best] & (d[rows, best] - d[rows, c] > 0.0)
            rb[go, i] = best[go]
            moved |= go
            moves += go
        rounds[live & moved] += 1
        live &= moved
        if not live.any():
            break
    return rb.astype(np.int32), rounds, moves, calls


def make_env(cfg, b):
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    return env


def run(name, iters, warmup):
    cfg, b = CONFIGS[name]
    env = make_env(cfg, b)
    res = env.rb_ascent(max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    k = env._rbascent
    rounds, moves, conv = res.rounds.cpu().numpy(), res.moves.cpu().numpy(), res.converged.cpu().numpy()
    solved = res.rb.cpu().numpy()
    dyn = env.best_response_dynamics(max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    rec = {'config': name, 'envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'max_rounds': MAX_ROUNDS,
           'lds_bytes': rb_ascent.lds_bytes(k.n, k.r, k.law != 0),
           'rounds': {'mean': round(float(rounds.mean()), 2), 'max': int(rounds.max())},
           'moves': {'mean': round(float(moves.mean()), 2), 'max': int(moves.max())}, 'converged': int(conv.sum()),
           'brdyn_rounds_mean': round(float(dyn.rounds.float().mean()), 2), 'brdyn_moves_mean': round(float(dyn.moves.float().mean()), 2)}
    labels = ['rb_ascent', 'brdyn']
    fns = [lambda: env.rb_ascent(max_rounds=MAX_ROUNDS), lambda: env.best_response_dynamics(max_rounds=MAX_ROUNDS)]
    times = dict(zip(labels, alternating_us(fns, iters, warmup)))
    rec['rb_ascent_us'], rec['brdyn_us'] = times['rb_ascent'], times['brdyn']
    rec['rb_ascent_over_brdyn'] = round(times['rb_ascent']['median'] / times['brdyn']['median'], 2)
    # the host loop: one run, wall clock, on the first host_envs envs (the same seeds give the same first envs)
    hb = HOST_ENVS[name]
    small = env if hb == b else make_env(cfg, hb)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hrb, hr, hm, calls = host_loop(small)
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    rec['host_envs'], rec['host_loop_evaluate_calls'], rec['host_loop_us'] = hb, calls, round(host_us, 1)
    rec['host_loop_equal'] = bool(np.array_equal(hrb, solved[:hb]) and np.array_equal(hr, rounds[:hb]) and np.array_equal(hm, moves[:hb]))
    rec['host_loop_scaled_us'] = round(host_us * b / hb, 1)
    rec['host_loop_scaled'] = hb != b
    rec['host_loop_over_rb_ascent'] = round(rec['host_loop_scaled_us'] / times['rb_ascent']['median'], 1)
    rec['host_loop_over_rb_ascent_unscaled'] = round(host_us / times['rb_ascent']['median'], 1)
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
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'rb_ascent_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='rb_ascent_cost', iters=a.iters, **run(name, a.iters, a.warmup)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

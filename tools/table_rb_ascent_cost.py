#!/usr/bin/env python3
"""Cost of the sum-capacity RB ascent on a path-loss table (VecD2DEnv.rb_ascent_table, csrc/d2d_tabascent.hip) on the GPU against
the native rb_ascent() of the same shape and against what the env offered before it: the same ascent as a host loop, one
evaluate_table() launch and one round trip per link turn; one JSON line per configuration, printed and appended to
profiles/table_rb_ascent_cost.jsonl (--out).

    python tools/table_rb_ascent_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--out FILE]

stress: 4096 envs x (256 + 256) links x 256 RBs, 1/d^2; config2: BASELINE config 2, 1024 x (25 + 25) links x 25 RBs.  ONE native env
per configuration; the table is the env's own law written out in dB by (tx link, rx link) in float64 torch ops and handed over as a
float32 tensor [B, N, N] through table=, so both solvers climb the same landscape (the trajectories need not agree word for word:
the table's entries are rounded to float32 dB).  No floors, no allowed mask, every link movable, min_gain_mbps 0, max_rounds 16.
If one rb_ascent_table() call of a configuration takes more than --limit-s seconds, the configuration is timed on its first
--fallback-envs envs instead, and the line says so (timed_envs).  In one process, per configuration:

  table_us          one rb_ascent_table() call: the conversion and every turn of every round of every env (two launches).  Device
                    events, median of K after W warm-up calls, timed ALTERNATELY with the two legs below (one call of each per round)
  convert_us        the same call with NO movable link: the conversion of the whole table, the staging of every env and its final
                    planes, no turn.  An upper bound of the conversion's share
  native_us         one rb_ascent() launch on the same env
  host_loop_us      the whole host loop over evaluate_table(), ONE run, wall clock, on the first host_envs envs; its RBs, rounds and
                    moves must equal the call's on those envs (host_loop_equal).  host_loop_scaled_us is host_loop_us x timed_envs /
                    host_envs, a linear scaling stated as such
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
from gym_d2d_amd import table_rb_ascent
from rb_ascent_cost import make_env, seq_sum

HOST_ENVS = {'stress': 8, 'config2': 256}
MAX_ROUNDS = 16


def law_table(env):
    """The native law as a float32 dB table [B, N, N] by (tx link j, rx link i), evaluated in float64 torch ops, env chunk by env
    chunk: a_tx[tx_j] + a_rx[rx_i] + 10 exponent[tx_j] log10 d(tx_j, rx_i)."""
    sim = env.simulator
    law = {k: torch.as_tensor(np.asarray(v, dtype=np.float64), device=env.device) for k, v in sim.path_loss_table.law.items()
           if k in ('a_tx_db', 'a_rx_db', 'exponent')}
    tx, rx = (torch.as_tensor(np.asarray(j, dtype=np.int64), device=env.device) for j in (sim.link_tx, sim.link_rx))
    out = torch.empty((env.num_envs, env.num_links, env.num_links), dtype=torch.float32, device=env.device)
    for lo in range(0, env.num_envs, 64):
        p = env.link_positions()[lo:lo + 64].to(torch.float64)
        d = torch.sqrt((p[:, :, None, 0] - p[:, None, :, 2]) ** 2 + (p[:, :, None, 1] - p[:, None, :, 3]) ** 2)           # [b, j, i]
        out[lo:lo + 64] = law['a_tx_db'][tx][None, :, None] + law['a_rx_db'][rx][None, None, :] \
            + 10.0 * law['exponent'][tx][None, :, None] * torch.log10(d)
    return out


def host_loop(env, table, max_rounds=MAX_ROUNDS):
    """include/d2d_tabascent.h's statement over evaluate_table(), without floors or mask, every env taking link i's turn in one
    call; returns (rb, rounds, moves, evaluate_table calls)."""
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
            cap = env.evaluate_table(torch.as_tensor(cand.astype(np.int32), device=env.device), pwr, table=table,
                                     planes=('capacity_mbps',))['capacity_mbps']
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


def run(name, iters, warmup, limit_s, fallback_envs):
    cfg, b = CONFIGS[name]
    env = make_env(cfg, b)
    table = law_table(env)
    call = lambda: env.rb_ascent_table(table, max_rounds=MAX_ROUNDS)
    call()                                                               # allocates the work space
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize()
    one_call_s = time.perf_counter() - t0
    timed = b
    if one_call_s > limit_s and b > fallback_envs:                       # too long for 50 + 50 calls: time the first envs only
        env.close()
        del table, res
        torch.cuda.empty_cache()
        timed = fallback_envs
        env = make_env(cfg, timed)
        table = law_table(env)
        res = call()
        torch.cuda.synchronize()
    k = env._table_rbascent
    rounds, moves, conv = res.rounds.cpu().numpy(), res.moves.cpu().numpy(), res.converged.cpu().numpy()
    solved = res.rb.cpu().numpy()
    nat = env.rb_ascent(max_rounds=MAX_ROUNDS)
    torch.cuda.synchronize()
    rec = {'config': name, 'envs': b, 'timed_envs': timed, 'first_call_s': round(one_call_s, 3), 'links': k.n, 'rbs': k.r,
           'max_rounds': MAX_ROUNDS, 'table_dtype': 'float32', 'lds_bytes': table_rb_ascent.lds_bytes(k.n, k.r),
           'work_space_bytes': table_rb_ascent.work_space_bytes(timed, k.n), 'domain': int(res.domain.sum()),
           'rounds': {'mean': round(float(rounds.mean()), 2), 'max': int(rounds.max())},
           'moves': {'mean': round(float(moves.mean()), 2), 'max': int(moves.max())}, 'converged': int(conv.sum()),
           'native_rounds_mean': round(float(nat.rounds.float().mean()), 2), 'native_moves_mean': round(float(nat.moves.float().mean()), 2),
           'same_rbs_as_native': round(float((nat.rb == res.rb).float().mean()), 4)}
    nobody = np.zeros(k.n, bool)
    fns = [call, lambda: env.rb_ascent_table(table, movable=nobody, max_rounds=MAX_ROUNDS), lambda: env.rb_ascent(max_rounds=MAX_ROUNDS)]
    rec['table_us'], rec['convert_us'], rec['native_us'] = alternating_us(fns, iters, warmup)
    rec['convert_share'] = round(rec['convert_us']['median'] / rec['table_us']['median'], 4)
    rec['table_over_native'] = round(rec['table_us']['median'] / rec['native_us']['median'], 2)
    # the host loop: one run, wall clock, on the first host_envs envs (the same seeds give the same first envs)
    hb = min(HOST_ENVS[name], timed)
    small = env if hb == timed else make_env(cfg, hb)
    sub = table[:hb].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hrb, hr, hm, calls = host_loop(small, sub)
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    rec['host_envs'], rec['host_loop_evaluate_table_calls'], rec['host_loop_us'] = hb, calls, round(host_us, 1)
    rec['host_loop_equal'] = bool(np.array_equal(hrb, solved[:hb]) and np.array_equal(hr, rounds[:hb]) and np.array_equal(hm, moves[:hb]))
    rec['host_loop_scaled_us'] = round(host_us * timed / hb, 1)
    rec['host_loop_over_table'] = round(rec['host_loop_scaled_us'] / rec['table_us']['median'], 1)
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
    ap.add_argument('--limit-s', type=float, default=3.0, help='one call slower than this: time the first --fallback-envs envs')
    ap.add_argument('--fallback-envs', type=int, default=256)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'table_rb_ascent_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='table_rb_ascent_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.limit_s, a.fallback_envs)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

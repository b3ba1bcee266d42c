#!/usr/bin/env python3
"""Cost of packet traffic (VecD2DEnv(traffic=...), csrc/d2d_queue.hip) on the GPU; one JSON line per configuration and deadline,
appended to profiles/queue_cost.jsonl with --record.

    python tools/queue_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--deadlines 8,32] [--record]

stress: 4096 envs x 512 links x 256 RBs; config2: BASELINE config 2, 1024 x 50 links x 25 RBs.  In one process, per configuration
and deadline D:

  queue_us       the queue launch alone between two device events - launch to completion, which at config 2 is mostly launch and
                 event overhead, not the kernel - median of K after W warm-up calls, the step counter advancing so that the ring
                 wraps, timed ALTERNATELY with
  torch_us       the same model written in torch ops on planes of its own (the yardstick: what a user would keep around step()):
                 the on/off chain and the arrivals from torch.rand (torch's own generator - cheaper than a keyed counter-based draw,
                 and dependent on how the batch is sharded), bucketize on a float CDF, the drain as a loop over the D cohorts
  model_bytes    (8 D + 40) bytes per link: the ring read and written, capacity and backlog read, on read and written, seven planes
                 written; ceiling_fraction = model_bytes / queue_us over the store-only ceiling the other costs are held against
                 (6.69 TB/s).  The kernel moves LESS than the model when queues are short: it stops reading
                 the ring where no unserved bits remain.
  step_us        step() of the obs-less env (SignalPlanesObsFunction) without and with traffic=, the envs alternating, wall clock
                 over K steps between two synchronisations, median of five rounds; overhead_us is their difference
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

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.queues import PacketTraffic

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}
STORE_CEILING_BPS = 6.69e12


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
        out.append((statistics.median(t), min(t), max(t)))
    return out


def torch_formulation(env):
    """One queue step in torch ops on planes of its own, reading the env's capacity plane."""
    m, q = env._queues.model, env._queues
    dev, shape = env.device, tuple(q.backlog_bits.shape)
    d, pkt, buf = m.deadline_steps, m.packet_bits, m.buffer_bits
    cdf = torch.as_tensor(q.tables.astype('float64') / 2.0 ** 32, device=dev)                       # [2, 64]
    ring = torch.zeros((d,) + shape, dtype=torch.int32, device=dev)
    on = torch.ones(shape, dtype=torch.bool, device=dev)
    backlog = torch.zeros(shape, dtype=torch.int32, device=dev)
    cap = env._t['capacity_mbps']
    state = {'t': 0}

    def run():
        state['t'] += 1
        s = state['t'] % d
        u = torch.rand(shape, device=dev)
        on.copy_(torch.where(on, u >= m.p_on_to_off, u < m.p_off_to_on))
        u1 = torch.rand(shape, device=dev, dtype=torch.float64)
        k = torch.cat([torch.bucketize(u1[:, :q.cues], cdf[0], right=True), torch.bucketize(u1[:, q.cues:], cdf[1], right=True)], dim=1)
        k = torch.where(on, k, torch.zeros_like(k)).to(torch.int32)
        expired = ring[s].clone()
        kept = backlog - expired
        n = torch.minimum(k, (buf - kept) // pkt)
        ring[s] = n * pkt
        overflow = (k - n) * pkt
        budget = torch.nan_to_num(cap.double() * m.bits_per_mbps_step, nan=0.0).clamp(0.0, 2147483647.0).floor().to(torch.int64)
        served = torch.zeros(shape, dtype=torch.int64, device=dev)
        weighted = torch.zeros(shape, dtype=torch.int64, device=dev)
        hol = torch.zeros(shape, dtype=torch.int32, device=dev)
        for age in range(d - 1, -1, -1):
            slot = (state['t'] - age) % d
            take = torch.minimum(ring[slot].long(), budget)
            ring[slot] -= take.int()
            budget -= take; served += take; weighted += take * age
            hol = torch.where((hol == 0) & (ring[slot] > 0), torch.full_like(hol, age), hol)
        backlog.copy_(kept + n * pkt - served.int())
        delay = torch.where(served > 0, weighted.double() / served.double(), torch.zeros((), dtype=torch.float64, device=dev)).float()
        return k * pkt, overflow, expired, delay
    return run


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, deadline, iters, warmup):
    cfg, b = CONFIGS[name]
    # arrivals a little above what the links carry on average, so that the queues hold bits and the drain walks the ring
    model = PacketTraffic(packets_per_step=2.0, packet_bits=1000, deadline_steps=deadline, buffer_bits=32000, dt_s=1e-3, p_on_to_off=0.1,
                          p_off_to_on=0.3)
    envs = {'plain': VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b),
            'traffic': VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b, traffic=model)}
    for e in envs.values():
        e.reset(seed=1)
    actions = envs['plain'].action_buffer().clone()
    for e in envs.values():
        wall_us(e, actions, warmup)
    rounds = [{k: wall_us(e, actions, iters) for k, e in envs.items()} for _ in range(5)]
    step_us = {k: round(statistics.median(r[k] for r in rounds), 2) for k in envs}
    step_us['spread'] = {k: round(max(r[k] for r in rounds) - min(r[k] for r in rounds), 2) for k in envs}
    step_us['overhead_us'] = round(step_us['traffic'] - step_us['plain'], 2)
    env = envs['traffic']
    q = env._queues
    links = b * env.num_links
    clock = {'t': 5 * iters + warmup}

    def kernel():
        clock['t'] += 1
        q.step(env._t, 1, clock['t'], 0, env._stream_ptr)
    (med, lo, hi), (tm, tl, th) = alternating_us([kernel, torch_formulation(env)], iters, warmup)
    torch.cuda.synchronize()
    rec = {'config': name, 'envs': b, 'links': env.num_links, 'deadline_steps': deadline, 'model_bytes': (8 * deadline + 40) * links,
           'queue_us': {'median': round(med, 2), 'min': round(lo, 2), 'max': round(hi, 2)},
           'torch_us': {'median': round(tm, 2), 'min': round(tl, 2), 'max': round(th, 2)}, 'torch_over_kernel': round(tm / med, 2),
           'ceiling_fraction': round((8 * deadline + 40) * links / (med * 1e-6) / STORE_CEILING_BPS, 4),
           'mean_backlog_bits': round(float(q.backlog_bits.float().mean()), 1), 'step_us': step_us}
    for e in envs.values():
        e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--deadlines', default='8,32')
    ap.add_argument('--record', action='store_true')
    a = ap.parse_args()
    for name in a.configs.split(','):
        for d in map(int, a.deadlines.split(',')):
            line = json.dumps(dict(tool='queue_cost', iters=a.iters, **run(name, d, a.iters, a.warmup)))
            print(line, flush=True)
            if a.record:
                with (ROOT / 'profiles' / 'queue_cost.jsonl').open('a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()

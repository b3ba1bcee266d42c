#!/usr/bin/env python3
"""Cost of device mobility (VecD2DEnv(mobility=...), csrc/d2d_mobility.hip) on the GPU; one JSON line per configuration, appended to
profiles/mobility_cost.jsonl with --record.

    python tools/mobility_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--record]
    python tools/mobility_cost.py --kernel-stats DIR/..._kernel_stats.csv --configs stress [--record]

stress: 4096 envs x 512 links (769 devices) x 256 RBs; config2: BASELINE config 2, 1024 x 50 links x 25 RBs.  In one process, per
configuration:

  move_us        the move launch alone between two device events - launch to completion, which at config 2 is mostly launch and
                 event overhead, not the kernel (the kernel's own time: --kernel-stats below) - median of K after W warm-up
                 calls, timed ALTERNATELY with
  torch_us       the same update written in float32 torch ops on the same planes (what the kernel replaces): the Gaussians from
                 torch.randn (torch's own generator - cheaper than a keyed counter-based draw, and not reproducible across shards),
                 the two fmas, the tether and the wall by masked arithmetic
  moved_bytes    32 bytes per device (position and velocity, read and written); store_ceiling_fraction = moved_bytes / move_us
                 over the store-only ceiling the sensing and graph costs are held against (6.69 TB/s)
  step_us        step() of a mobility-less env, of an env with mobility, and the split of the difference: the move, the link-row
                 gather the step now runs every time (positions_changed), and - for NeighborObsFunction - the neighbour
                 re-selection at neighbor_refresh=1 against a refresh that never comes (K steps between two synchronisations, wall
                 clock, the envs alternating)

The kernel's own time comes from a run of ONE configuration under the profiler,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mobility_cost.py --configs stress`; --kernel-stats then
reads mobility_move_kernel's row of the *_kernel_stats.csv that run wrote and prints (records) it as kernel_ns for that configuration.
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
from gym_d2d_amd.envs.obs_fn import NeighborObsFunction, SignalPlanesObsFunction
from gym_d2d_amd.mobility import GaussMarkovMobility

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
    """One move in float32 torch ops on the env's own planes (the fixed mask left out: nothing is pinned in these configurations)."""
    m, t = env._mobility, env._t
    a, s, _, dt = m.consts
    cell, d2d = m.radii
    c = m.cues
    px, py, vx, vy = t['pos_x'], t['pos_y'], m.vel_x, m.vel_y

    def pull(x, y, cx, cy, radius):
        dx, dy = x - cx, y - cy
        d = torch.sqrt(dx * dx + dy * dy)
        hit = d > radius
        f = torch.where(hit, radius / d, torch.ones_like(d))
        return cx + dx * f, cy + dy * f, hit

    def run():
        vx[:, 1:] = a * vx[:, 1:] + s * torch.randn_like(vx[:, 1:])
        vy[:, 1:] = a * vy[:, 1:] + s * torch.randn_like(vy[:, 1:])
        px[:, 1:] += vx[:, 1:] * dt
        py[:, 1:] += vy[:, 1:] * dt
        first = slice(1, c + 1)                                     # CUEs, then the transmitters, against the wall
        for sl in (first, slice(c + 1, None, 2)):
            x, y, hit = pull(px[:, sl], py[:, sl], 0.0, 0.0, cell)
            px[:, sl], py[:, sl] = x, y
            sign = torch.where(hit, -1.0, 1.0)
            vx[:, sl] *= sign; vy[:, sl] *= sign
        rx, tx = slice(c + 2, None, 2), slice(c + 1, None, 2)       # the receivers: tether, then the wall
        x, y, hit = pull(px[:, rx], py[:, rx], px[:, tx], py[:, tx], d2d)
        x, y, wall = pull(x, y, 0.0, 0.0, cell)
        px[:, rx], py[:, rx] = x, y
        sign = torch.where(hit ^ wall, -1.0, 1.0)
        vx[:, rx] *= sign; vy[:, rx] *= sign
    return run


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def step_costs(cfg, b, iters, warmup, obs_fn, variants):
    """Median per-step wall time of each env variant (name -> VecD2DEnv keywords), the envs alternating, five rounds."""
    envs = {name: VecD2DEnv(dict(cfg, obs_fn=obs_fn), num_envs=b, **kw) for name, kw in variants.items()}
    for e in envs.values():
        e.reset(seed=1)
    actions = next(iter(envs.values())).action_buffer().clone()
    for e in envs.values():
        wall_us(e, actions, warmup)
    rounds = [{name: wall_us(e, actions, iters) for name, e in envs.items()} for _ in range(5)]
    out = {name: round(statistics.median(r[name] for r in rounds), 2) for name in envs}
    out['spread'] = {name: round(max(r[name] for r in rounds) - min(r[name] for r in rounds), 2) for name in envs}
    return out, envs


def run(name, iters, warmup):
    cfg, b = CONFIGS[name]
    model = GaussMarkovMobility()
    rec = {'config': name, 'envs': b}
    planes, envs = step_costs(cfg, b, iters, warmup, SignalPlanesObsFunction, {'still': {}, 'moving': {'mobility': model}})
    env = envs['moving']
    envs['still'].close()
    m = env._mobility
    devices = env.simulator.handle.num_devices
    rec.update(links=env.num_links, devices=devices, moved_bytes=32 * b * devices)
    # the gather alone: a mobility-less step that is told every time that the positions changed
    h = env.simulator.handle
    actions = env.action_buffer().clone()

    def gather_step():
        h.positions_changed(); h.step(actions.data_ptr())

    def plain_step():
        h.step(actions.data_ptr())
    t_gather, t_plain = alternating_us([gather_step, plain_step], iters, warmup)
    fns = [lambda: m.move(env._t, 1, 3, 0, env._stream_ptr), torch_formulation(env)]
    (med, lo, hi), (tm, tl, th) = alternating_us(fns, iters, warmup)
    rec['move_us'] = {'median': round(med, 2), 'min': round(lo, 2), 'max': round(hi, 2)}
    rec['torch_us'] = {'median': round(tm, 2), 'min': round(tl, 2), 'max': round(th, 2)}
    rec['torch_over_kernel'] = round(tm / med, 2)
    rec['store_ceiling_fraction'] = round(rec['moved_bytes'] / (med * 1e-6) / STORE_CEILING_BPS, 4)
    rec['step_us'] = {'planes': planes, 'link_row_gather_us': round(t_gather[0] - t_plain[0], 2)}
    env.close()
    nb, envs = step_costs(cfg, b, iters, warmup, NeighborObsFunction,
                          {'still': {}, 'moving_refresh_1': {'mobility': model}, 'moving_no_refresh': {'mobility': model, 'neighbor_refresh': 1 << 30}})
    nb['neighbor_reselect_us'] = round(nb['moving_refresh_1'] - nb['moving_no_refresh'], 2)
    rec['step_us']['neighbor_obs'] = nb
    for e in envs.values():
        e.close()
    return rec


def kernel_stats(path, name):
    """mobility_move_kernel's row of a rocprofv3 *_kernel_stats.csv, for the one configuration that run timed."""
    import csv
    cfg, b = CONFIGS[name]
    devices = 1 + cfg['num_cues'] + 2 * cfg['num_due_pairs']
    with open(path, newline='') as f:
        rows = [r for r in csv.DictReader(f) if 'mobility_move_kernel' in r['Name']]
    if len(rows) != 1:
        raise SystemExit(f'{path}: {len(rows)} rows name mobility_move_kernel')
    r = rows[0]
    avg = float(r['AverageNs'])
    return {'config': name, 'envs': b, 'devices': devices, 'source': 'rocprofv3 --kernel-trace --stats', 'calls': int(r['Calls']),
            'kernel_ns': {'average': round(avg, 1), 'min': float(r['MinNs']), 'max': float(r['MaxNs']), 'stddev': round(float(r['StdDev']), 1)},
            'moved_bytes': 32 * b * devices, 'store_ceiling_fraction': round(32 * b * devices / (avg * 1e-9) / STORE_CEILING_BPS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--record', action='store_true')
    ap.add_argument('--kernel-stats', default=None)
    a = ap.parse_args()
    for name in a.configs.split(','):
        if a.kernel_stats:
            line = json.dumps(dict(tool='mobility_cost', **kernel_stats(a.kernel_stats, name)))
        else:
            line = json.dumps(dict(tool='mobility_cost', iters=a.iters, **run(name, a.iters, a.warmup)))
        print(line, flush=True)
        if a.record:
            with (ROOT / 'profiles' / 'mobility_cost.jsonl').open('a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

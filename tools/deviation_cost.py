#!/usr/bin/env python3
"""Cost of the unilateral-deviation gains (VecD2DEnv.deviation_gains / best_deviation, csrc/d2d_deviate.hip) on the GPU against the
only other route to the same words - the host loop of evaluate() launches, one per selected link with R Lmax + 1 candidates - and,
for scale, against one rb_ascent() plus one power_ascent() launch on the same state; one JSON line per configuration, printed and
appended to profiles/deviation_cost.jsonl (--out).

    python tools/deviation_cost.py [--iters K] [--warmup W] [--configs config2,stress] [--out FILE]

config2: BASELINE config 2, 1024 envs x (25 + 25) links x 25 RBs, every link selected.  stress: the first 256 envs of 4096 envs x
(256 + 256) links x 256 RBs, 1/d^2; the table is taken for every fourth link (128 links: 0.8 GB), best_deviation() for all 512.  No
floors, no allowed mask, min_gain_mbps 0.  In one process, per configuration:

  gains_us          one deviation_gains() launch.  Device events, median of K after W warm-up calls, timed ALTERNATELY with the legs
                    below (one call of each per round).  table_bytes, table_gb_s and, where the probe library is built,
                    fraction_of_write_ceiling: the table store's share of the box's store-only ceiling (tools/write_probe.py)
  best_us           one best_deviation() call (two launches) at the full selection
  rb_ascent_us      one rb_ascent(max_rounds=16) launch on the same state
  power_ascent_us   one power_ascent(max_rounds=16) launch on the same state
                    (an ascent whose single probe call takes more than --leg-limit-s seconds is not put through K rounds: its one
                    call is *_one_call_us and its median is 'not measured')
  host_loop_us      the host loop (tests/deviation_util.by_evaluate: the statement, stated once), ONE run, wall clock, on host_envs
                    envs and host_links links; table and best_deviation outputs must equal the launch's on those envs and links
                    (host_loop_equal).  host_loop_scaled_us is host_loop_us x envs / host_envs x links / host_links, a linear
                    scaling stated as such
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
from deviation_util import by_evaluate
from gym_d2d_amd import deviation
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

ENVS = {'config2': 1024, 'stress': 256}
TABLE_EVERY = {'config2': 1, 'stress': 4}       # the table's selection: every k-th link
HOST = {'config2': (16, 1), 'stress': (2, 128)}  # the host loop: envs, and every k-th link
MAX_ROUNDS = 16


def make_env(cfg, b):
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    return env


def one_call_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) * 1e3, 2)


def run(name, iters, warmup, leg_limit_s, ceiling):
    cfg, full = CONFIGS[name]
    b = ENVS[name]
    env = make_env(cfg, b)
    n = env.num_links
    links = list(range(0, n, TABLE_EVERY[name]))
    table, sel, levels = env.deviation_gains(links)
    best = env.best_deviation()
    torch.cuda.synchronize()
    k = env._deviation
    nbytes = deviation.table_bytes(*table.shape)
    rec = {'config': name, 'envs_of_the_config': full, 'timed_envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'levels': int(table.shape[3]),
           'lds_bytes': deviation.lds_bytes(k.n, k.r), 'table_links': len(links), 'table_shape': list(table.shape), 'table_bytes': nbytes,
           'best_links': k.n, 'open_share': round(float(torch.isfinite(table).float().mean()), 4),
           'regret_mbps_mean': round(float(best.regret_mbps.mean()), 4), 'movers_mean': round(float((best.gain_mbps > 0).sum(dim=1).float().mean()), 2)}
    legs = {'gains_us': lambda: env.deviation_gains(links), 'best_us': lambda: env.best_deviation()}
    for leg, fn in (('rb_ascent_us', lambda: env.rb_ascent(max_rounds=MAX_ROUNDS)), ('power_ascent_us', lambda: env.power_ascent(max_rounds=MAX_ROUNDS))):
        once = one_call_us(fn)
        if once > leg_limit_s * 1e6:
            rec[leg.replace('_us', '_one_call_us')], rec[leg] = once, 'not measured'
        else:
            legs[leg] = fn
    for leg, t in zip(legs, alternating_us(list(legs.values()), iters, warmup)):
        rec[leg] = t
    rec['table_gb_s'] = round(nbytes / rec['gains_us']['median'] / 1e3, 1)
    if ceiling:
        rec['box_write_ceiling_gb_s'] = round(ceiling, 1)
        rec['fraction_of_write_ceiling'] = round(rec['table_gb_s'] / ceiling, 4)
    else:
        rec['fraction_of_write_ceiling'] = 'not measured'
    if all(isinstance(rec[x], dict) for x in ('rb_ascent_us', 'power_ascent_us')):
        both = rec['rb_ascent_us']['median'] + rec['power_ascent_us']['median']
        rec['gains_over_rb_plus_power'] = round(rec['gains_us']['median'] / both, 3)
        rec['best_over_rb_plus_power'] = round(rec['best_us']['median'] / both, 3)
    env.close()
    # the host loop: one run, wall clock, on the first host_envs envs (the same seeds give the same first envs) and host_links links
    hb, every = HOST[name]
    small = make_env(cfg, hb)
    hl = list(range(0, n, every))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    (want,), calls = by_evaluate(small, hl, [(None, None, 0.0)])
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) * 1e6
    got_t = small.deviation_gains(hl)[0].cpu().numpy()
    got_b = [t.cpu().numpy() for t in small.best_deviation(hl)]
    same = [got_t.tobytes() == want.table.tobytes()] + [x.tobytes() == np.ascontiguousarray(y.astype(x.dtype)).tobytes() for x, y in
                                                       zip(got_b, (want.rb_out, want.pwr_out, want.gain_link, want.regret, want.leader))]
    rec.update(host_envs=hb, host_links=len(hl), host_loop_evaluate_calls=calls, host_loop_us=round(host_us, 1), host_loop_equal=bool(all(same)))
    rec['host_loop_scaled_us'] = round(host_us * b / hb * len(links) / len(hl), 1)
    rec['host_loop_over_gains'] = round(rec['host_loop_scaled_us'] / rec['gains_us']['median'], 1)
    small.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', default='config2,stress')
    ap.add_argument('--leg-limit-s', type=float, default=0.25)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'deviation_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    ceiling = 0.0
    try:
        import write_probe
        ceiling = float(write_probe.write_variants(1 << 31, 5)[0])
    except Exception as e:      # the probe library is measurement equipment: report without it
        print(json.dumps({'tool': 'deviation_cost', 'write_probe': f'unavailable: {e}'}), file=sys.stderr)
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='deviation_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.leg_limit_s, ceiling)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

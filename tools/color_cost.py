#!/usr/bin/env python
"""Cost of the conflict-graph RB colouring (VecD2DEnv.color_graph / color_rbs, csrc/d2d_color.hip) on the GPU; one JSON line per
configuration, printed and appended to profiles/color_cost.jsonl (--out).

    python tools/color_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--margin-db M] [--out FILE]

Per configuration (state: reset, then one step with the reset's random actions; the SIR graph at --margin-db, every agent link
movable, every RB allowed, pack False):
  conflicts, rbs_used, proper, degree   what the kernel did per env, and the mean degree of the conflict graph
  color_graph_us   the colouring launch alone on the prepared score / bias / threshold tensors, device events, median of K after W
                   warm-up calls - timed ALTERNATELY, one call of each per round in one process, with
  color_rbs_us     color_rbs(): coupling(), the three elementwise torch operations and the colouring
  coupling_us      coupling() alone
  brdyn_us         best_response_dynamics() at its defaults, for scale
  assign_rbs_us    assign_rbs() at its defaults (the DUE pairs, one RB each), for scale
  numpy_env_us     the NumPy restatement (tests/color_util.py) of ONE env on one host core: the host clock around 8 envs, divided by 8
  numpy_all_us     numpy_env_us x envs: SCALED from those 8 envs, not measured

Every GPU step of a measuring session runs under its own `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/color_cost.py --configs stress && timeout -k 10 120 python tools/color_cost.py --configs config2
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
import numpy as np
import torch

import color_util
from gym_d2d_amd import coloring
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}
HOST_ENVS = 8


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


def run(name, iters, warmup, margin_db):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    res = env.color_rbs(margin_db)
    k = env._color
    # the tensors color_rbs() hands the kernel, kept: the launch alone is timed on them
    score = env.coupling().clone()
    bias = env._t['pwr'].to(torch.float32).contiguous()
    thr = coloring.sir_threshold(score, bias, k.margin(margin_db, env.num_cues)).contiguous()
    alone = env.color_graph(score, thr, bias)
    assert all(torch.equal(x, y) for x, y in zip(alone, env.color_rbs(margin_db)))
    hurts = (score[:HOST_ENVS] + bias[:HOST_ENVS, None, :]) >= thr[:HOST_ENVS, :, None]
    hurts &= ~torch.eye(k.n, dtype=torch.bool, device=env.device)
    degree = float((hurts | hurts.transpose(1, 2)).sum(dim=2).float().mean())
    rec = {'config': name, 'envs': b, 'links': k.n, 'rbs': k.r, 'margin_db': margin_db, 'pack': False,
           'lds_bytes': coloring.lds_bytes(k.n, k.r, False),
           'conflicts': {'mean': round(float(res.conflicts.float().mean()), 2), 'max': int(res.conflicts.max())},
           'rbs_used': {'mean': round(float(res.rbs_used.float().mean()), 2), 'max': int(res.rbs_used.max())},
           'proper': round(float(res.proper.float().mean()), 4), 'degree_mean_of_8_envs': round(degree, 2)}
    times = alternating_us([lambda: env.color_graph(score, thr, bias), lambda: env.color_rbs(margin_db), env.coupling,
                            env.best_response_dynamics, env.assign_rbs], iters, warmup)
    rec['color_graph_us'], rec['color_rbs_us'], rec['coupling_us'], rec['brdyn_us'], rec['assign_rbs_us'] = times
    # the restatement on the host: the same tensors, downloaded
    host = [a[:HOST_ENVS].cpu().numpy() for a in (score, bias, thr, env._t['rb'])]
    t0 = time.perf_counter()
    want = color_util.color_graph(host[0], host[1], host[2], host[3], k.r, env._agent_links(), None, False)
    per_env = (time.perf_counter() - t0) / HOST_ENVS * 1e6
    assert all(np.array_equal(x[:HOST_ENVS].cpu().numpy(), y) for x, y in zip(env.color_graph(score, thr, bias), want))
    rec['numpy_env_us'] = round(per_env, 1)
    rec['numpy_all_us'] = round(per_env * b, 1)
    rec['numpy_all_scaled_from_envs'] = HOST_ENVS
    rec['numpy_all_over_color_graph'] = round(per_env * b / times[0]['median'], 1)
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--margin-db', type=float, default=10.0)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'color_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='color_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.margin_db)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

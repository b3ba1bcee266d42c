#!/usr/bin/env python
"""Cost of the stable RB matching (VecD2DEnv.solve_stable_matching / stable_rbs, csrc/d2d_stable.hip) on the GPU; one JSON line per
configuration, printed and appended to profiles/stable_cost.jsonl (--out).

    python tools/stable_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--margin-db M] [--out FILE]

Per configuration (state: reset, then one step with the reset's random actions; the DUE pairs movable, every RB allowed, quota 1,
rb_pref 'harm'):
  proposals, unmatched   what the kernel did per env
  solve_us         the matching launch alone on the prepared preference tensors, device events, median of K after W warm-up calls -
                   timed ALTERNATELY, one call of each per round in one process, with
  stable_rbs_us    stable_rbs(): assignment_weights(), the negation, the matching and the scatter
  weights_us       assignment_weights(objective='own', harm=True) alone
  assign_rbs_us    assign_rbs() at its defaults (the Hungarian optimum of the same pairs), for scale
  color_rbs_us     color_rbs(--margin-db) at its defaults, for scale
  numpy_env_us     the sequential NumPy restatement (tests/stable_util.py) of ONE env on one host core: the host clock around 8 envs,
                   divided by 8; its four outputs must equal the kernel's

Every GPU step of a measuring session runs under its own `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/stable_cost.py --configs stress && timeout -k 10 120 python tools/stable_cost.py --configs config2
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
sys.path.insert(0, str(ROOT / 'tools'))
import numpy as np
import torch

import stable_util
from color_cost import CONFIGS, HOST_ENVS, alternating_us
from gym_d2d_amd import stable_matching
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction


def run(name, iters, warmup, margin_db):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    res = env.stable_rbs()
    # the tensors stable_rbs() hands the kernel, kept: the launch alone is timed on them
    own, links, harm = (x.clone() for x in env.assignment_weights(objective='own', harm=True))
    pref = torch.neg(harm)
    alone = env.solve_stable_matching(own, pref)
    idx = links.long()
    assert torch.equal(alone.col, res.rb[:, idx]) and torch.equal(alone.proposals, res.proposals)
    m, r = int(own.shape[1]), int(own.shape[2])
    rec = {'config': name, 'envs': b, 'links': env.num_links, 'movable': m, 'rbs': r, 'quota': 1, 'rb_pref': 'harm',
           'lds_bytes': stable_matching.lds_bytes(m, r),
           'proposals': {'mean': round(float(res.proposals.float().mean()), 2), 'max': int(res.proposals.max())},
           'unmatched': {'mean': round(float(res.unmatched.float().mean()), 2), 'max': int(res.unmatched.max())}}
    times = alternating_us([lambda: env.solve_stable_matching(own, pref), env.stable_rbs,
                            lambda: env.assignment_weights(objective='own', harm=True), env.assign_rbs, lambda: env.color_rbs(margin_db)],
                           iters, warmup)
    rec['solve_us'], rec['stable_rbs_us'], rec['weights_us'], rec['assign_rbs_us'], rec['color_rbs_us'] = times
    rec['color_margin_db'] = margin_db
    # the restatement on the host: the same tensors, downloaded
    host = [a[:HOST_ENVS].cpu().numpy() for a in (own, pref)]
    t0 = time.perf_counter()
    want = stable_util.solve_batch(host[0], host[1], 1)
    per_env = (time.perf_counter() - t0) / HOST_ENVS * 1e6
    assert all(np.array_equal(x[:HOST_ENVS].cpu().numpy(), y) for x, y in zip(env.solve_stable_matching(own, pref), want))
    rec['numpy_env_us'] = round(per_env, 1)
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--margin-db', type=float, default=10.0)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'stable_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='stable_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.margin_db)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

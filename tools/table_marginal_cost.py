#!/usr/bin/env python3
"""Cost of difference rewards on a path-loss table (VecD2DEnv.marginal_capacity_table, TableDifferenceRewardFunction,
csrc/d2d_tabmarg.hip) on the GPU; one JSON line per configuration and entry type, printed and appended to
profiles/table_marginal_cost.jsonl (--out).

    python tools/table_marginal_cost.py [--iters K] [--warmup W] [--configs config2,stress] [--dtypes float64,float32] [--out FILE]

config2: BASELINE config 2, 1024 envs x 50 links x 25 RBs; stress: 4096 x 512 links x 256 RBs.  The channel env is a
SpatialChannelPathLoss (log-distance median, 8 dB shadowing, Rayleigh fading: the table is filled before every step).  In one
process, per configuration and entry type of the live table, device events, median of K after W warm-up calls, all legs timed
ALTERNATELY (one call of each per round); the line states the box (device, architecture, compute units, memory, torch and HIP versions):

  marginal_table_us   (a) one marginal_capacity_table() launch on the channel env
  loo_us              (b) what it replaces: one evaluate_table() launch with K = N + 1 leave-one-out candidates per env (the state,
                      and the state with link i on no RB), totals only, on the first loo_envs envs (an env of its own with the same
                      seed: the full batch at config2, --loo-envs at stress, where the candidate planes alone would be 8.6 GB);
                      loo_scaled_us is loo_us x envs / loo_envs, a linear scaling stated as such
  marginal_us         (c) one marginal_capacity() launch on the native env of the same shape (log-distance, the same exponent)
  step_us             (d) step() with TableDifferenceRewardFunction against step() with SystemCapacityRewardFunction on the same
                      'channel' env (both fill the table before the step), both obs-less
  equal               difference == the last step's capacity_mbps - harm as float32, bit for bit; domain flags raised

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/table_marginal_cost.py --out ''`: the kernel
is tabmarg_kernel<float | double> (libd2d_tabmarg.so).
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tools'))
import torch

from gym_d2d_amd import table_marginal
from gym_d2d_amd.envs import TableDifferenceRewardFunction, VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.envs.reward_fn import SystemCapacityRewardFunction
from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss
from table_evaluate_cost import CONFIGS, PLE, Median, alternating_us


def channel_model(dtype):
    return type('Channel', (SpatialChannelPathLoss,), dict(median=LogDistancePathLoss, median_kwargs={'ple': PLE}, fading='rayleigh',
                                                           num_sinusoids=8, table_dtype=dtype))


def box():
    p = torch.cuda.get_device_properties(0)
    return {'device': p.name, 'arch': getattr(p, 'gcnArchName', ''), 'compute_units': p.multi_processor_count,
            'memory_gib': round(p.total_memory / 2 ** 30, 1), 'torch': torch.__version__, 'hip': torch.version.hip}


def make(cfg, b, **kw):
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, **kw), num_envs=b)
    env.reset(seed=1)
    return env


def loo_planes(env):
    """rb, pwr int32 [B, N + 1, N]: candidate 0 is the env's state, candidate i + 1 has link i on no RB."""
    n = env.num_links
    rb = env._t['rb'][:, None, :].repeat(1, n + 1, 1)
    idx = torch.arange(n, device=env.device)
    rb[:, idx + 1, idx] = -1
    return rb.contiguous(), env._t['pwr'][:, None, :].repeat(1, n + 1, 1).contiguous()


def run(name, dtype, iters, warmup, loo_envs):
    cfg, b = CONFIGS[name]
    model = channel_model(dtype)
    diff_env = make(cfg, b, path_loss_model=model, reward_fn=TableDifferenceRewardFunction)
    cap_env = make(cfg, b, path_loss_model=model, reward_fn=SystemCapacityRewardFunction)
    native = make(cfg, b, path_loss_model=Median)
    hb = b if name == 'config2' else min(b, loo_envs)
    small = make(cfg, hb, path_loss_model=model)
    actions = diff_env.action_buffer().clone()
    _, rewards, _, info = diff_env.step(actions)
    for env in (cap_env, native):
        env.step(actions)
    small.step(actions[:hb].contiguous())
    n, r = diff_env.num_links, diff_env.config.num_rbs
    live = diff_env.simulator.path_loss_table.live
    res = diff_env.marginal_capacity_table()
    rec = {'config': name, 'envs': b, 'links': n, 'rbs': r, 'table_dtype': dtype, 'box': box(),
           'table_bytes': int(live.numel() * live.element_size()), 'lds_bytes': table_marginal.lds_bytes(n, r),
           'equal': {'difference': bool(torch.equal(res.difference_mbps, info['capacity_mbps'] - res.harm_mbps)),
                     'reward': bool(torch.equal(rewards, res.difference_mbps)), 'domain': int(res.domain.sum())},
           'harmful_share': round(float((res.harm_mbps > 0).float().mean()), 4)}
    rb, pwr = loo_planes(small)
    fns = [lambda: diff_env.marginal_capacity_table(), lambda: small.evaluate_table(rb, pwr, planes=()),
           lambda: native.marginal_capacity(), lambda: diff_env.step(actions), lambda: cap_env.step(actions)]
    a, loo, nat, step_diff, step_cap = alternating_us(fns, iters, warmup)
    rec['marginal_table_us'], rec['loo_us'], rec['loo_envs'] = a, loo, hb
    rec['loo_scaled_us'] = round(loo['median'] * b / hb, 1)
    rec['loo_over_table'] = round(rec['loo_scaled_us'] / a['median'], 1)
    rec['marginal_us'] = nat
    rec['table_over_native'] = round(a['median'] / nat['median'], 2)
    rec['step_us'] = {'table_difference': step_diff, 'system_capacity': step_cap}
    rec['step_extra_us'] = round(step_diff['median'] - step_cap['median'], 2)
    for env in (diff_env, cap_env, native, small):
        env.close()
    del diff_env, cap_env, native, small, rb, pwr, res, info, rewards, live
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--configs', default='config2,stress')
    ap.add_argument('--dtypes', default='float64,float32')
    ap.add_argument('--loo-envs', type=int, default=256, help='envs the leave-one-out evaluate_table() leg is timed on at stress')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'table_marginal_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        for dtype in a.dtypes.split(','):
            line = json.dumps(dict(tool='table_marginal_cost', iters=a.iters, **run(name, dtype, a.iters, a.warmup, a.loo_envs)))
            print(line, flush=True)
            if a.out:
                Path(a.out).parent.mkdir(parents=True, exist_ok=True)
                with open(a.out, 'a') as f:
                    f.write(line + '\n')


if __name__ == '__main__':
    main()

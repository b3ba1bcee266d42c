#!/usr/bin/env python3
"""Cost of the difference rewards (VecD2DEnv.marginal_capacity, csrc/d2d_marginal.hip) on the GPU; one JSON line per configuration.

    python tools/marginal_cost.py [--iters K] [--warmup W] [--configs stress,stress_hata,config2] [--no-baseline]

stress: 4096 envs x 512 links x 256 RBs, 1/d^2; stress_hata: the same with COST-Hata urban (the pow-k law); config2: BASELINE
config 2, 1024 x 50 links x 25 RBs.  In one process, per configuration:

  marginal_us    the launch alone, device events, median of K after W warm-up calls - timed ALTERNATELY with
  torch_us       the same two planes the way a user had to compute them before: the gain cube [B, N, N] from coupling()-style
                 arithmetic in float32 torch, the same-RB mask, leave-one-out by broadcast (cap_j(I_j - t_ij) for every pair)
  torch_vs_kernel_max_abs_mbps   their mutual difference on harm and on difference (the torch side is float32 throughout)
  step_us        step() with DifferenceRewardFunction against step() with SystemCapacityRewardFunction, both obs-less
                 (SignalPlanesObsFunction), lockstep and autoreset (K steps between two synchronisations, wall clock, alternating)

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/marginal_cost.py --no-baseline`: the kernel
is marginal_kernel<law> (libd2d_marginal.so).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from gym_d2d_amd.envs import DifferenceRewardFunction, VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.envs.reward_fn import SystemCapacityRewardFunction
from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss


class UrbanHata(CostHataPathLoss):
    def __init__(self, f):
        super().__init__(f, AreaType.URBAN)


CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'stress_hata': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256, 'path_loss_model': UrbanHata}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}


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
    """marginal_capacity() rebuilt in float32 torch from the kernel's own columns (what a user had to write before)."""
    m, t = env._marginal_kernel(), env._t
    tx, rx, cols, cap_cols = m.tx.long(), m.rx.long(), m.cols, m.cap_cols
    n = m.n
    eye = torch.eye(n, dtype=torch.bool, device=env.device)
    expo = None
    if m.law != 0:
        expo = torch.as_tensor(env.simulator.path_loss_table.law['exponent'], dtype=torch.float32, device=env.device)[tx]
    rx_pl, rx_lin, noise = cols[1][rx][None, :], cols[2][rx][None, :], cols[3][rx][None, :]
    bw, sens = cap_cols[0][tx][None, :], cap_cols[1][rx][None, :]

    def capacity(sig, ix, bw_, sens_, rx_pl_, noise_):
        sinr = sig / (ix * rx_pl_ + noise_)
        return torch.where(10.0 * torch.log10(sinr) > sens_, bw_ * torch.log2(1.0 + sinr), torch.zeros((), device=sinr.device))

    def run():
        px, py = t['pos_x'], t['pos_y']
        dx = px[:, tx, None] - px[:, None, rx]
        dy = py[:, tx, None] - py[:, None, rx]
        d2 = dx * dx + dy * dy                                                 # [B, i (transmits), j (receives)]
        gain = 1.0 / d2 if expo is None else d2 ** (-0.5 * expo)[None, :, None]
        pw = torch.pow(10.0, t['pwr'].float() / 10.0) * cols[0][tx][None, :]   # [B, i]
        sig = (pw * torch.diagonal(gain, dim1=1, dim2=2)) * (rx_pl * rx_lin)   # [B, j]
        same = (t['rb'][:, :, None] == t['rb'][:, None, :]) & ~eye[None]
        tij = (gain * pw[:, :, None]) * same                                   # what i puts into j's receiver, same RB only
        ix = tij.sum(dim=1)                                                    # [B, j]
        cap = capacity(sig, ix, bw, sens, rx_pl, noise)
        without = capacity(sig[:, None, :], ix[:, None, :] - tij, bw[:, None, :], sens[:, None, :], rx_pl[:, None, :], noise[:, None, :])
        harm = ((without - cap[:, None, :]) * same).sum(dim=2)
        return cap - harm, harm
    return run


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, iters, warmup, baseline):
    cfg, b = CONFIGS[name]
    rec = {'config': name, 'envs': b}
    step_us = {}
    for mode, kw in (('lockstep', {}), ('autoreset', {'autoreset': True})):
        base = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, reward_fn=SystemCapacityRewardFunction), num_envs=b, **kw)
        diff = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction, reward_fn=DifferenceRewardFunction), num_envs=b, **kw)
        base.reset(seed=1); diff.reset(seed=1)
        actions = base.action_buffer().clone()
        for e in (base, diff):
            wall_us(e, actions, warmup)
        pairs = [(wall_us(base, actions, iters), wall_us(diff, actions, iters)) for _ in range(5)]
        step_us[mode] = {'system_capacity': round(statistics.median(p[0] for p in pairs), 2),
                         'difference': round(statistics.median(p[1] for p in pairs), 2),
                         'added': round(statistics.median(p[1] - p[0] for p in pairs), 2)}
        if mode == 'lockstep':
            env = diff
            base.close()
        else:
            base.close(); diff.close()
    m = env._marginal_kernel()
    rec.update(links=m.n, rbs=m.r, law=m.law, out_bytes=2 * b * m.n * 4)
    fns = [lambda: env.marginal_capacity()]
    if baseline:
        fn = torch_formulation(env)
        (rd, rh), (gd, gh) = fn(), env.marginal_capacity()
        rec['torch_vs_kernel_max_abs_mbps'] = {'harm': round(float((rh - gh).abs().max()), 6), 'difference': round(float((rd - gd).abs().max()), 6)}
        del rd, rh
        fns.append(fn)
    times = alternating_us(fns, iters, warmup if not baseline else 3)
    med, lo, hi = times[0]
    rec['marginal_us'] = {'median': round(med, 2), 'min': round(lo, 2), 'max': round(hi, 2)}
    if baseline:
        tm, tl, th = times[1]
        rec['torch_us'] = {'median': round(tm, 2), 'min': round(tl, 2), 'max': round(th, 2)}
        rec['torch_over_kernel'] = round(tm / med, 2)
        torch.cuda.empty_cache()
    rec['step_us'] = step_us
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,stress_hata,config2')
    ap.add_argument('--no-baseline', action='store_true')
    a = ap.parse_args()
    for name in a.configs.split(','):
        print(json.dumps(dict(tool='marginal_cost', iters=a.iters, **run(name, a.iters, a.warmup, not a.no_baseline))), flush=True)


if __name__ == '__main__':
    main()

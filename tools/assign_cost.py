#!/usr/bin/env python3
"""Cost of the optimal one-to-one RB matching (VecD2DEnv.assignment_weights / solve_assignment / assign_rbs, csrc/d2d_assign.hip) on
the GPU; one JSON line per configuration, printed and appended to profiles/assign_cost.jsonl (--out).

    python tools/assign_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--no-baseline] [--out FILE]

stress: 4096 envs x (256 + 256) links x 256 RBs, 1/d^2; config2: BASELINE config 2, 1024 x (25 + 25) links x 25 RBs.  The DUE
links are movable.  In one process, per configuration, device events, median of K after W warm-up calls, all device callables timed
ALTERNATELY (one call of each per round):

  weights_us     one assignment_weights() launch (objective 'total'), and one with the harm plane
  solve_us       one solve_assignment() launch on those weights
  assign_us      assign_rbs(): both launches and the scatter of the columns
  torch_us       the float32 torch formulation of the same weights ([B, M, N] pair terms scattered by RB); inverse-square
                 configurations only; its largest difference from the kernel
  brdyn_us       one best_response_dynamics() call, for scale
  scipy_ms       scipy.optimize.linear_sum_assignment per env on the host, on the downloaded weights, wall clock, where scipy
                 imports (--scipy-envs of them, scaled to the batch); its assignment's value against the kernel's

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/assign_cost.py --no-baseline --out ''`: the
kernels are assign_weights_kernel<law, objective> and assign_solve_kernel<threads> (libd2d_assign.so).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
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
        out.append({'median': round(statistics.median(t), 2), 'min': round(min(t), 2), 'max': round(max(t), 2)})
    return out


def torch_formulation(env, k, links):
    """The 'total' weights in float32 torch ops, inverse-square law: [B, M, R]."""
    t = env._t
    tx, rx = k.tx.long(), k.rx.long()
    cols, cap_cols = k.cols.view(6, k.d), k.cap_cols.view(2, k.d)
    tx_lin, rx_pl, rx_lin, noise = cols[0][tx], cols[1][rx], cols[2][rx], cols[3][rx]
    bw_mhz, sens = cap_cols[0][tx], cap_cols[1][rx]
    mov = torch.zeros(k.n, dtype=torch.bool, device=env.device)
    mov[links.long()] = True
    bg = torch.nonzero(~mov)[:, 0]
    lk = links.long()
    r = k.r

    def cap_of(sig, ix, who):
        sinr = sig / (ix * rx_pl[who] + noise[who])
        return torch.where(10.0 * torch.log10(sinr) > sens[who], bw_mhz[who] * torch.log2(1.0 + sinr), torch.zeros_like(sinr))

    def run():
        dx = t['pos_x'][:, tx, None] - t['pos_x'][:, None, rx]           # [b, j, i]
        dy = t['pos_y'][:, tx, None] - t['pos_y'][:, None, rx]
        g = 1.0 / (dx * dx + dy * dy)
        pw = torch.pow(10.0, t['pwr'].float() / 10.0) * tx_lin           # [b, j]
        mw = pw[:, :, None] * g
        sig = pw * torch.diagonal(g, dim1=1, dim2=2) * rx_pl * rx_lin    # [b, i]
        rb_bg = t['rb'][:, bg].long()
        on = ((rb_bg >= 0) & (rb_bg < r)).float()
        member = torch.nn.functional.one_hot(rb_bg.clamp(0, r - 1), r).float() * on[:, :, None]       # [b, k, r]
        ix_own = torch.einsum('bkr,bka->bar', member, mw[:, bg][:, :, lk])                               # [b, a, r]
        own = cap_of(sig[:, lk, None], ix_own, lk[:, None])
        same = (rb_bg[:, :, None] == rb_bg[:, None, :]).float() * on[:, :, None] * on[:, None, :]
        same = same * (1.0 - torch.eye(len(bg), device=env.device))
        ix_bg = (mw[:, bg][:, :, bg] * same).sum(dim=1)                                                  # [b, k]
        without = cap_of(sig[:, bg], ix_bg, bg)
        with_a = cap_of(sig[:, None, bg], ix_bg[:, None, :] + mw[:, lk][:, :, bg], bg)                  # [b, a, k]
        harm = torch.einsum('bak,bkr->bar', without[:, None, :] - with_a, member)
        return own - harm
    return run


def run(name, iters, warmup, baseline, scipy_envs):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    k = env._assignment_kernel()
    w, links = env.assignment_weights()
    m = int(links.shape[0])
    rec = {'config': name, 'envs': b, 'links': k.n, 'movable': m, 'rbs': k.r, 'law': k.law, 'weights_bytes': 4 * b * m * k.r}
    res = env.assign_rbs()
    torch.cuda.synchronize()
    rec['feasible'] = int(res.feasible.sum())
    rec['value_mbps_mean'] = float(res.value_mbps.double().mean())
    labels = ['weights', 'weights_harm', 'solve', 'assign_rbs']
    fns = [lambda: env.assignment_weights(), lambda: env.assignment_weights(harm=True), lambda: env.solve_assignment(w),
           lambda: env.assign_rbs()]
    if baseline:
        labels.append('best_response_dynamics')
        fns.append(lambda: env.best_response_dynamics())
        if k.law == 0:
            ref = torch_formulation(env, k, links)
            rec['torch_max_abs_diff'] = float((ref() - env.assignment_weights()[0]).abs().max())
            labels.append('torch_weights')
            fns.append(ref)
    times = dict(zip(labels, alternating_us(fns, iters, warmup)))
    rec['weights_us'] = {'total': times['weights'], 'with_harm': times['weights_harm']}
    rec['solve_us'] = times['solve']
    rec['assign_us'] = times['assign_rbs']
    if baseline:
        rec['brdyn_us'] = times['best_response_dynamics']
        if 'torch_weights' in times:
            rec['torch_us'] = times['torch_weights']
        try:
            from scipy.optimize import linear_sum_assignment
        except ImportError:
            rec['scipy_ms'] = None
        else:
            host = env.assignment_weights()[0][:scipy_envs].cpu().numpy().astype(np.float64)
            col = env.solve_assignment(w)[0][:scipy_envs].cpu().numpy()
            t0 = time.perf_counter()
            sol = [linear_sum_assignment(-host[e]) for e in range(len(host))]
            dt = time.perf_counter() - t0
            mine = sum(host[e][np.arange(m), col[e]].sum() for e in range(len(host)))
            theirs = sum(host[e][rows, cols].sum() for e, (rows, cols) in enumerate(sol))
            rec['scipy_ms'] = {'envs_timed': len(host), 'per_env': round(1e3 * dt / len(host), 4), 'batch': round(1e3 * dt / len(host) * b, 2),
                               'value_rel_diff': float(abs(mine - theirs) / abs(theirs))}
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--scipy-envs', type=int, default=64, help='envs the host scipy baseline is timed on (scaled to the batch)')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'assign_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='assign_cost', iters=a.iters, **run(name, a.iters, a.warmup, not a.no_baseline, a.scipy_envs)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Cost of what-if evaluation of candidate joint actions (VecD2DEnv.evaluate, csrc/d2d_evaluate.hip) on the GPU; one JSON line per
configuration, printed and appended to profiles/evaluate_cost.jsonl (--out).

    python tools/evaluate_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--no-baseline] [--out FILE]

stress: 4096 envs x 512 links x 256 RBs, 1/d^2; config2: BASELINE config 2, 1024 x 50 links x 25 RBs.  In one process, per
configuration, device events, median of K after W warm-up calls, all callables timed ALTERNATELY (one call of each per round):

  evaluate_us    one evaluate() launch at K = 1, 4 and 16 candidates per env, totals only (planes=()) and with both planes
  marginal_us    one marginal_capacity() launch (whose phase 1 is one candidate's evaluation)
  step_us        K = 1, 4, 16 calls of step(): what scoring K joint actions took before evaluate() (and it moves the env)
  torch_us       the float32 torch formulation of the same evaluation ([B, K, N, N] pair terms), at the K whose pair block stays
                 below --torch-bytes (default 8 GiB per tensor); inverse-square configurations only
  equal          evaluate() of the env's own planes against the last step's planes, bit for bit; the torch formulation's largest
                 difference from evaluate()

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/evaluate_cost.py --no-baseline --out ''`: the
kernel is evaluate_kernel<law> (libd2d_evaluate.so).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch

from gym_d2d_amd import _native
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
}
KS = (1, 4, 16)


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


def torch_formulation(env, ev):
    """evaluate() in float32 torch ops, inverse-square law: (sinr_db, capacity_mbps [B, K, N], total_mbps [B, K])."""
    t = env._t
    tx, rx = ev.tx.long(), ev.rx.long()
    d = ev.d
    cols, cap_cols = ev.cols.view(6, d), ev.cap_cols.view(2, d)
    tx_lin, rx_pl, rx_lin, noise = cols[0][tx], cols[1][rx], cols[2][rx], cols[3][rx]
    bw_mhz, sens = cap_cols[0][tx], cap_cols[1][rx]
    eye = torch.eye(ev.n, dtype=torch.bool, device=env.device)

    def run(rb, pwr):
        dx = t['pos_x'][:, tx, None] - t['pos_x'][:, None, rx]           # [b, j, i]
        dy = t['pos_y'][:, tx, None] - t['pos_y'][:, None, rx]
        g = 1.0 / (dx * dx + dy * dy)
        pw = torch.pow(10.0, pwr.float() / 10.0) * tx_lin                # [b, k, j]
        same = (rb[:, :, :, None] == rb[:, :, None, :]) & ~eye
        ix = (pw[:, :, :, None] * g[:, None] * same).sum(dim=2)          # [b, k, i]
        sig = pw * torch.diagonal(g, dim1=1, dim2=2)[:, None] * rx_pl * rx_lin
        sinr = sig / (ix * rx_pl + noise)
        sinr_db = 10.0 * torch.log10(sinr)
        cap = torch.where(sinr_db > sens, bw_mhz * torch.log2(1.0 + sinr), torch.zeros_like(sinr))
        return sinr_db, cap, cap.sum(dim=2)
    return run


def run(name, iters, warmup, baseline, torch_bytes):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    actions = env.action_buffer().clone()
    _, _, _, info = env.step(actions)
    ev = env._evaluate_kernel()
    n, r = ev.n, ev.r
    rec = {'config': name, 'envs': b, 'links': n, 'rbs': r, 'law': ev.law, 'chunk': _native.EVALUATE_CHUNK}
    gen = torch.Generator(device=env.device).manual_seed(3)
    planes = {k: (torch.randint(0, r, (b, k, n), generator=gen, device=env.device, dtype=torch.int32),
                  torch.randint(0, 20, (b, k, n), generator=gen, device=env.device, dtype=torch.int32)) for k in KS}
    own = env.evaluate(env._t['rb'].unsqueeze(1).contiguous(), env._t['pwr'].unsqueeze(1).contiguous())
    rec['equal'] = {'sinr_db': bool(torch.equal(own['sinr_db'][:, 0], info['sinr_db'])),
                    'capacity_mbps': bool(torch.equal(own['capacity_mbps'][:, 0], info['capacity_mbps']))}
    labels, fns = [], []
    for k in KS:
        rb, pwr = planes[k]
        labels += [f'evaluate_totals_k{k}', f'evaluate_planes_k{k}']
        fns += [lambda rb=rb, pwr=pwr: env.evaluate(rb, pwr, planes=()), lambda rb=rb, pwr=pwr: env.evaluate(rb, pwr)]
    if baseline:
        labels.append('marginal')
        fns.append(lambda: env.marginal_capacity())
        for k in KS:
            labels.append(f'step_x{k}')
            fns.append(lambda k=k: [env.step(actions) for _ in range(k)])
        if ev.law == 0:
            ref = torch_formulation(env, ev)
            for k in KS:
                if b * k * n * n * 4 <= torch_bytes:
                    rb, pwr = planes[k]
                    got, want = env.evaluate(rb, pwr), ref(rb, pwr)
                    rec.setdefault('torch_max_abs_diff', {})[f'k{k}'] = {
                        'sinr_db': float((got['sinr_db'] - want[0]).abs().max()), 'capacity_mbps': float((got['capacity_mbps'] - want[1]).abs().max())}
                    del got, want
                    labels.append(f'torch_k{k}')
                    fns.append(lambda rb=rb, pwr=pwr: ref(rb, pwr))
    times = dict(zip(labels, alternating_us(fns, iters, warmup)))
    rec['evaluate_us'] = {k: v for k, v in times.items() if k.startswith('evaluate')}
    rec['per_candidate_us'] = {k: round(v['median'] / int(k.rsplit('k', 1)[1]), 2) for k, v in rec['evaluate_us'].items()}
    if baseline:
        rec['marginal_us'] = times['marginal']
        rec['step_us'] = {k: v for k, v in times.items() if k.startswith('step')}
        rec['torch_us'] = {k: v for k, v in times.items() if k.startswith('torch')}
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--torch-bytes', type=int, default=8 << 30, help='largest [B, K, N, N] float32 block the torch formulation may form')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'evaluate_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='evaluate_cost', iters=a.iters, **run(name, a.iters, a.warmup, not a.no_baseline, a.torch_bytes)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

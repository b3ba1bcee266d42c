#!/usr/bin/env python
"""Cost of target-SINR power control (VecD2DEnv.power_control, csrc/d2d_powerctl.hip) on the GPU; one JSON line per configuration,
printed and appended to profiles/power_control_cost.jsonl (--out).

    python tools/power_control_cost.py [--iters K] [--warmup W] [--configs stress,config2] [--out FILE]

Per configuration (state: reset, then one step with the reset's random actions; target: --target-db for every link):
  sweeps           the sweeps the kernel ran per env (mean, max) - the torch formulation below runs max + 1 evaluations
  kernel_us        the launch alone, device events, median of K after W warm-up calls - timed ALTERNATELY with
  torch_us         the float32 torch formulation of the same iteration: per sweep one [B, N, N] pass (pair gains once, outside the
                   timed part's loop only the powers change: gains [B, N, N] float32 are kept, as a user would), run for the same
                   number of sweeps, same final evaluation
  equal            the torch formulation's powers against the kernel's (share of envs that agree; the float32 sums differ in
                   order, so a ceiling may land elsewhere) - a sanity figure, not a test
  actions_us       power_control_actions() end to end (target / mask look-up, launch, encode), host clock around K calls that end
                   in a device synchronise

Every GPU step of a measuring session runs under its own `timeout`, chained with `&&`:
    timeout -k 10 300 python tools/power_control_cost.py --configs stress && timeout -k 10 120 python tools/power_control_cost.py --configs config2
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


def torch_formulation(env, k, target, sweeps, chunk):
    """The same iteration in float32 torch, `sweeps` update sweeps and the final evaluation: per sweep a [chunk, N, N] pass over
    the pair gains, which are computed once (inverse-square law only: the configurations timed here)."""
    t = env._t
    tx, rx = k.tx.long(), k.rx.long()
    cols = k.cols
    lo, hi = k.p_min.float(), k.p_max.float()
    tgt = torch.full((k.n,), float(target), device=env.device)
    eye = torch.eye(k.n, dtype=torch.bool, device=env.device)
    gains = []
    for s in range(0, k.b, chunk):
        px, py = t['pos_x'][s:s + chunk], t['pos_y'][s:s + chunk]
        dx = px[:, tx][:, :, None] - px[:, rx][:, None, :]               # [b, j, i]
        dy = py[:, tx][:, :, None] - py[:, rx][:, None, :]
        g = 1.0 / (dx * dx + dy * dy) * cols[0][tx][None, :, None]
        rb = t['rb'][s:s + chunk]
        g = g * ((rb[:, :, None] == rb[:, None, :]) & ~eye[None])        # interferers: same RB, j != i
        own = (1.0 / ((px[:, tx] - px[:, rx]) ** 2 + (py[:, tx] - py[:, rx]) ** 2)) * cols[0][tx][None] * cols[1][rx][None] * cols[2][rx][None]
        gains.append((g, own))
    rx_pl, noise = cols[1][rx][None], cols[3][rx][None]

    def sinr(p, g, own):
        z = torch.pow(10.0, p / 10.0)
        ix = torch.einsum('bj,bji->bi', z, g)
        return 10.0 * torch.log10(z * own / (ix * rx_pl + noise))

    def run():
        out = []
        for g, own in gains:
            p = lo[None].expand(g.shape[0], -1).clone()
            for _ in range(sweeps):
                need = torch.ceil(p + (tgt - sinr(p, g, own)))
                p = torch.maximum(p, torch.minimum(hi, torch.maximum(lo, need)))
            out.append((p, sinr(p, g, own)))
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    return run


def run(name, iters, warmup, target):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b)
    env.reset(seed=1)
    env.step(env.action_buffer().clone())
    res = env.power_control(target)
    k = env._powerctl
    sweeps = res.iters.float()
    n_sweeps = int(sweeps.max())
    rec = {'config': name, 'envs': b, 'links': k.n, 'rbs': k.r, 'law': k.law, 'target_db': target,
           'sweeps': {'mean': round(float(sweeps.mean()), 2), 'max': n_sweeps}, 'converged': round(float(res.converged.float().mean()), 4)}
    chunk = max(1, min(b, (1 << 28) // (k.n * k.n * 4)))                 # the kept gains: 4 B N^2 bytes in all, passes of <= 256 MB
    fn = torch_formulation(env, k, target, n_sweeps, chunk)
    p_torch, _ = fn()
    rec['equal'] = {'envs_with_equal_powers': round(float((p_torch.int() == res.power_dbm).all(dim=1).float().mean()), 4)}
    rec['torch_gain_bytes'] = 4 * b * k.n * k.n
    times = alternating_us([lambda: env.power_control(target), fn], iters, warmup)
    rec['kernel_us'], rec['torch_us'] = times
    rec['torch_over_kernel'] = round(times[1]['median'] / times[0]['median'], 2)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            env.power_control_actions(target)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / iters * 1e6)
    rec['actions_us'] = round(statistics.median(walls), 2)
    env.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,config2')
    ap.add_argument('--target-db', type=float, default=10.0)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'power_control_cost.jsonl'), help="file the lines are appended to ('' = none)")
    a = ap.parse_args()
    if a.iters < 50:
        ap.error('--iters must be >= 50: the figures are medians of 50 or more')
    for name in a.configs.split(','):
        line = json.dumps(dict(tool='power_control_cost', iters=a.iters, **run(name, a.iters, a.warmup, a.target_db)))
        print(line, flush=True)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()

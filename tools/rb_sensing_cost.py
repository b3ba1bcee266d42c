#!/usr/bin/env python3
"""Cost of per-RB sensing (VecD2DEnv.sense, csrc/d2d_sense.hip) on the GPU; one JSON line per configuration.

    python tools/rb_sensing_cost.py [--iters K] [--warmup W] [--configs stress,config2,stress_hata] [--no-baseline]

stress: 4096 envs x 512 links x 256 RBs (2.1 GB out); config2: BASELINE config 2, 1024 x 50 links x 25 RBs; stress_hata: stress
with COST-Hata urban (the pow-k law).  In one process, per configuration:

  sense_us       the sensing launch alone, median of K device-event timings after W warm-up calls, with its bytes / time as a
                 fraction of 8 TB/s and of the best store-only kernel this box runs (tools/write_probe.py, same process)
  torch_us       the same block computed the way a user had to before: gain cube [B, N, N] from the same columns in float32 torch,
                 bmm with the one-hot [B, N, R] of the RB plane, then the SINR
  step_us        step() with RbSensingObsFunction against step() with SignalPlanesObsFunction (K synchronised steps each, wall clock)

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/rb_sensing_cost.py --no-baseline`: the
kernel is sense_kernel<law, what> (libd2d_sense.so).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import torch

from gym_d2d_amd.envs import RbSensingObsFunction, VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss


class UrbanHata(CostHataPathLoss):
    def __init__(self, f):
        super().__init__(f, AreaType.URBAN)


CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
    'stress_hata': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256, 'path_loss_model': UrbanHata}, 4096),
}


def event_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(t), min(t), max(t)


def torch_formulation(env):
    """sense('sinr_db') rebuilt in float32 torch from the sensor's own columns (what a user had to write before)."""
    s, t = env._rb_sensor(), env._t
    tx, rx, cols = s.tx.long(), s.rx.long(), s.cols
    n, r = s.n, s.r
    eye = torch.eye(n, dtype=torch.bool, device=env.device)
    expo = None
    if s.law != 0:
        expo = torch.as_tensor(env.simulator.path_loss_table.law['exponent'], dtype=torch.float32, device=env.device)[tx]

    def run():
        px, py = t['pos_x'], t['pos_y']
        dx = px[:, tx, None] - px[:, None, rx]
        dy = py[:, tx, None] - py[:, None, rx]
        d2 = dx * dx + dy * dy                                                 # [B, j, i]
        gain = 1.0 / d2 if expo is None else d2 ** (-0.5 * expo)[None, :, None]
        pw = torch.pow(10.0, t['pwr'].float() / 10.0) * cols[0][tx][None, :]   # [B, j]
        g = (gain * pw[:, :, None]).masked_fill(eye[None], 0.0)
        onehot = torch.nn.functional.one_hot(t['rb'].long(), r).float()        # [B, j, r]
        ix = torch.bmm(g.transpose(1, 2), onehot)                              # [B, i, r]
        sig = (pw * torch.diagonal(gain, dim1=1, dim2=2)) * (cols[1][rx] * cols[2][rx])[None, :]
        return 10.0 * torch.log10(sig[:, :, None] / (ix * cols[1][rx][None, :, None] + cols[3][rx][None, :, None]))
    return run


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, iters, warmup, baseline, ceiling):
    cfg, b = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, obs_fn=SignalPlanesObsFunction), num_envs=b, reward_per_env=True)
    env.reset(seed=1)
    n, r = env.num_links, cfg['num_rbs']
    nbytes = b * n * r * 4
    med, lo, hi = event_us(lambda: env.sense('sinr_db'), iters, warmup)
    rec = {'config': name, 'envs': b, 'links': n, 'rbs': r, 'out_bytes': nbytes, 'law': env._rb_sensor().law,
           'sense_us': {'median': round(med, 2), 'min': round(lo, 2), 'max': round(hi, 2)},
           'sense_gb_s': round(nbytes / med / 1e3, 1), 'fraction_of_8tb_s': round(nbytes / med / 1e3 / 8000, 3)}
    if ceiling:
        rec['box_write_ceiling_gb_s'] = round(ceiling, 1)
        rec['fraction_of_write_ceiling'] = round(nbytes / med / 1e3 / ceiling, 3)
    if baseline:
        fn = torch_formulation(env)
        ref, got = fn(), env.sense('sinr_db')
        rec['torch_vs_kernel_max_abs_db'] = round(float((ref - got).abs().max()), 6)
        del ref
        tm, tl, th = event_us(fn, max(3, iters // 5), 2)
        rec['torch_us'] = {'median': round(tm, 2), 'min': round(tl, 2), 'max': round(th, 2)}
        rec['torch_over_kernel'] = round(tm / med, 2)
        torch.cuda.empty_cache()
    actions = env.action_buffer().clone()
    sens = VecD2DEnv(dict(cfg, obs_fn=RbSensingObsFunction), num_envs=b, reward_per_env=True)
    sens.reset(seed=1)
    for e in (env, sens):
        wall_us(e, actions, warmup)
    pairs = [(wall_us(env, actions, iters), wall_us(sens, actions, iters)) for _ in range(5)]
    rec['step_us'] = {'signal_planes': round(statistics.median(p[0] for p in pairs), 2),
                      'rb_sensing': round(statistics.median(p[1] for p in pairs), 2),
                      'added': round(statistics.median(p[1] - p[0] for p in pairs), 2)}
    env.close(); sens.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='stress,config2,stress_hata')
    ap.add_argument('--no-baseline', action='store_true')
    a = ap.parse_args()
    ceiling = 0.0
    try:
        import write_probe
        ceiling = float(write_probe.write_variants(1 << 31, 5)[0])
    except Exception as e:      # the probe library is measurement equipment: report without it
        print(json.dumps({'tool': 'rb_sensing_cost', 'write_probe': f'unavailable: {e}'}), file=sys.stderr)
    for name in a.configs.split(','):
        print(json.dumps(dict(tool='rb_sensing_cost', iters=a.iters, **run(name, a.iters, a.warmup, not a.no_baseline, ceiling))), flush=True)


if __name__ == '__main__':
    main()

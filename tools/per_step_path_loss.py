#!/usr/bin/env python3
"""Cost of a per-step ArrayPathLoss against the built-in ShadowingPathLoss, on the GPU; one JSON line.

    python tools/per_step_path_loss.py [--steps K] [--warmup W] [--configs config2,full]

For each configuration - BASELINE config 2 (1024 envs x 25 RBs / 25 CUEs / 25 DUE pairs, LinearObs) and 4096 x 512 obs-less
with reward_per_env=True - it times VecD2DEnv.step (ms per step, wall, synchronised) with the built-in model and with
PerStepShadowing (the same model written as a user's per-step ArrayPathLoss around view.normal()), and splits the plugin's step
by HIP events into the user's compute (torch, d2d_plugin_normal included), the d2d_plugin_normal fills alone and the step kernel
(the library's own event timing of the mode-5 launch).  For the per-kernel view run it under
`rocprofv3 --kernel-trace --stats -- python tools/per_step_path_loss.py --steps 20 --warmup 5`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np
import torch

from gym_d2d_amd import _native
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import ArrayPathLoss, ShadowingPathLoss, pl_constant_dB


class PerStepShadowing(ArrayPathLoss):
    per_step = True

    def __init__(self, carrier_freq_GHz, ple=2.0, d0_m=100.0, chi_dB=2.7):
        super().__init__(carrier_freq_GHz)
        self.ple, self.d0_m, self.chi_dB = float(ple), float(d0_m), float(chi_dB)
        self.const = pl_constant_dB(carrier_freq_GHz, ple)

    def compute(self, view):
        xp, d = view.xp, view.distance()
        base = 10 * self.ple * xp.log10(d) + self.const
        pl = base + self.chi_dB * xp.where(d > self.d0_m, view.normal(0), 0.0)
        dd = xp.diagonal(d, dim1=1, dim2=2)
        return pl, xp.diagonal(base, dim1=1, dim2=2) + self.chi_dB * xp.where(dd > self.d0_m, view.normal(1), 0.0)


CONFIGS = {
    'config2': (dict(num_rbs=25, num_cues=25, num_due_pairs=25), 1024, {}),
    'full': (dict(num_rbs=256, num_cues=256, num_due_pairs=256, obs_fn=SignalPlanesObsFunction), 4096, dict(reward_per_env=True)),
}


def ev_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def run(name, model, steps, warmup):
    cfg, b, kw = CONFIGS[name]
    env = VecD2DEnv(dict(cfg, path_loss_model=model, seed=11), num_envs=b, **kw)
    env.reset(seed=3)
    acts = env.action_buffer().clone()
    for _ in range(warmup):
        env.step(acts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(acts)
    torch.cuda.synchronize()
    out = {'ms_per_step': (time.perf_counter() - t0) / steps * 1e3}
    sim, h = env.simulator, env.simulator.handle
    h.profile_enable(True); h.profile_reset()
    for _ in range(max(steps // 2, 5)):
        env.step(acts)
    torch.cuda.synchronize()
    out['step_kernel_ms'] = h.profile_median(0)
    h.profile_enable(False)
    if getattr(model, 'per_step', False):
        out['compute_ms'] = ev_ms(sim.prepare_step, max(steps // 2, 5))            # the user's compute into the live table
        n = env.num_links
        buf = torch.empty((b, n, n), dtype=torch.float64, device=env.device)
        stream = torch.cuda.current_stream().cuda_stream
        out['plugin_normal_kind0_ms'] = ev_ms(lambda: _native.plugin_normal(buf.data_ptr(), _native.F64, b, 0, n, n, 1, 0, 5, stream), 10)
        out['plugin_normal_kind0_GBs'] = buf.numel() * 8 / out['plugin_normal_kind0_ms'] / 1e6
        out['plugin_normal_kind0_of_8TBs_peak'] = out['plugin_normal_kind0_GBs'] / 8000.0
        del buf
    assert env.status_flags() & (_native.FLAG_ZERO_DISTANCE | _native.FLAG_PATH_LOSS_DOMAIN) == 0
    env.close()
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--configs', default='config2,full')
    args = ap.parse_args()
    res = {'tool': 'per_step_path_loss', 'steps': args.steps}
    for name in args.configs.split(','):
        res[name] = {'builtin_shadowing': run(name, ShadowingPathLoss, args.steps, args.warmup),
                     'per_step_shadowing': run(name, PerStepShadowing, args.steps, args.warmup)}
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()

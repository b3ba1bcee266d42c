#!/usr/bin/env python3
"""Cost of the neighbour graph (VecD2DEnv.coupling / neighbors, NeighborObsFunction, csrc/d2d_graph.hip) on the GPU; one JSON line
per configuration.

    python tools/neighbors_cost.py [--iters K] [--warmup W] [--k 8] [--configs stress,config2,stress_hata,config2_hata]

stress: 4096 envs x 512 links; config2: BASELINE config 2, 1024 x 50 links; *_hata: the same with COST-Hata urban (the pow-k law).
In one process, per configuration, medians of K device-event timings after W warm-up calls, kernel and torch timed alternately:

  coupling / neighbors / neighbor_obs   each kernel alone, with its algorithmic bytes (what it must write, plus what the gather must
                 read) over its time as a fraction of 8 TB/s and of the best store-only kernel this box runs (tools/write_probe.py)
  torch_select   the selection a user had to write before: the [B, N, N] float32 cube from the same columns, then topk
  torch_obs      the per-step observation a user had to write before: gathers of the planes through the lists, stack and cat
  step_us        step() with NeighborObsFunction against step() with SignalPlanesObsFunction, with and without autoreset (K
                 synchronised steps each, wall clock, five alternating rounds)

For the per-kernel view run it under `rocprofv3 --kernel-trace --stats -- python tools/neighbors_cost.py --no-baseline`: the kernels
are coupling_kernel<law, vec>, neighbors_kernel<law>, neighbor_obs_kernel (libd2d_graph.so).
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

from gym_d2d_amd.envs import NeighborObsFunction, VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss


class UrbanHata(CostHataPathLoss):
    def __init__(self, f):
        super().__init__(f, AreaType.URBAN)


CONFIGS = {
    'stress': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256}, 4096),
    'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 1024),
    'stress_hata': ({'num_rbs': 256, 'num_cues': 256, 'num_due_pairs': 256, 'path_loss_model': UrbanHata}, 4096),
    'config2_hata': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25, 'path_loss_model': UrbanHata}, 1024),
}


def alternating_us(fns, iters, warmup):
    """{name: (median, min, max) us} of device-event timings, the functions taken in turn inside every round."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for name in fns}
    for r in range(iters):
        for name, fn in fns.items():
            a, b = ev[name][r]
            a.record(); fn(); b.record()
    torch.cuda.synchronize()
    out = {}
    for name in fns:
        t = [a.elapsed_time(b) * 1e3 for a, b in ev[name]]
        out[name] = {'median': round(statistics.median(t), 2), 'min': round(min(t), 2), 'max': round(max(t), 2)}
    return out


def torch_formulation(env, k):
    """(select, obs): the selection and the per-step observation rebuilt in float32 torch from the graph's own columns."""
    g, t = env._neighbor_graph(), env._t
    tx, rx, cols = g.tx.long(), g.rx.long(), g.cols
    b, n = g.b, g.n
    expo = None
    if g.law != 0:
        expo = torch.as_tensor(env.simulator.path_loss_table.law['exponent'], dtype=torch.float32, device=env.device)[tx]
    eye = torch.eye(n, dtype=torch.bool, device=env.device)
    state = {}

    def select():
        px, py = t['pos_x'], t['pos_y']
        dx = px[:, None, tx] - px[:, rx, None]                                  # [B, i, j]
        dy = py[:, None, tx] - py[:, rx, None]
        d2 = dx * dx + dy * dy
        gain = 1.0 / d2 if expo is None else d2 ** (-0.5 * expo)[None, None, :]
        c = 10.0 * torch.log10(gain * cols[0][tx][None, None, :] * cols[1][rx][None, :, None])
        state['vals'], state['idx'] = torch.topk(c.masked_fill(eye[None], float('-inf')), k, dim=2)
        return state['vals'], state['idx']

    def obs():
        j = state['idx'].view(b, n * k)
        own = torch.stack([t['rb'].float(), t['pwr'].float(), t['sinr_db'], t['snr_db']], dim=-1)[:, :, None, :]
        nb = torch.stack([state['vals'], torch.gather(t['rb'], 1, j).view(b, n, k).float(), torch.gather(t['pwr'], 1, j).view(b, n, k).float(),
                          torch.gather(t['sinr_db'], 1, j).view(b, n, k)], dim=-1)
        return torch.cat([own, nb], dim=2).view(b, n, 4 * (k + 1))
    return select, obs


def wall_us(env, actions, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step(actions)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def run(name, k, iters, warmup, baseline, ceiling):
    cfg, b = CONFIGS[name]

    class Fn(NeighborObsFunction):
        pass
    Fn.k = k
    env = VecD2DEnv(dict(cfg, obs_fn=Fn), num_envs=b, reward_per_env=True)
    env.reset(seed=1)
    n, g = env.num_links, env._neighbor_graph()
    idx, cdb = env._neighbors
    nbytes = {'coupling': 4 * b * n * n, 'neighbors': 8 * b * n * k, 'neighbor_obs': 16 * b * n * (k + 1) + 8 * b * n * k}
    fns = {'coupling': env.coupling, 'neighbors': lambda: env.neighbors(k),
           'neighbor_obs': lambda: g.obs_torch(env._t, k, idx, cdb, env._stream_ptr)}
    if baseline:
        select, obs = torch_formulation(env, k)
        vals, tidx = select()
        rec_check = {'torch_vs_kernel_values_max_abs_db': round(float((vals - cdb).abs().max()), 6),
                     'torch_vs_kernel_idx_differ': round(float((tidx != idx).float().mean()), 6),
                     'torch_vs_kernel_obs_max_abs': round(float((obs() - fns['neighbor_obs']()).abs().nan_to_num(0.0).max()), 6)}
        fns.update(torch_select=select, torch_obs=obs)
    times = alternating_us(fns, iters, warmup)
    rec = {'config': name, 'envs': b, 'links': n, 'k': k, 'law': g.law}
    for w, nb in nbytes.items():
        gbs = nb / times[w]['median'] / 1e3
        rec[w] = dict(us=times[w], bytes=nb, gb_s=round(gbs, 1), fraction_of_8tb_s=round(gbs / 8000, 3))
        if ceiling:
            rec[w]['fraction_of_write_ceiling'] = round(gbs / ceiling, 3)
    if ceiling:
        rec['box_write_ceiling_gb_s'] = round(ceiling, 1)
    if baseline:
        rec.update(rec_check)
        rec['torch_select_us'], rec['torch_obs_us'] = times['torch_select'], times['torch_obs']
        rec['torch_select_over_neighbors'] = round(times['torch_select']['median'] / times['neighbors']['median'], 2)
        rec['torch_obs_over_neighbor_obs'] = round(times['torch_obs']['median'] / times['neighbor_obs']['median'], 2)
    env._graph.own.pop('coupling', None)                 # the cube is not part of a step: give it back before the step timings
    torch.cuda.empty_cache()
    actions = env.action_buffer().clone()
    rec['step_us'] = {}
    for auto in (False, True):
        envs = [VecD2DEnv(dict(cfg, obs_fn=fn), num_envs=b, reward_per_env=True, autoreset=auto) for fn in (SignalPlanesObsFunction, Fn)]
        for e in envs:
            e.reset(seed=1)
            wall_us(e, actions, warmup)
        pairs = [tuple(wall_us(e, actions, iters) for e in envs) for _ in range(5)]
        rec['step_us']['autoreset' if auto else 'lockstep'] = {
            'signal_planes': round(statistics.median(p[0] for p in pairs), 2), 'neighbor_obs': round(statistics.median(p[1] for p in pairs), 2),
            'added': round(statistics.median(p[1] - p[0] for p in pairs), 2)}
        for e in envs:
            e.close()
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--k', type=int, default=8)
    ap.add_argument('--configs', default='stress,config2,stress_hata,config2_hata')
    ap.add_argument('--no-baseline', action='store_true')
    a = ap.parse_args()
    ceiling = 0.0
    try:
        import write_probe
        ceiling = float(write_probe.write_variants(1 << 31, 5)[0])
    except Exception as e:      # the probe library is measurement equipment: report without it
        print(json.dumps({'tool': 'neighbors_cost', 'write_probe': f'unavailable: {e}'}), file=sys.stderr)
    for name in a.configs.split(','):
        print(json.dumps(dict(tool='neighbors_cost', iters=a.iters, **run(name, a.k, a.iters, a.warmup, not a.no_baseline, ceiling))), flush=True)


if __name__ == '__main__':
    main()

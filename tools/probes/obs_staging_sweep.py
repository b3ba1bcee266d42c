#!/usr/bin/env python3
"""The bounded sweep behind plan_obs's default for the flat LinearObs kernels (single-trip staging):

    block {1024, 512} x pieces per workgroup {2, 3, 4} x store policy {1 nt, 5 sc1 nt}, float32 and float64,
    and with --arms the values of D2D_TUNE_OBS_VARIANT to set side by side (e.g. --arms flat=0,rows=3; a tree under experiment
    adds its own: profiles/r8_obs_preload_sweep.jsonl is new=0,parent=4,preload=5,dma=6 of the tree that had those arms),

interleaved rounds in ONE process at 4096 envs x 512 links, the obs kernel's own time from the library's per-launch events.
Policy 5 needs a diagnostic build wherever it is no release value (include/d2d_hip_diag.h).  One JSON line per shape, sorted
by dtype, shape and median; `--out file` appends them (profiles/r7_obs_staging_sweep.jsonl is this).

    python tools/probes/obs_staging_sweep.py [--rounds 5] [--launches 10] [--arms NAME=VARIANT,...] [--sweep LABEL] [--out FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
import torch

from gym_d2d_amd import _native, build
from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import LinearObsFunction


def obs_us(h, acts, launches):
    h.profile_reset(); h.profile_enable(True)
    for k in range(launches):
        h.step(acts[k % acts.shape[0]].data_ptr())
    ms, n = h.profile_read(1)
    h.profile_enable(False)
    return ms / max(n, 1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--links', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--arms', default='', help='comma list name=D2D_TUNE_OBS_VARIANT value, interleaved with the shapes (diagnostic build)')
    ap.add_argument('--sweep', default='obs_single_trip_staging', help="the records' label")
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    b, n = a.envs, a.links
    cfg = {'num_rbs': n // 2, 'num_cues': n // 2, 'num_due_pairs': n // 2, 'obs_fn': LinearObsFunction}
    envs = {'float32': VecD2DEnv(dict(cfg), num_envs=b), 'float64': VecD2DEnv(dict(cfg, obs_dtype='float64'), num_envs=b)}
    for e in envs.values():
        e.reset(seed=1)
    dev = next(iter(envs.values())).device
    acts = torch.randint(0, (n // 2) * 21, (8, b, n), device=dev, dtype=torch.int32)
    arms = [(k, int(v)) for k, v in (kv.split('=') for kv in a.arms.split(',') if kv)] or [('', None)]
    shapes = [(dt, blk, pieces, pol, arm) for blk in (1024, 512) for pieces in (2, 3, 4) for pol in (1, 5) for dt in envs for arm in arms]
    times = {s: [] for s in shapes}
    for rnd in range(a.rounds + 1):                       # round 0 warms every shape up and is dropped
        for s in shapes:
            dt, blk, pieces, pol, (arm, variant) = s
            h = envs[dt].simulator.handle
            if variant is not None:
                h.set_tuning(_native.TUNE_OBS_VARIANT, variant)
            h.set_tuning(_native.TUNE_OBS_BLOCK, blk)
            h.set_tuning(_native.TUNE_OBS_ROWS_PER_WG, pieces)
            h.set_tuning(_native.TUNE_OBS_NONTEMPORAL, pol)
            t = obs_us(h, acts, a.launches)
            if rnd:
                times[s].append(t)
    digest = build.source_digest()
    recs = []
    for s in shapes:
        dt, blk, pieces, pol, (arm, variant) = s
        med = statistics.median(times[s])
        nbytes = b * n * 6 * n * (8 if dt == 'float64' else 4)
        recs.append({'sweep': a.sweep, 'envs': b, 'links': n, 'dtype': dt, 'block': blk, 'pieces': pieces, 'policy': pol,
                     **({'arm': arm, 'variant': variant} if variant is not None else {}),
                     'median_us': round(med, 1), 'min_us': round(min(times[s]), 1), 'max_us': round(max(times[s]), 1),
                     'TBps': round(nbytes / med / 1e6, 3), 'rounds': len(times[s]), 'launches_per_round': a.launches,
                     'source_digest': digest})
    for r in sorted(recs, key=lambda r: (r['dtype'], r['block'], r['pieces'], r['policy'], r['median_us'])):
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    for e in envs.values():
        e.close()


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate the difference-reward fixtures by RUNNING the reference, one step per link with that link's entry removed.

Usage (build container only - the reference does not exist on the GPU box):

    python tests/golden/make_marginal_golden.py       # rewrites tests/golden/marginal_case*.npz

Same approach as make_rb_sensing_golden.py (make_golden.py's gym stub and helpers, the same two small configs): reset the
reference's env, round the positions to float32, call the reference's Simulator.step once with every action and N times with ONE
link's entry removed from the actions, and keep the sum of capacity_mbps over the links that remain: g_without[i].  DATA ONLY is
stored: device configs, positions, the link list, every link's (rb, tx power) and the reference's numbers.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg            # noqa: E402


def run_case(gym, name, seed, env_config, pl):
    from gym_d2d.actions import Actions
    mg.seed_all(gym, seed)
    env = gym.make('D2DEnv-v0', env_config=dict(env_config))
    env.reset()
    mg.round_positions(env)
    mg.recompute_after_reset(env)
    base = dict(env.actions.data)
    keys = list(base.keys())
    n = len(keys)
    full = env.simulator.step(Actions(dict(base)))['capacity_mbps']
    capacity = np.asarray([full[k] for k in keys])
    assert np.array_equal(capacity, np.asarray([env.state['capacity_mbps'][k] for k in keys]))
    g_without = np.empty(n)
    for i, key in enumerate(keys):
        rest = env.simulator.step(Actions({k: v for k, v in base.items() if k != key}))['capacity_mbps']
        assert key not in rest and len(rest) == n - 1
        g_without[i] = sum(rest[k] for k in keys if k != key)
    ids, pos, cfgs, is_bs = mg.snapshot_devices(env)
    meta = dict(mg.env_meta(env, pl), seed=seed, case=name, dev_ids=ids, dev_cfgs=cfgs, keys=[f'{t}:{r}' for t, r in keys])
    out = HERE / f'{name}.npz'
    np.savez_compressed(out, dev_pos=pos, dev_is_bs=is_bs, rb=np.asarray([base[k].rb for k in keys], dtype=np.int64),
                        pwr=np.asarray([base[k].tx_pwr_dBm for k in keys], dtype=np.int64),
                        link_type=np.asarray([base[k].link_type.value for k in keys], dtype=np.int64),
                        capacity_mbps=capacity, g_without=g_without,
                        meta_json=np.frombuffer(json.dumps(meta, default=str).encode(), dtype=np.uint8))
    print(f'wrote {out.name}: {n} links, {out.stat().st_size} bytes')


def main():
    gym = mg.import_reference()
    from gym_d2d.path_loss import AreaType, CostHataPathLoss
    small = {'num_rbs': 4, 'num_cues': 5, 'num_due_pairs': 5}
    run_case(gym, 'marginal_case01', 201, small, {'kind': 'log_distance', 'ple': 2.0})

    class UrbanHata(CostHataPathLoss):
        def __init__(self, f):
            super().__init__(f, AreaType.URBAN)
    run_case(gym, 'marginal_case02', 202, dict(small, path_loss_model=UrbanHata), {'kind': 'cost_hata', 'area': 'urban'})


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Generate the per-RB sensing fixtures by RUNNING the reference, one counterfactual step per (link, RB).

Usage (build container only - the reference does not exist on the GPU box):

    python tests/golden/make_rb_sensing_golden.py       # rewrites tests/golden/rb_sensing_case*.npz

Same approach as make_golden.py (whose gym stub and helpers it imports): reset the reference's env, round the positions to
float32, then call the reference's Simulator.step N * R times on that one layout, each time with ONE link's RB changed to r and
everything else as the reset left it, and keep that link's sinrs_db entry: sinr_db[i, r].  DATA ONLY is stored: device configs,
positions, the link list, every link's (rb, tx power) and the reference's numbers.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden as mg            # noqa: E402


def run_case(gym, name, seed, env_config, pl):
    from gym_d2d.actions import Action, Actions
    mg.seed_all(gym, seed)
    env = gym.make('D2DEnv-v0', env_config=dict(env_config))
    env.reset()
    mg.round_positions(env)
    mg.recompute_after_reset(env)
    base = dict(env.actions.data)
    keys = list(base.keys())
    n, r_total = len(keys), env.simulator.config.num_rbs
    step_sinr = np.asarray([env.state['sinrs_db'][k] for k in keys])
    sinr = np.empty((n, r_total))
    for i, key in enumerate(keys):
        a = base[key]
        for r in range(r_total):
            acts = Actions({k: (Action(a.tx, a.rx, a.link_type, r, a.tx_pwr_dBm) if k == key else v) for k, v in base.items()})
            sinr[i, r] = env.simulator.step(acts)['sinrs_db'][key]
    rb = np.asarray([base[k].rb for k in keys], dtype=np.int64)
    assert np.array_equal(sinr[np.arange(n), rb], step_sinr)       # the column of a link's own RB is the plain step
    ids, pos, cfgs, is_bs = mg.snapshot_devices(env)
    meta = dict(mg.env_meta(env, pl), seed=seed, case=name, dev_ids=ids, dev_cfgs=cfgs, keys=[f'{t}:{r}' for t, r in keys])
    out = HERE / f'{name}.npz'
    np.savez_compressed(out, dev_pos=pos, dev_is_bs=is_bs, rb=rb,
                        pwr=np.asarray([base[k].tx_pwr_dBm for k in keys], dtype=np.int64),
                        link_type=np.asarray([base[k].link_type.value for k in keys], dtype=np.int64),
                        step_sinr_db=step_sinr, sinr_db=sinr,
                        meta_json=np.frombuffer(json.dumps(meta, default=str).encode(), dtype=np.uint8))
    print(f'wrote {out.name}: {n} links x {r_total} RBs, {out.stat().st_size} bytes')


def main():
    gym = mg.import_reference()
    from gym_d2d.path_loss import AreaType, CostHataPathLoss
    small = {'num_rbs': 4, 'num_cues': 5, 'num_due_pairs': 5}
    run_case(gym, 'rb_sensing_case01', 201, small, {'kind': 'log_distance', 'ple': 2.0})

    class UrbanHata(CostHataPathLoss):
        def __init__(self, f):
            super().__init__(f, AreaType.URBAN)
    run_case(gym, 'rb_sensing_case02', 202, dict(small, path_loss_model=UrbanHata), {'kind': 'cost_hata', 'area': 'urban'})


if __name__ == '__main__':
    main()

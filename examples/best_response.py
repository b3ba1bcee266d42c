"""Best-response resource-block choice on the GPU: every round, every DUE pair that would gain more than MIN_GAIN_DB moves to the RB on
which it would see the highest SINR (VecD2DEnv.best_response_actions(): one launch of csrc/d2d_bestrb.hip, no [B, N, R] block), the
CUEs keep the RBs their traffic model gave them.  Half of the pairs may move per round - all of them moving at once chase each other
onto the same quiet RBs.  Prints the system capacity (sum of the links' capacities, mean over the envs) per round beside uniformly
random actions on the same layouts."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, ROUNDS, MIN_GAIN_DB = 256, 16, 16, 48, 8, 0.5
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)                                                    # the reset's step: uniformly random DUE actions
gen = torch.Generator(device=env.device).manual_seed(7)
actions = torch.randint(0, RBS * levels, (NUM_ENVS, DUES), generator=gen, device=env.device, dtype=torch.int32)
_, _, _, info = env.step(actions)
random_capacity = float(info['capacity_mbps'].sum(dim=1).mean())
print(f'system capacity, mean of {NUM_ENVS} envs x {CUES + DUES} links on {RBS} RBs')
print(f'  random actions          {random_capacity:9.1f} Mbps')

link = torch.arange(CUES + DUES, device=env.device)
every_rb = torch.ones((CUES + DUES, RBS), dtype=torch.bool, device=env.device)
capacities, movers = [], []
for k in range(ROUNDS):
    allowed = every_rb & (link % 2 == k % 2)[:, None]               # the other half has no allowed RB: best_rb -1, nobody moves
    before = info['rb'].clone()
    _, _, _, info = env.step(env.best_response_actions(allowed=allowed, min_gain_db=MIN_GAIN_DB))
    capacities.append(float(info['capacity_mbps'].sum(dim=1).mean()))
    movers.append(float((info['rb'] != before).sum(dim=1).float().mean()))
    print(f'  best response, round {k + 1}  {capacities[-1]:9.1f} Mbps   ({movers[-1]:.1f} links moved per env)')
best_response_capacity = capacities[-1]
env.close()

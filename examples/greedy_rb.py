"""Best-response resource-block choice from per-RB sensing: every DUE pair repeatedly moves to the RB on which it would see the
highest SINR (argmax_r of VecD2DEnv.sense()), the CUEs keep the RBs their traffic model gave them.  Prints the system capacity
(sum of the links' capacities, mean over the envs) against uniformly random actions on the same layouts."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, ROUNDS = 256, 16, 16, 48, 8
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)                                                    # the reset's step: uniformly random DUE actions
gen = torch.Generator(device=env.device).manual_seed(7)
actions = torch.randint(0, RBS * levels, (NUM_ENVS, DUES), generator=gen, device=env.device, dtype=torch.int32)
_, _, _, info = env.step(actions)
random_capacity = float(info['capacity_mbps'].sum(dim=1).mean())

# best response, half of the DUE pairs per round (all of them moving at once chase each other onto the same quiet RBs)
power = actions % levels
for k in range(ROUNDS):
    best = env.sense('sinr_db')[:, CUES:, :].argmax(dim=2).to(torch.int32)          # [B, DUES]: each pair's best RB as things stand
    movers = (torch.arange(DUES, device=env.device) % 2 == k % 2)[None, :]
    rb = torch.where(movers, best, actions // levels)
    actions = rb * levels + power
    _, _, _, info = env.step(actions)
greedy_capacity = float(info['capacity_mbps'].sum(dim=1).mean())
env.close()
print(f'system capacity, mean of {NUM_ENVS} envs x {CUES + DUES} links on {RBS} RBs: random {random_capacity:.1f} Mbps, '
      f'greedy best response after {ROUNDS} rounds {greedy_capacity:.1f} Mbps')

"""The interference-graph observation: every agent sees its own link and the K transmitters that couple most strongly into its
receiver (NeighborObsFunction), 4 (K + 1) floats whatever the number of links - against the 6 N of LinearObsFunction.  Runs a few
autoreset steps and prints, for one DUE pair, who its strongest interferers are and what they last did."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import NeighborObsFunction, VecD2DEnv

NUM_ENVS, RBS, CUES, DUES, STEPS = 256, 16, 16, 48, 25


class Neighbor4(NeighborObsFunction):
    k = 4                                                            # obs functions are instantiated without arguments: subclass for another K


env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': Neighbor4}, num_envs=NUM_ENVS, autoreset=True)
k = Neighbor4.k
obs = env.reset(seed=7, elapsed=torch.arange(NUM_ENVS) % 10)         # staggered episodes: some env resets on every step
gen = torch.Generator(device=env.device).manual_seed(7)
high = RBS * env.num_pwr_actions['due']
for _ in range(STEPS):
    actions = torch.randint(0, high, (NUM_ENVS, CUES + DUES), generator=gen, device=env.device, dtype=torch.int32)
    obs, rewards, dones, info = env.step(actions)                    # the lists of the envs this step reset were re-selected
obs_shape = tuple(obs.shape)
idx, coupling_db = env.neighbors(k)                                  # [B, N, K], row [b, i] belongs to the RECEIVING link i
b, i = 0, CUES                                                       # env 0, the first DUE pair
row = obs[b, i].view(k + 1, 4).cpu()
print(f'observation {obs_shape} (LinearObsFunction: {(NUM_ENVS, CUES + DUES, 6 * (CUES + DUES))})')
print(f'env {b}, link {i}: rb {int(row[0, 0])}, {row[0, 1]:.0f} dBm, sinr {row[0, 2]:.1f} dB, snr {row[0, 3]:.1f} dB; strongest interferers:')
for m in range(k):
    print(f'  link {int(idx[b, i, m]):3d}: coupling {row[1 + m, 0]:7.1f} dB, rb {int(row[1 + m, 1])}, {row[1 + m, 2]:.0f} dBm, '
          f'sinr {row[1 + m, 3]:.1f} dB' + ('   <- same RB' if row[1 + m, 1] == row[0, 0] else ''))
env.close()

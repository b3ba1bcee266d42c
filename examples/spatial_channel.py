"""A spatially consistent channel: SpatialChannelPathLoss (csrc/d2d_channel.hip) gives every device pair a power-law median, a
log-normal shadow that is a smooth function of where the two devices stand, and Rayleigh block fading drawn afresh every step.
Follows one DUE pair of a mobile env over an episode: the shadow drifts as the pair moves (and would stand still if it did), the
fading is independent from step to step.  Two envs with the same seeds - one without fading - separate the two terms."""
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.mobility import GaussMarkovMobility
from gym_d2d_amd.path_loss import SpatialChannelPathLoss, pl_constant_dB

NUM_ENVS, RBS, CUES, DUES, STEPS, PLE = 16, 8, 8, 24, 10, 3.5


class Urban(SpatialChannelPathLoss):                                 # the reference's plugin construction: a class, configured here
    median_kwargs = {'ple': PLE}
    shadow_std_dB = 8.0
    decorrelation_m = 20.0
    fading = 'rayleigh'


class UrbanShadowOnly(Urban):
    fading = None


def make(model):
    env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'path_loss_model': model}, num_envs=NUM_ENVS,
                    mobility=GaussMarkovMobility(speed_std_mps=2.0, memory=0.8))
    env.reset(seed=7)
    return env


full, shadow_only = make(Urban), make(UrbanShadowOnly)               # same seeds: same positions, same shadow
actions = full.action_buffer().clone()
pair = CUES                                                          # link index of the first DUE pair
const = pl_constant_dB(full.config.carrier_freq_GHz, PLE)
print(f'{NUM_ENVS} envs x {CUES + DUES} links; env 0, DUE pair 0 (shadow: sigma 8 dB, decorrelation 20 m):')
print('  step  distance m  median dB  shadow dB  fading dB    sinr dB')
for step in range(1, STEPS + 1):
    _, _, _, info = full.step(actions)
    shadow_only.step(actions)
    rows = full.link_positions()[0, pair]
    distance = float(torch.hypot(rows[2] - rows[0], rows[3] - rows[1]))
    median = 10 * PLE * math.log10(distance) + const
    with_fading = float(full.path_loss_db()[0, pair, pair])
    without = float(shadow_only.path_loss_db()[0, pair, pair])
    sinr = float(info['sinr_db'][0, pair])
    print(f'  {step:4d}  {distance:10.3f}  {median:9.2f}  {without - median:9.2f}  {with_fading - without:9.2f}  {sinr:9.2f}')
full.close(); shadow_only.close()

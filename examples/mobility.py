"""Device mobility: VecD2DEnv(mobility=GaussMarkovMobility(...)) moves every device before every step (one kernel launch,
csrc/d2d_mobility.hip).  Follows one DUE pair's distance and SINR over an episode while everybody keeps the RB and power of the first
step - the stale choice mobility makes costly - and counts how often a link's strongest interferer changes from one step to the next."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.mobility import GaussMarkovMobility

NUM_ENVS, RBS, CUES, DUES, STEPS = 64, 8, 16, 48, 10
model = GaussMarkovMobility(speed_std_mps=8.0, memory=0.8, dt_s=1.0)  # vehicles: sigma 8 m/s per axis, one second per step
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                mobility=model)
env.reset(seed=7)
actions = env.action_buffer().clone()                                # the reset's random (rb, power): kept for the whole episode
pair = CUES                                                          # link index of the first DUE pair
strongest = env.neighbors(1)[0][..., 0].clone()
changed = []
print(f'{NUM_ENVS} envs x {CUES + DUES} links, {model}; env 0, DUE pair 0:')
print('  step  distance m   speed m/s   sinr dB')
for step in range(1, STEPS + 1):
    _, _, _, info = env.step(actions)
    rows = env.link_positions()[0, pair]                             # (tx_x, tx_y, rx_x, rx_y), current after the move
    distance = float(torch.hypot(rows[2] - rows[0], rows[3] - rows[1]))
    vx, vy = env.velocities()
    tx_dev = int(env.simulator.link_tx[pair])
    speed = float(torch.hypot(vx[0, tx_dev], vy[0, tx_dev]))
    now = env.neighbors(1)[0][..., 0]
    changed.append(float((now != strongest).float().mean()))
    strongest = now.clone()
    print(f'  {step:4d}  {distance:10.3f}  {speed:10.3f}  {float(info["sinr_db"][0, pair]):8.2f}')
env.close()
print(f'a link\'s strongest interferer changed between consecutive steps for {sum(changed) / len(changed):.1%} of the links on average')

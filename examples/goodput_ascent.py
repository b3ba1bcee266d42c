"""The queue-aware baseline of the D2D underlay on the GPU: with a packet queue behind every link, a link moves its RB or its power
to where the env delivers most of its BACKLOG, not most Shannon capacity - a link with an empty buffer is worth nothing, and a link
that can deliver all it holds at a fifth of its power goes down to that power and stops interfering.  VecD2DEnv.goodput_ascent()
runs the whole local search - every link turn of every round of every env, RBs and powers alike - in one launch of
csrc/d2d_goodput.hip, and goodput_ascent_actions() hands step() the result.

6 CUEs + 10 pairs on 6 RBs, the pairs the agents, PacketTraffic with uneven loads (bursty pairs offered five times what a CUE is).
Four policies over one episode on the same layouts and the same arrivals:

    random            uniformly random actions every step
    capacity_ascent   rb_ascent() and power_ascent() in turn, one of them per step: what maximises the total capacity
    goodput_ascent    goodput_ascent_actions() every step: weight 1, demand the live backlog
    max_weight        the classic max-weight rule: weight = backlog_bits >> 4, demand uncapped

Ends in `results`: per policy the delivered Mbps and the expired bits of every env."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
from gym_d2d_amd.queues import PacketTraffic

NUM_ENVS, CUES, PAIRS, RBS, STEPS, CUE_FLOOR_DB = 64, 6, 10, 6, 40, 0.0
# 1 ms steps; an ON CUE is offered 0.4 and an ON pair 2 packets of 1000 bits per step on average, in bursts of mean length 5 steps
model = PacketTraffic(packets_per_step=(0.4, 2.0), packet_bits=1000, deadline_steps=4, buffer_bits=8 * 1000, dt_s=1e-3, p_on_to_off=0.2,
                      p_off_to_on=0.2)
floor = {'cue': CUE_FLOOR_DB, 'due': float('-inf')}
results = {}


def run(policy: str):
    env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                    cue_actions='traffic', traffic=model)            # the pairs are the agents; the CUEs keep their traffic model's RBs
    levels = env.num_pwr_actions['due']                              # action = rb * levels + power level
    gen = torch.Generator(device=env.device).manual_seed(7)
    env.reset(seed=7)
    served = torch.zeros(NUM_ENVS, dtype=torch.float64, device=env.device)
    expired = torch.zeros(NUM_ENVS, dtype=torch.float64, device=env.device)
    for k in range(STEPS):
        if policy == 'random':
            actions = torch.randint(0, RBS * levels, (NUM_ENVS, PAIRS), generator=gen, device=env.device, dtype=torch.int32)
        elif policy == 'capacity_ascent':
            actions = env.rb_ascent_actions(floor_sinr_db=floor) if k % 2 == 0 else env.power_ascent_actions(floor_sinr_db=floor)
        elif policy == 'goodput_ascent':
            actions = env.goodput_ascent_actions(floor_sinr_db=floor)
        else:
            weight = (env.queues().backlog_bits >> 4).clamp(0, 1 << 20)
            actions = env.goodput_ascent_actions(demand_bits=(1 << 31) - 1, weight=weight, floor_sinr_db=floor)
        env.step(actions)
        q = env.queues()
        served += q.served_bits.sum(dim=1, dtype=torch.float64)
        expired += q.expired_bits.sum(dim=1, dtype=torch.float64)
    env.close()
    results[policy] = {'delivered_mbps': (served / (STEPS * model.bits_per_mbps_step)).cpu().numpy(), 'expired_bits': expired.cpu().numpy()}
    print(f'  {policy:<16} delivered {float(served.mean()) / (STEPS * model.bits_per_mbps_step):8.3f} Mbps per env   '
          f'expired {float(expired.mean()):9.0f} bits per env')


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {PAIRS} pairs) on {RBS} RBs, {STEPS} steps, CUE floor {CUE_FLOOR_DB:g} dB')
for name in ('random', 'capacity_ascent', 'goodput_ascent', 'max_weight'):
    run(name)

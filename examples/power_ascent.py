"""The sum-capacity power baseline of the D2D underlay on the GPU: with the RBs where they are, which powers maximise the total
capacity, with the cellular links kept above a SINR floor?  VecD2DEnv.power_ascent() runs the whole coordinate ascent - every link
turn of every round of every env - in one launch of csrc/d2d_ascent.hip; as a host loop it is one evaluate() launch and one round
trip per link turn.

Three allocations on the same layouts, compared by evaluate(): the uniformly random actions of the first step; the RBs of
color_rbs_actions() (a conflict-graph colouring) and then the ascent on the powers; and the ascent alone on the random RBs, started
once from the held powers and once from every link's maximum, the better of the two kept per env (coordinate ascent ends in a local
optimum that depends on where it began).  A CUE that meets its floor at the start is never pushed under it.

Ends in `results`: per allocation the total capacity of every env (Mbps)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv

NUM_ENVS, RBS, CUES, DUES, CUE_FLOOR_DB, COLOR_MARGIN_DB = 64, 6, 6, 10, 0.0, 10.0
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES}, num_envs=NUM_ENVS)
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
highs = torch.as_tensor(env._initial_action_highs(), device=env.device)
random_actions = (torch.rand((NUM_ENVS, env.num_agents), generator=gen, device=env.device) * highs).to(torch.int32)
floor = {'cue': CUE_FLOOR_DB, 'due': float('-inf')}


def total(actions):
    """The total capacity [B] evaluate() gives an action tensor [B, num_agents], at the current positions."""
    return env.evaluate_actions(actions[:, None, :].contiguous(), planes=())['total_mbps'][:, 0].clone()


env.step(random_actions)
random_mbps = total(random_actions)

# the ascent alone, from the held powers and from the top: the better per env
held = env.power_ascent_actions(floor_sinr_db=floor, start='held').clone()
solved = env.power_ascent(floor_sinr_db=floor, start='held')
rounds, moves, converged = solved.rounds.clone(), solved.moves.clone(), solved.converged.clone()
top = env.power_ascent_actions(floor_sinr_db=floor, start='max').clone()
held_mbps, top_mbps = total(held), total(top)
ascent_mbps = torch.maximum(held_mbps, top_mbps)

# RBs by colouring, then powers by ascent: one call picks RBs, the other picks powers
env.step(env.color_rbs_actions(COLOR_MARGIN_DB))
colored = env.power_ascent_actions(floor_sinr_db=floor, start='held').clone()
colored_ascent_mbps = total(colored)

print(f'{NUM_ENVS} envs x ({CUES} CUEs + {DUES} pairs) on {RBS} RBs, CUE floor {CUE_FLOOR_DB:g} dB; total capacity per env, mean over envs')
for what, mbps in (('random actions', random_mbps), ("power_ascent('held')", held_mbps), ("power_ascent('max')", top_mbps),
                   ('the better of the two', ascent_mbps), ('color_rbs, then power_ascent', colored_ascent_mbps)):
    print(f'  {what:<30} {float(mbps.mean()):8.2f} Mbps')
print(f"  from the held powers: {float(rounds.float().mean()):.1f} rounds and {float(moves.float().mean()):.1f} moves per env in the one "
      f'launch, {int(converged.sum())} of {NUM_ENVS} envs converged')
results = {'random_mbps': random_mbps.cpu().numpy(), 'held_mbps': held_mbps.cpu().numpy(), 'max_mbps': top_mbps.cpu().numpy(),
           'ascent_mbps': ascent_mbps.cpu().numpy(), 'colored_ascent_mbps': colored_ascent_mbps.cpu().numpy(),
           'rounds': rounds.cpu().numpy(), 'moves': moves.cpu().numpy(), 'converged': converged.cpu().numpy()}
env.close()

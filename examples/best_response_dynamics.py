"""RB choice by sequential best response, then power control, on the GPU: the DUE pairs take turns moving to the RB on which they
would see the highest SINR, each seeing the moves made before its turn, until a whole round moves nobody
(VecD2DEnv.best_response_dynamics_actions(): every turn of every round in one launch of csrc/d2d_brdyn.hip); then all pairs take
the least power that meets a target SINR given everybody else (VecD2DEnv.power_control_actions(): csrc/d2d_powerctl.hip).  Two
steps in all.  The CUEs keep what their traffic model gave them.

Beside it, on the same layouts: uniformly random actions, and the loop examples/power_control.py runs - eight rounds in which a
quarter of the pairs answer the same old state at once (best_response_actions()) and all pairs are then power-controlled.  Moving in
turns needs neither the quarter nor the eight rounds: nobody moves onto an RB that somebody else has just moved onto.

As in examples/power_control.py, a pair whose target is out of reach at its maximum power stands down to its lowest level."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, ROUNDS, MOVERS, TARGET_DB, MIN_GAIN_DB = 256, 16, 16, 48, 8, 4, 12.0, 3.0
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
random_actions = torch.randint(0, RBS * levels, (NUM_ENVS, DUES), generator=gen, device=env.device, dtype=torch.int32)
_, _, _, info = env.step(random_actions)


def report(what, info):
    mw = (10.0 ** (info['tx_pwr_dbm'][:, CUES:].float() / 10.0)).sum(dim=1).mean()
    met = (info['sinr_db'][:, CUES:] >= TARGET_DB).float().mean()
    print(f'  {what:<44} {float(mw):9.1f} mW per env   {float(met):6.1%} of the pairs at {TARGET_DB:g} dB or more')
    return float(mw), float(met)


def power_step():
    """All pairs to the least power that meets the target; the pairs that cannot meet it at full power stand down."""
    solved = env.power_control(TARGET_DB)
    out_of_reach = solved.sinr_db[:, CUES:] < TARGET_DB               # at full power and still short of the target
    actions = env.power_control_actions(TARGET_DB)
    return env.step(torch.where(out_of_reach, actions - actions % levels, actions))[3]


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {DUES} pairs) on {RBS} RBs, target {TARGET_DB:g} dB for the pairs')
random_mw, random_met = report('random actions', info)

# the alternating loop of examples/power_control.py: 2 steps and 3 launches per round
link = torch.arange(CUES + DUES, device=env.device)
every_rb = torch.ones((CUES + DUES, RBS), dtype=torch.bool, device=env.device)
for k in range(ROUNDS):
    allowed = every_rb & (link % MOVERS == k % MOVERS)[:, None]       # a quarter of the pairs may move per round
    env.step(env.best_response_actions(allowed=allowed, min_gain_db=MIN_GAIN_DB))
    info = power_step()
loop_mw, loop_met = report(f'{ROUNDS} rounds of a quarter at once + power control', info)

# sequential best response from the same random start: one launch and one step for the RBs, one of each for the powers
env.step(random_actions)
solved = env.best_response_dynamics(min_gain_db=MIN_GAIN_DB)
rounds, moves, converged = float(solved.rounds.float().mean()), float(solved.moves.float().mean()), float(solved.converged.float().mean())
_, _, _, info = env.step(env.best_response_dynamics_actions(min_gain_db=MIN_GAIN_DB))
report(f'pairs in turns ({rounds:.1f} rounds, {moves:.0f} moves per env)', info)
info = power_step()
final_mw, final_met = report('... then power control', info)
print(f'  {converged:.0%} of the envs reached a round that moved nobody')
env.close()

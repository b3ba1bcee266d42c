"""The regret of a joint action on the GPU: how much the total capacity would gain if ONE link alone changed its (RB, power).
VecD2DEnv.deviation_gains() gives the whole counterfactual row of every agent - one entry per action of its alphabet, -inf where a
protected link would be pushed under its SINR floor - in one launch of csrc/d2d_deviate.hip; best_deviation() reduces it to every
link's best move and the env's regret without writing the table, and best_deviation_actions() is one steepest-ascent step: the link
that gains most moves, RB and power in ONE move, everybody else repeats.  A joint action is a Nash point of the team game iff its
regret is 0.

6 CUEs + 10 pairs on 6 RBs, the pairs the agents.  The regret and the total capacity of three joint actions on the same layouts: the
uniformly random actions of the first step; rb_ascent() alternated with power_ascent() until neither moves (at most 8 alternations),
which moves one half of the action at a time; and steepest ascent by step(best_deviation_actions()) until the regret is 0
everywhere.  share_rbs(), the exact optimum over the pairs' RBs at the powers held, scores the RB half of each end point.

Ends in `results`: per joint action the total capacity and the regret of every env (Mbps)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, CUES, PAIRS, RBS, CUE_FLOOR_DB, ALTERNATIONS, MAX_STEPS = 64, 6, 10, 6, 0.0, 8, 400

env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')                               # the pairs are the agents; the CUEs keep their traffic model's RBs
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
random_actions = torch.randint(0, RBS * levels, (NUM_ENVS, PAIRS), generator=gen, device=env.device, dtype=torch.int32)
floor = {'cue': CUE_FLOOR_DB, 'due': float('-inf')}
results = {}


def total(rb_plane, pwr_plane):
    return env.evaluate(rb_plane[:, None, :].contiguous(), pwr_plane[:, None, :].contiguous(), planes=())['total_mbps'][:, 0].double()


def report(what, info, note=''):
    """The total capacity and the regret of the joint action the last step applied, per env; and what share_rbs() makes of its RBs."""
    rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()
    res = env.best_deviation(floor_sinr_db=floor)
    regret, movers = res.regret_mbps.clone(), (res.gain_mbps > 0).sum(dim=1).float()
    mbps, best_rbs = total(rb, pwr), total(env.share_rbs().rb.clone(), pwr)
    results[what + '_mbps'], results[what + '_regret_mbps'] = mbps.cpu().numpy(), regret.cpu().numpy()
    print(f'  {what:<18} {float(mbps.mean()):9.3f} Mbps per env   regret {float(regret.mean()):7.3f} Mbps, {float(movers.mean()):4.1f} of {PAIRS} '
          f'pairs would move, {float((regret == 0).float().mean()):4.0%} of the envs at a Nash point   share_rbs() at these powers '
          f'{float(best_rbs.mean()):9.3f}{note}')


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {PAIRS} pairs) on {RBS} RBs, CUE floor {CUE_FLOOR_DB:g} dB; total capacity scored by evaluate()')
_, _, _, info = env.step(random_actions)
report('random', info)

# the table itself: one row per pair, indexed by the action (the pairs share one class, so [B, M, R * L] is [B, M, action])
gains, links, _ = env.deviation_gains(floor_sinr_db=floor)
by_action = gains.view(NUM_ENVS, PAIRS, RBS * levels)
held = random_actions.long()[:, :, None]
assert bool((by_action.gather(2, held) == 0).all())                   # +0.0 on the action each pair holds
print(f'  the table: {list(gains.shape)} float32, {float(torch.isinf(by_action).float().mean()):.1%} of the actions closed by the CUE floor, '
      f'{float((by_action > 0).float().mean()):.1%} would raise the total')

# RBs and powers in turn: one call picks RBs, the other picks powers, and step() applies each
alternations = 0
for _ in range(ALTERNATIONS):
    alternations += 1
    moved = int(env.rb_ascent(floor_sinr_db=floor).moves.sum())
    env.step(env.rb_ascent_actions(floor_sinr_db=floor))
    moved += int(env.power_ascent(floor_sinr_db=floor).moves.sum())
    _, _, _, info = env.step(env.power_ascent_actions(floor_sinr_db=floor))
    if moved == 0:
        break
report('alternating', info, f'   ({alternations} alternations of rb_ascent, power_ascent)')

# steepest ascent in the product neighbourhood, from the random actions again: only the leader moves, RB and power at once
_, _, _, info = env.step(random_actions)
steps = 0
while steps < MAX_STEPS and bool((env.best_deviation(floor_sinr_db=floor).regret_mbps > 0).any()):
    _, _, _, info = env.step(env.best_deviation_actions(floor_sinr_db=floor))
    steps += 1
report('steepest_ascent', info, f'   ({steps} steps, one move per env and step)')
results['alternations'], results['steepest_steps'] = alternations, steps
env.close()

"""The cooperative RB baseline of the D2D underlay on the GPU: with the powers where they are, a link moves to the RB where the TOTAL
capacity gains most, and a cellular link that meets its SINR floor is never pushed under it.  VecD2DEnv.rb_ascent() runs the whole
local search - every link turn of every round of every env - in one launch of csrc/d2d_rbascent.hip; as a host loop it is one
evaluate() launch and one round trip per link turn.  Alternated with power_ascent() it moves RBs and powers in turn, on the device.

6 CUEs + 10 pairs on 6 RBs, the pairs the agents.  Five allocations on the same layouts, every plane scored by evaluate(): the
uniformly random actions of the first step; best_response_dynamics(), which maximises each link's own SINR; rb_ascent();
rb_ascent() alternated with power_ascent() until neither moves (at most 8 alternations); and share_rbs(), the exact optimum over
the RBs of the ten pairs at the powers held - a certificate for the RB half, taken at the random powers and again at the powers
the alternation ended at.

Ends in `results`: per allocation the total capacity of every env (Mbps)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, CUES, PAIRS, RBS, CUE_FLOOR_DB, ALTERNATIONS = 64, 6, 10, 6, 0.0, 8

env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')                               # the pairs are the agents; the CUEs keep their traffic model's RBs
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
_, _, _, info = env.step(torch.randint(0, RBS * levels, (NUM_ENVS, PAIRS), generator=gen, device=env.device, dtype=torch.int32))
rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()
floor = {'cue': CUE_FLOOR_DB, 'due': float('-inf')}
results = {}


def report(what, rb_plane, pwr_plane, note=''):
    """evaluate()'s total capacity of an (rb, power) plane pair [B, N], per env."""
    mbps = env.evaluate(rb_plane[:, None, :].contiguous(), pwr_plane[:, None, :].contiguous(), planes=())['total_mbps'][:, 0]
    results[what] = mbps.double().cpu().numpy()
    print(f'  {what[:-5]:<30} {float(mbps.double().mean()):9.3f} Mbps per env{note}')


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {PAIRS} pairs) on {RBS} RBs, CUE floor {CUE_FLOOR_DB:g} dB; total capacity, scored by evaluate()')
report('random_mbps', rb, pwr)
res = env.best_response_dynamics()
report('best_response_dynamics_mbps', res.rb.clone(), pwr, f'   ({float((res.converged != 0).float().mean()):.0%} converged)')
res = env.rb_ascent(floor_sinr_db=floor)
report('rb_ascent_mbps', res.rb.clone(), pwr, f'   ({float(res.moves.float().mean()):.1f} moves in {float(res.rounds.float().mean()):.1f} rounds per env, '
       f'{float((res.converged != 0).float().mean()):.0%} converged)')
report('share_rbs_mbps', env.share_rbs().rb.clone(), pwr, '   (the optimum over the pairs\' RBs at these powers)')

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
rb_alt, pwr_alt = info['rb'].clone(), info['tx_pwr_dbm'].clone()
report('alternating_mbps', rb_alt, pwr_alt, f'   (rb_ascent, power_ascent, ...: {alternations} alternations)')
report('share_rbs_alternating_mbps', env.share_rbs().rb.clone(), pwr_alt, '   (the optimum over the pairs\' RBs at the powers above)')
results['alternations'] = alternations
env.close()

"""Max-min fairness for the D2D underlay on the GPU: the largest SINR every DUE pair can be given at once with every cellular link
kept above a floor, and the least powers that give it (VecD2DEnv.balance_sinr(): the whole bisection, every probe a full
power-control solve, in one launch of csrc/d2d_balance.hip).  The CUEs keep what their traffic model gave them and are protected
by the floor; only the pairs move.

Three allocations on the same layouts and RBs: the uniformly random powers of the first step, one fixed power_control() target -
the level a designer would pick without knowing the layout, here the lowest level of the grid - and the balanced level of every env.
Because the fixed target is a level of the grid, the balanced run can only do better where that level is feasible at all: either
the search stops there (the same solve, the same powers) or it ends on a higher level, which every pair then meets.  Envs in which
even the lowest level breaks a CUE's floor are reported as infeasible (level -1) and left out of the comparison.

Ends in `results`: per allocation the minimum DUE SINR of every env, and the share of envs that keep every CUE floor."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, CUE_FLOOR_DB, FIXED_DB, TOP_DB = 256, 8, 8, 24, -5.0, 0.0, 40.0
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=11)
gen = torch.Generator(device=env.device).manual_seed(11)
random_actions = torch.randint(0, RBS * levels, (NUM_ENVS, DUES), generator=gen, device=env.device, dtype=torch.int32)
floor = {'cue': CUE_FLOOR_DB, 'due': float('-inf')}
margins = torch.arange(FIXED_DB, TOP_DB + 1.0, device=env.device)     # FIXED_DB, FIXED_DB + 1, ..., TOP_DB over a base of 0 dB


def measure(info):
    """(minimum DUE SINR per env, every CUE at its floor or above per env) of a step."""
    sinr = info['sinr_db']
    return sinr[:, CUES:].min(dim=1).values.clone(), (sinr[:, :CUES] >= CUE_FLOOR_DB).all(dim=1)


_, _, _, info = env.step(random_actions)
random_min, random_kept = measure(info)

# one fixed target for every pair: the least powers that meet it, whatever that does to the CUEs
_, _, _, info = env.step(env.power_control_actions({'cue': 0.0, 'due': FIXED_DB}))
fixed_min, fixed_kept = measure(info)

# the balanced level: back on the random powers first (the CUEs' held powers and the RBs are the same for both solves)
env.step(random_actions)
solved = env.balance_sinr(0.0, margins, floor)
level, margin_db, probes = solved.level.clone(), solved.margin_db.clone(), solved.probes.clone()
_, _, _, info = env.step(env.balance_sinr_actions(0.0, margins, floor))
balanced_min, balanced_kept = measure(info)
feasible = level >= 0

print(f'{NUM_ENVS} envs x ({CUES} CUEs + {DUES} pairs) on {RBS} RBs, CUE floor {CUE_FLOOR_DB:g} dB; minimum DUE SINR per env, mean over envs')
for what, worst, kept in (('random powers', random_min, random_kept), (f'power_control({FIXED_DB:g} dB)', fixed_min, fixed_kept),
                          ('balance_sinr()', balanced_min, balanced_kept)):
    print(f'  {what:<24} {float(worst[feasible].mean()):7.2f} dB on the {int(feasible.sum())} feasible envs   '
          f'every CUE floor kept in {float(kept.float().mean()):6.1%} of all envs')
print(f'  balanced level {float(margin_db[feasible].mean()):.1f} dB on average ({float(margin_db[feasible].min()):g} .. '
      f'{float(margin_db[feasible].max()):g}), {float(probes.float().mean()):.1f} solves per env in the one launch; '
      f'{int((~feasible).sum())} envs cannot keep the floors even at {FIXED_DB:g} dB')
results = {'feasible': feasible.cpu().numpy(), 'level': level.cpu().numpy(), 'margin_db': margin_db.cpu().numpy(),
           'probes': probes.cpu().numpy(), 'random_min_db': random_min.cpu().numpy(), 'fixed_min_db': fixed_min.cpu().numpy(),
           'balanced_min_db': balanced_min.cpu().numpy(), 'random_floors_kept': random_kept.cpu().numpy(),
           'fixed_floors_kept': fixed_kept.cpu().numpy(), 'balanced_floors_kept': balanced_kept.cpu().numpy()}
env.close()

"""The cooperative baseline of the D2D-underlay literature: admission control, the best power for every admissible (pair, RB), and
maximum-weight matching - VecD2DEnv.assign_rbs_power(), one launch of csrc/d2d_assignpwr.hip and the matching launch of
csrc/d2d_assign.hip.

Every DUE pair gets an RB of its own AND a power, so that the total capacity of the env is maximal while every link that could keep
its minimum SINR still keeps it.  A background link sees at most one pair under a one-to-one placement, so its loss and its floor
depend on that pair's RB and power alone: the Hungarian optimum of the best-power weights is the joint optimum, not a heuristic.

Beside it, on the same layouts and scored by evaluate(): the random actions the layouts start from, and assign_rbs(), which places
the pairs at the powers they happen to have and protects nobody."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES = 256, 32, 16, 24
FLOORS = {'cue': 5.0, 'due': 0.0}
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS)
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
highs = torch.as_tensor(env._initial_action_highs(), device=env.device)
random_actions = (torch.rand((NUM_ENVS, CUES + DUES), generator=gen, device=env.device) * highs).to(torch.int32)
_, _, _, info = env.step(random_actions)
rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()
floor = torch.cat([torch.full((CUES,), FLOORS['cue']), torch.full((DUES,), FLOORS['due'])]).to(env.device)


def score(rb_plane, pwr_plane):
    """(total Mbps [B], sinr_db [B, N]) of one assignment per env, by evaluate()."""
    out = env.evaluate(rb_plane[:, None, :].contiguous(), pwr_plane[:, None, :].contiguous(), planes=('sinr_db',))
    return out['total_mbps'][:, 0].clone(), out['sinr_db'][:, 0].clone()


off = rb.clone()
off[:, CUES:] = -1
_, background_sinr = score(off, pwr)
bound = background_sinr >= floor                                     # the links the background alone holds over their floor
bound[:, CUES:] = True                                               # ... and every pair that is placed

results = {}


def report(what, rb_plane, pwr_plane):
    total, sinr = score(rb_plane, pwr_plane)
    under = int((bound & (sinr < floor - 1e-4)).sum())
    results[what] = float(total.double().mean())
    print(f'  {what:<52} {float(total.mean()):9.2f} Mbps per env, {under:5d} constrained links under their floor')
    return under


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {DUES} pairs) on {RBS} RBs; total capacity and the floors {FLOORS} dB, scored by evaluate()')
report('random actions', rb, pwr)
res = env.assign_rbs()
report('assign_rbs() at the current powers', res.rb.clone(), pwr)
res = env.assign_rbs_power()
report('assign_rbs_power()', res.rb.clone(), res.power_dbm.clone())
res = env.assign_rbs_power(min_sinr_db=FLOORS)
feasible = res.feasible.bool()
matched_rb, matched_pwr = res.rb.clone(), res.power_dbm.clone()
print(f'  with floors: {float(feasible.float().mean()):.0%} of the envs feasible (the others keep their rows)')
total, sinr = score(matched_rb, matched_pwr)
results['links under their floor with floors (5, 0) dB'] = int((bound & (sinr < floor - 1e-4))[feasible].sum())
results['assign_rbs_power(min_sinr_db=...)'] = float(total[feasible].double().mean()) if bool(feasible.any()) else 0.0
print(f"  {'assign_rbs_power(min_sinr_db=...) where feasible':<52} {results['assign_rbs_power(min_sinr_db=...)']:9.2f} Mbps per env, "
      f"{results['links under their floor with floors (5, 0) dB']:5d} constrained links under their floor")

# the step that takes the actions exports those planes
res = env.assign_rbs_power()
matched_rb, matched_pwr = res.rb.clone(), res.power_dbm.clone()
_, _, _, info = env.step(env.assign_rbs_power_actions())
assert torch.equal(info['rb'], matched_rb) and torch.equal(info['tx_pwr_dbm'], matched_pwr)
results['the step that takes assign_rbs_power_actions()'] = float(info['capacity_mbps'].double().sum(dim=1).mean())
print(f"  {'the step that takes assign_rbs_power_actions()':<52} {results['the step that takes assign_rbs_power_actions()']:9.2f} Mbps per env")
env.close()

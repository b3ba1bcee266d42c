"""The cooperative optimum a learner can be scored against: every DUE pair matched to an RB of its own so that the TOTAL capacity of
the env is maximal (VecD2DEnv.assign_rbs(): the weights of every pair on every RB and their maximum-weight matching, two launches
of csrc/d2d_assign.hip).  The CUEs keep what their traffic model gave them; the pairs keep their powers.

Pairs on distinct RBs do not interfere with each other, so the total capacity of such a placement is the background's plus the
sum of the matched weights (own capacity minus the harm done to the CUE on that RB) - exactly, which makes the Hungarian optimum the
optimum of the total capacity over all one-to-one placements, not a heuristic.

Beside it, on the same layouts and scored by evaluate(): uniformly random RBs, the best of 32 random one-to-one placements, and
best_response_dynamics(), the selfish SINR response - which may put several pairs on one RB, so it is not bound by the optimum of
the one-to-one placements, and which ignores the harm it does."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, RANDOM = 256, 32, 16, 24, 32
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
random_actions = torch.randint(0, RBS * levels, (NUM_ENVS, DUES), generator=gen, device=env.device, dtype=torch.int32)
_, _, _, info = env.step(random_actions)
rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()


def total(rb_planes):
    """evaluate()'s total capacity of candidate RB planes [B, K, N] at the current powers: [B, K] Mbps."""
    k = rb_planes.shape[1]
    return env.evaluate(rb_planes.contiguous(), pwr[:, None, :].expand(-1, k, -1).contiguous(), planes=())['total_mbps'].clone()


results = {}


def report(what, mbps):
    results[what] = float(mbps.double().mean())
    print(f'  {what:<52} {float(mbps.mean()):9.2f} Mbps per env')


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {DUES} pairs) on {RBS} RBs; total capacity, scored by evaluate()')
report('random actions', total(rb[:, None, :])[:, 0])

# 32 random one-to-one placements of the pairs per env
perms = torch.rand((NUM_ENVS, RANDOM, RBS), generator=gen, device=env.device).argsort(dim=2)[:, :, :DUES].to(torch.int32)
cand = rb[:, None, :].repeat(1, RANDOM, 1)
cand[:, :, CUES:] = perms
report(f'the best of {RANDOM} random one-to-one placements', total(cand).max(dim=1).values)

# selfish SINR response, in turns
dyn = env.best_response_dynamics()
report(f'best_response_dynamics() ({float(dyn.converged.float().mean()):.0%} converged)', total(dyn.rb[:, None, :].clone())[:, 0])

# the matching: total capacity, then the pairs' own capacities alone
for objective in ('total', 'own'):
    res = env.assign_rbs(objective=objective)
    assert bool(res.feasible.all())
    report(f"assign_rbs(objective='{objective}')", total(res.rb[:, None, :].clone())[:, 0])

# the certificate: total(rb) = total(background) + value_mbps, and the step that takes the actions exports that rb
res = env.assign_rbs()
matched, value = res.rb.clone(), res.value_mbps.clone()
off = rb.clone()
off[:, CUES:] = -1
background = env.evaluate(off[:, None, :].contiguous(), pwr[:, None, :].contiguous(), planes=('capacity_mbps',))['capacity_mbps'][:, 0, :CUES]
gap = (background.double().sum(dim=1) + value.double()) / total(matched[:, None, :])[:, 0].double() - 1.0
print(f'  background + value_mbps against evaluate(): largest relative gap {float(gap.abs().max()):.1e}')
_, _, _, info = env.step(env.assign_rbs_actions())
assert torch.equal(info['rb'], matched)
report('the step that takes assign_rbs_actions()', info['capacity_mbps'].double().sum(dim=1))
env.close()

"""How far are the many-to-one RB allocators from the optimum?  VecD2DEnv.share_rbs() answers exactly for up to twelve movable links:
sharing_values() holds the capacity of every RB under every subset of the pairs, mutual interference included, and solve_sharing()
takes the best of all R^M placements by a max-plus subset convolution over the RBs - two launches of csrc/d2d_share.hip.

6 CUEs + 10 pairs on 6 RBs: more pairs than RBs, so assign_rbs() (one pair per RB) is a ValueError, and 6^10 = 60 million
placements are out of reach of evaluate() over an enumerated candidate tensor.  The optimum stands beside color_rbs() (both pack
settings), stable_rbs(quota=2), best_response_dynamics() and random actions, every plane scored by evaluate()."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, CUES, PAIRS, RBS, MARGIN = 64, 6, 10, 6, 15.0

env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')                               # the pairs are the agents; the CUEs keep their traffic model's RBs
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
_, _, _, info = env.step(torch.randint(0, RBS * levels, (NUM_ENVS, PAIRS), generator=gen, device=env.device, dtype=torch.int32))
rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()
results = {}


def report(what, rb_plane, note=''):
    """evaluate()'s total capacity of an RB plane [B, N] at the current powers, per env."""
    mbps = env.evaluate(rb_plane[:, None, :].contiguous(), pwr[:, None, :].contiguous(), planes=())['total_mbps'][:, 0]
    results[what] = mbps.double()
    print(f'  {what:<34} {float(mbps.double().mean()):9.3f} Mbps per env{note}')


print(f'{NUM_ENVS} envs x ({CUES} CUEs + {PAIRS} pairs) on {RBS} RBs; total capacity, scored by evaluate()')
report('random actions', rb)
try:
    env.assign_rbs()
except ValueError as why:                                            # more pairs than RBs: one pair per RB cannot be had
    print(f'  {"assign_rbs()":<34} ValueError: {why}')
for pack in (False, True):
    res = env.color_rbs(MARGIN, pack=pack)
    report(f'color_rbs({MARGIN:g} dB, pack={pack})', res.rb.clone(), f'   ({float((res.proper != 0).float().mean()):.0%} proper)')
res = env.stable_rbs(quota=2)
report('stable_rbs(quota=2)', res.rb.clone(), f'   ({float(res.unmatched.float().mean()):.1f} pairs unmatched)')
res = env.best_response_dynamics()
report('best_response_dynamics()', res.rb.clone(), f'   ({float((res.converged != 0).float().mean()):.0%} converged)')
best = env.share_rbs()
optimum = best.value_mbps.clone()
report('share_rbs(): the optimum', best.rb.clone(), f'   (value_mbps {float(optimum.double().mean()):.3f})')
report('share_rbs(quota=2)', env.share_rbs(quota=2).rb.clone(), '   (the optimum with at most two pairs per RB)')
top = results['share_rbs(): the optimum']
for what, mbps in results.items():
    assert bool((mbps <= top * (1 + 1e-6)).all()), what              # nothing beats the optimum
    print(f'  {what:<34} reaches {float((mbps / top).mean()):7.2%} of the optimum')
# the step that takes the actions exports that rb
want = env.share_rbs().rb.clone()
_, _, _, info = env.step(env.share_rbs_actions())
assert torch.equal(info['rb'], want)
env.close()

"""Difference rewards: what the system capacity loses when one link alone is taken out, D_i = G(a) - G(a without link i), from
VecD2DEnv.marginal_capacity() - one kernel launch for all envs and links.  Prints a few links' capacity, harm and difference, the
share of links whose difference reward is negative (links a shared or a selfish reward keeps rewarding), and checks one link of
every env against an actual second step in which that link is parked on an RB nobody uses."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES = 64, 24, 16, 48
SPARE = RBS - 1                                                      # the RB this example keeps free
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS)
levels = torch.tensor([env.num_pwr_actions['cue']] * CUES + [env.num_pwr_actions['due']] * DUES, device=env.device)[None, :]
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
rb = torch.randint(0, SPARE, (NUM_ENVS, CUES + DUES), generator=gen, device=env.device)
power = (torch.rand((NUM_ENVS, CUES + DUES), generator=gen, device=env.device) * levels).long()
actions = (rb * levels + power).to(torch.int32)                      # action = rb * levels + power level
_, _, _, info = env.step(actions)
capacity = info['capacity_mbps'].clone()
difference, harm = (t.clone() for t in env.marginal_capacity())
negative_share = float((difference < 0).float().mean())

print(f'{NUM_ENVS} envs x {CUES + DUES} links on {RBS - 1} of {RBS} RBs; env 0:')
print('  link   capacity       harm difference   (Mbps)')
for i in (0, 1, CUES, CUES + 1, CUES + DUES - 1):
    print(f'  {i:4d} {float(capacity[0, i]):10.4f} {float(harm[0, i]):10.4f} {float(difference[0, i]):10.4f}')
print(f'difference reward negative for {negative_share:.1%} of the links')

# the definition, executed: park link `pick[b]` of env b on the spare RB and step again; what the others gain is its harm
pick = torch.randint(0, CUES + DUES, (NUM_ENVS, 1), generator=gen, device=env.device)
parked = actions.long().scatter(1, pick, SPARE * levels.expand_as(actions).gather(1, pick) + power.gather(1, pick)).to(torch.int32)
_, _, _, info = env.step(parked)
others = torch.ones_like(capacity, dtype=torch.bool).scatter(1, pick, False)
gain = ((info['capacity_mbps'].double() - capacity.double()) * others).sum(dim=1)
self_check_error = float((gain - harm.gather(1, pick)[:, 0].double()).abs().max())
env.close()
print(f'self-check: harm of one link per env against a second step with that link parked: max |error| {self_check_error:.2e} Mbps '
      f'({"ok" if self_check_error <= 1e-4 else "MISMATCH"})')

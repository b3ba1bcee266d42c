"""Search over joint actions with the what-if scorer: per env, draw K complete joint actions of the DUE pairs, score them all in one
launch (VecD2DEnv.evaluate_actions(): csrc/d2d_evaluate.hip - K candidates share the env's layout, the env itself is not stepped),
take each env's best and step() it.  Then a few rounds of mutate-the-best: the K candidates of a round are the best so far (kept as
candidate 0, so a round never loses ground) and K - 1 copies of it in which a tenth of the pairs draw a fresh action.  Prints the system
capacity (sum of the links' capacities, mean over the envs) beside uniformly random actions and beside eight rounds of best response
on the same layouts.  The CUEs keep the RBs their traffic model gave them."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, RBS, CUES, DUES, K, ROUNDS, MUTATE = 256, 16, 16, 48, 64, 6, 0.1
env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': DUES, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                cue_actions='traffic')
levels = env.num_pwr_actions['due']                                  # action = rb * levels + power level
env.reset(seed=7)
gen = torch.Generator(device=env.device).manual_seed(7)
pick = torch.arange(NUM_ENVS, device=env.device)


def draw(*shape):
    return torch.randint(0, RBS * levels, shape, generator=gen, device=env.device, dtype=torch.int32)


def system_capacity(actions):
    """step() the actions [B, num_agents]: the mean over the envs of the summed capacities, and each env's own sum."""
    _, _, _, info = env.step(actions.contiguous())
    per_env = info['capacity_mbps'].sum(dim=1)
    return float(per_env.mean()), per_env.clone()


print(f'system capacity, mean of {NUM_ENVS} envs x {CUES + DUES} links on {RBS} RBs')
random_capacity, _ = system_capacity(draw(NUM_ENVS, DUES))
print(f'  random actions                       {random_capacity:9.1f} Mbps')

# ---- random shooting: K candidates per env, one launch, totals only
candidates = draw(NUM_ENVS, K, DUES)
total = env.evaluate_actions(candidates, planes=())['total_mbps']    # [B, K]; the env is untouched
best = candidates[pick, total.argmax(dim=1)]
predicted = total.max(dim=1).values.clone()
shooting_capacity, per_env = system_capacity(best)
# the scorer's total is the step's: the float32 sum of the plane step() exports differs from it by rounding only
self_check_error = float(((per_env - predicted).abs() / predicted).max())
print(f'  best of {K} random joint actions      {shooting_capacity:9.1f} Mbps   (self-check: predicted vs stepped {self_check_error:.1e})')

# ---- mutate the best
search_capacities = []
for k in range(ROUNDS):
    candidates = best[:, None, :].repeat(1, K, 1)
    mutate = torch.rand((NUM_ENVS, K, DUES), generator=gen, device=env.device) < MUTATE
    mutate[:, 0] = False                                             # candidate 0: the best so far, unchanged
    candidates = torch.where(mutate, draw(NUM_ENVS, K, DUES), candidates)
    total = env.evaluate_actions(candidates, planes=())['total_mbps']
    best = candidates[pick, total.argmax(dim=1)]
    search_capacities.append(float(total.max(dim=1).values.mean()))
    print(f'  mutate the best, round {k + 1}             {search_capacities[-1]:9.1f} Mbps   (predicted; no step taken)')
search_capacity, _ = system_capacity(best)
print(f'  ... stepped                          {search_capacity:9.1f} Mbps')

# ---- the best-response baseline on the same layouts, from the same random start
system_capacity(draw(NUM_ENVS, DUES))
link = torch.arange(CUES + DUES, device=env.device)
every_rb = torch.ones((CUES + DUES, RBS), dtype=torch.bool, device=env.device)
for k in range(8):
    allowed = every_rb & (link % 2 == k % 2)[:, None]               # half of the pairs may move per round
    best_response_capacity, _ = system_capacity(env.best_response_actions(allowed=allowed, min_gain_db=0.5))
print(f'  best response, 8 rounds              {best_response_capacity:9.1f} Mbps')
if self_check_error > 1e-5:
    print('MISMATCH between the predicted and the stepped capacity')
env.close()

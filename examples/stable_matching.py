"""The stable-matching baseline of the D2D-underlay literature (VecD2DEnv.stable_rbs(): the pairs and the RBs rank each other by the
planes of assignment_weights(), and Gale-Shapley deferred acceptance with the pairs proposing places them in one launch of
csrc/d2d_stable.hip), beside the other RB allocators, on the same layouts and scored by evaluate().

assign_rbs() maximises a sum nobody's incentives enforce; best_response_dynamics() follows incentives and can cycle; stable_rbs()
always ends, and no pair and RB would both rather be together than where the matching has them.  With quota 1 the pairs end on
distinct RBs, do not interfere with each other, and the preferences are the true capacities.  With a quota above 1 the matching
serves more pairs than RBs, as color_rbs() does - but the pairs that share an RB interfere, which the fixed preferences ignore:
stability then holds for the stated tensors only, and evaluate() below tells what the placement is worth."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, MARGIN = 64, 15.0
SHAPES = {'one-to-one: 16 + 16 links on 32 RBs': (16, 16, 32, 1), 'many-to-one: 6 + 24 links on 8 RBs, quota 3': (6, 24, 8, 3)}
results = {}

for label, (cues, dues, rbs, quota) in SHAPES.items():
    env = VecD2DEnv({'num_rbs': rbs, 'num_cues': cues, 'num_due_pairs': dues, 'obs_fn': SignalPlanesObsFunction}, num_envs=NUM_ENVS,
                    cue_actions='traffic')                           # the pairs are the agents; the CUEs keep their traffic model's RBs
    levels = env.num_pwr_actions['due']                              # action = rb * levels + power level
    env.reset(seed=7)
    gen = torch.Generator(device=env.device).manual_seed(7)
    _, _, _, info = env.step(torch.randint(0, rbs * levels, (NUM_ENVS, dues), generator=gen, device=env.device, dtype=torch.int32))
    rb, pwr = info['rb'].clone(), info['tx_pwr_dbm'].clone()
    out = results[label] = {}

    def report(what, rb_plane, note=''):
        """evaluate()'s total capacity of an RB plane [B, N] at the current powers, per env."""
        mbps = env.evaluate(rb_plane[:, None, :].contiguous(), pwr[:, None, :].contiguous(), planes=())['total_mbps'][:, 0]
        out[what] = float(mbps.double().mean())
        print(f'  {what:<38} {out[what]:9.2f} Mbps per env{note}')

    print(f'{NUM_ENVS} envs x ({cues} CUEs + {dues} pairs) on {rbs} RBs; total capacity, scored by evaluate()')
    report('random actions', rb)
    try:
        report('assign_rbs()', env.assign_rbs().rb.clone())
    except ValueError as why:                                        # more pairs than RBs: one pair per RB cannot be had
        out['assign_rbs()'] = 'ValueError'
        print(f'  {"assign_rbs()":<38} ValueError: {why}')
    res = env.color_rbs(MARGIN)
    report(f'color_rbs({MARGIN:g} dB)', res.rb.clone(), f'   ({float((res.proper != 0).float().mean()):.0%} proper)')
    for rb_pref in ('harm', 'total'):
        res = env.stable_rbs(quota=quota, rb_pref=rb_pref)
        note = f'   ({float(res.proposals.float().mean()):.1f} proposals, {float(res.unmatched.float().mean()):.1f} pairs unmatched)'
        report(f"stable_rbs(quota={quota}, rb_pref='{rb_pref}')", res.rb.clone(), note)
    # the step that takes the actions exports that rb
    want = env.stable_rbs(quota=quota).rb.clone()
    _, _, _, info = env.step(env.stable_rbs_actions(quota=quota))
    assert torch.equal(info['rb'], want)
    env.close()

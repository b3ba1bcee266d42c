"""The interference-graph colouring baseline of the D2D-underlay literature (VecD2DEnv.color_rbs(): the SIR conflict graph from
coupling() and the power plane, coloured by DSATUR in one launch of csrc/d2d_color.hip), beside the other RB allocators, on the same
layouts and scored by evaluate().

Two links are joined by an edge when one of them alone would hold the other's signal-to-interference ratio under the margin; the
graph is coloured with the RBs, and compatible pairs may share one.  That makes it the one cooperative allocator here that serves
MORE pairs than RBs: assign_rbs() places one pair per RB and refuses such a shape by name.  A larger margin joins more links - fewer
may share - until the graph cannot be coloured properly any more and the rule degrades to the least-conflicting RB.  A heuristic:
where proper is 1 the pairwise margins hold; nothing is said about the aggregate SINR, and there is no optimality certificate."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))      # run from a checkout without installing

import torch

from gym_d2d_amd.envs import VecD2DEnv
from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction

NUM_ENVS, MARGINS = 64, (15.0, 30.0)
SHAPES = {'one-to-one: 16 + 16 links on 32 RBs': (16, 16, 32), 'many-to-one: 6 + 24 links on 8 RBs': (6, 24, 8)}
results = {}

for label, (cues, dues, rbs) in SHAPES.items():
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
        print(f'  {what:<34} {out[what]:9.2f} Mbps per env{note}')

    print(f'{NUM_ENVS} envs x ({cues} CUEs + {dues} pairs) on {rbs} RBs; total capacity, scored by evaluate()')
    report('random actions', rb)
    dyn = env.best_response_dynamics()
    report('best_response_dynamics()', dyn.rb.clone(), f'   ({float(dyn.converged.float().mean()):.0%} converged)')
    try:
        report('assign_rbs()', env.assign_rbs().rb.clone())
    except ValueError as why:                                        # more pairs than RBs: one pair per RB cannot be had
        out['assign_rbs()'] = 'ValueError'
        print(f'  {"assign_rbs()":<34} ValueError: {why}')
    for margin in MARGINS:
        for pack in (False, True):
            res = env.color_rbs(margin, pack=pack)
            note = (f'   ({float((res.proper != 0).float().mean()):.0%} proper, {float(res.rbs_used.float().mean()):.1f} RBs used, '
                    f'{float(res.conflicts.float().mean()):.1f} conflicts)')
            report(f'color_rbs({margin:g} dB, pack={pack})', res.rb.clone(), note)
    # the step that takes the actions exports that rb
    want = env.color_rbs(MARGINS[0]).rb.clone()
    _, _, _, info = env.step(env.color_rbs_actions(MARGINS[0]))
    assert torch.equal(info['rb'], want)
    env.close()

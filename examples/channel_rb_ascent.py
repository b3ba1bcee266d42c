"""Cooperative RB ascent on a realistic channel: raise the total capacity on the live path-loss table, then step the solved RBs.

A SpatialChannelPathLoss env (log-distance median plus spatially consistent shadowing) is one of the table routes: rb_ascent() has no
law to evaluate there, rb_ascent_table() runs the same local search on the table the step reads.  With fading=None and nothing
moving, that table is the next step's, so the planes the solver returns are the planes step() then exports, bit for bit.

    python examples/channel_rb_ascent.py
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch                                                               # noqa: E402

from gym_d2d_amd.envs import VecD2DEnv                                    # noqa: E402
from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss   # noqa: E402

ENVS, CUES, PAIRS, RBS = 64, 6, 10, 6


class ShadowedChannel(SpatialChannelPathLoss):
    median, median_kwargs = LogDistancePathLoss, {'ple': 3.5}
    shadow_std_dB, fading = 8.0, None


def totals(capacity_mbps):
    """Per-env totals of a capacity plane [B, N], summed in double on the host."""
    return capacity_mbps.detach().cpu().numpy().astype('float64').sum(axis=1)


def main():
    env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'path_loss_model': ShadowedChannel, 'seed': 7},
                    num_envs=ENVS)
    env.reset(seed=1)
    gen = torch.Generator(device=env.device).manual_seed(5)
    levels = [env.num_pwr_actions['cue']] * CUES + [env.num_pwr_actions['due']] * PAIRS     # action = rb * levels + power level
    highs = RBS * torch.as_tensor(levels, device=env.device)
    draws = torch.randint(0, 2 ** 31 - 1, (ENVS, env.num_agents), generator=gen, device=env.device)
    _, _, _, info = env.step((draws % highs).to(torch.int32))              # uniformly random actions
    random_mbps = totals(info['capacity_mbps'])
    res = env.rb_ascent_table()                                            # the live table, the decoded planes of that step
    solved_mbps, domain = totals(res.capacity_mbps), int(res.domain.sum())
    rounds, moves, converged = (t.cpu().numpy() for t in (res.rounds, res.moves, res.converged))
    _, _, _, info = env.step(env.rb_ascent_table_actions())                # the same solve as actions: solved RBs, held powers
    delivered_mbps = totals(info['capacity_mbps'])
    results = {'random_mbps': random_mbps, 'rb_ascent_table_mbps': solved_mbps, 'delivered_mbps': delivered_mbps, 'domain': domain}
    print(f'{ENVS} envs, {CUES} + {PAIRS} links on {RBS} RBs, shadowed channel without fading')
    print(f'  random actions          {random_mbps.mean():10.3f} Mbps per env')
    print(f'  rb_ascent_table()       {solved_mbps.mean():10.3f} Mbps per env ({moves.mean():.1f} moves in {rounds.mean():.1f} rounds, '
          f'{int(converged.sum())} of {ENVS} converged)')
    print(f'  delivered by step()     {delivered_mbps.mean():10.3f} Mbps per env (largest gap {abs(delivered_mbps - solved_mbps).max():.1e})')
    env.close()
    return results


if __name__ == '__main__':
    results = main()

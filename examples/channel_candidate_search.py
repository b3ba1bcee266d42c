"""Random shooting on a realistic channel: score K candidate joint actions per env on the live path-loss table, step the best one.

A SpatialChannelPathLoss env (log-distance median plus spatially consistent shadowing) is one of the table routes: evaluate() has no
law to evaluate there, evaluate_table() reads the table the step reads.  With fading=None and nothing moving, that table is the
next step's, so the predicted total of the chosen candidate is what step() then delivers - bit for bit on the planes, and the
totals agree to float32 rounding.

    python examples/channel_candidate_search.py
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch                                                               # noqa: E402

from gym_d2d_amd.envs import VecD2DEnv                                    # noqa: E402
from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss   # noqa: E402

ENVS, CUES, PAIRS, RBS, K = 64, 6, 10, 6, 256


class ShadowedChannel(SpatialChannelPathLoss):
    median, median_kwargs = LogDistancePathLoss, {'ple': 3.5}
    shadow_std_dB, fading = 8.0, None


def main():
    env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'path_loss_model': ShadowedChannel, 'seed': 7},
                    num_envs=ENVS)
    env.reset(seed=1)
    gen = torch.Generator(device=env.device).manual_seed(5)
    highs = torch.as_tensor(env._initial_action_highs(), device=env.device)
    # K uniformly random action sets per env, in step()'s layout
    draws = torch.randint(0, 2 ** 31 - 1, (ENVS, K, env.num_agents), generator=gen, device=env.device)
    candidates = (draws % highs).to(torch.int32)
    scores = env.evaluate_table_actions(candidates, planes=())             # totals only: no [B, K, N] block is written
    assert int(scores['domain'].sum()) == 0
    predicted, best = scores['total_mbps'].max(dim=1)
    actions = candidates[torch.arange(ENVS, device=env.device), best].contiguous()
    _, _, _, info = env.step(actions)
    delivered = info['capacity_mbps'].sum(dim=1)
    mean_candidate = scores['total_mbps'].mean(dim=1)
    results = {'predicted_mbps': float(predicted.mean()), 'delivered_mbps': float(delivered.mean()),
               'mean_candidate_mbps': float(mean_candidate.mean()),
               'max_rel_gap': float(((predicted - delivered).abs() / delivered.clamp_min(1.0)).max())}
    print(f'{ENVS} envs, {CUES} + {PAIRS} links on {RBS} RBs, best of {K} random candidates per env')
    print(f'  mean candidate        {results["mean_candidate_mbps"]:10.3f} Mbps per env')
    print(f'  best candidate        {results["predicted_mbps"]:10.3f} Mbps per env (predicted by evaluate_table_actions)')
    print(f'  delivered by step()   {results["delivered_mbps"]:10.3f} Mbps per env (largest relative gap {results["max_rel_gap"]:.1e})')
    env.close()
    return results


if __name__ == '__main__':
    results = main()

"""Difference rewards under shadowing and Rayleigh fading: per-agent credit on a realistic channel.

A SpatialChannelPathLoss env is one of the table routes: marginal_capacity() has no law to evaluate there.
TableDifferenceRewardFunction makes step() return D_i = G(a) - G(a without link i), G the total capacity, computed by one extra
kernel launch on the table the step just read.  The self-check recomputes it the long way: evaluate_table() on the same table with
N + 1 candidates per env - the state, and the state with link i on no RB - and harm_i as what the OTHER links gain.

    python examples/channel_difference_reward.py
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch                                                               # noqa: E402

from gym_d2d_amd.envs import TableDifferenceRewardFunction, VecD2DEnv     # noqa: E402
from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss   # noqa: E402

ENVS, CUES, PAIRS, RBS = 32, 6, 10, 4


class FadingChannel(SpatialChannelPathLoss):
    median, median_kwargs = LogDistancePathLoss, {'ple': 3.5}
    shadow_std_dB, fading = 8.0, 'rayleigh'


def leave_one_out(env, info):
    """(difference, harm) float64 [B, N] by evaluate_table(): candidate 0 is the state, candidate i + 1 has link i on no RB."""
    n = env.num_links
    rb = info['rb'][:, None, :].repeat(1, n + 1, 1)
    idx = torch.arange(n, device=env.device)
    rb[:, idx + 1, idx] = -1
    pwr = info['tx_pwr_dbm'][:, None, :].repeat(1, n + 1, 1).contiguous()
    cap = env.evaluate_table(rb.contiguous(), pwr, planes=('capacity_mbps',))['capacity_mbps'].double()
    others = 1.0 - torch.eye(n, dtype=torch.float64, device=env.device)
    harm = ((cap[:, 1:] - cap[:, :1]) * others).sum(dim=2)
    return cap[:, 0] - harm, harm


def main():
    env = VecD2DEnv({'num_rbs': RBS, 'num_cues': CUES, 'num_due_pairs': PAIRS, 'path_loss_model': FadingChannel, 'seed': 7,
                     'reward_fn': TableDifferenceRewardFunction}, num_envs=ENVS)
    env.reset(seed=1)
    gen = torch.Generator(device=env.device).manual_seed(5)
    highs = torch.as_tensor(env._initial_action_highs(), device=env.device)
    worst, shared, total = 0.0, 0.0, 0.0
    for _ in range(3):
        actions = (torch.randint(0, 2 ** 31 - 1, (ENVS, env.num_agents), generator=gen, device=env.device) % highs).to(torch.int32)
        _, rewards, _, info = env.step(actions)
        want, harm = leave_one_out(env, info)
        worst = max(worst, float(((rewards.double() - want).abs() / want.abs().clamp_min(1.0)).max()))
        shared += float(info['capacity_mbps'].sum(dim=1).mean())
        total += float(rewards.sum(dim=1).mean())
    results = {'max_rel_gap': worst, 'mean_capacity_mbps': shared / 3, 'mean_difference_mbps': total / 3,
               'harmful_links': float((harm > 0).double().mean())}
    print(f'{ENVS} envs, {CUES} + {PAIRS} links on {RBS} RBs, shadowing 8 dB and Rayleigh fading, three steps')
    print(f'  total capacity              {results["mean_capacity_mbps"]:10.3f} Mbps per env')
    print(f'  sum of difference rewards   {results["mean_difference_mbps"]:10.3f} Mbps per env')
    print(f'  links that cost others      {results["harmful_links"]:10.1%}')
    print(f'  self-check against a leave-one-out by evaluate_table(): largest relative gap {worst:.1e}')
    env.close()
    return results


if __name__ == '__main__':
    results = main()

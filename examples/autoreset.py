"""A staggered rollout with per-env autoreset: done envs start their next episode inside step(), on the GPU.

With autoreset=True, the step() after the one that returned dones[b] = True resets env b instead of stepping it (new positions,
the reset's random actions, one step), returns its obs with reward 0 and marks it in info['reset'].  reset(elapsed=...) staggers
the first episodes, so the batch does not hold one episode phase; request_reset(mask) resets chosen envs at the next step.
Nothing here synchronises the host until the final print.

    python examples/autoreset.py
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np                                                        # noqa: E402
import torch                                                              # noqa: E402

from gym_d2d_amd.envs import VecD2DEnv                                    # noqa: E402


def main():
    b, horizon = 256, 32
    env = VecD2DEnv({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25, 'seed': 7}, num_envs=b, autoreset=True)
    env.reset(seed=1, elapsed=np.arange(b) % 10)                         # env b's first episode lasts 10 - b % 10 steps
    highs = torch.as_tensor(env._initial_action_highs(), device=env.device)
    rewards = torch.empty((horizon, b, env.num_links), device=env.device)
    dones = torch.empty((horizon, b), dtype=torch.bool, device=env.device)
    resets = torch.empty((horizon, b), dtype=torch.bool, device=env.device)
    for t in range(horizon):
        if t == 20:
            env.request_reset(torch.arange(b, device=env.device) < 8)     # reset the first eight envs at the next step
        actions = (torch.rand((b, env.num_agents), device=env.device) * highs).to(torch.int32)
        _, r, d, info = env.step(actions)
        rewards[t], dones[t], resets[t] = r, d, info['reset']             # dones / info['reset'] are reused: copy them
    print(f'{int(dones.sum())} episodes ended, {int(resets.sum())} envs reset, '
          f'{int(dones.any(1).sum())} of {horizon} steps had a done env, mean reward {float(rewards.mean()):.3f}')
    env.close()


if __name__ == '__main__':
    main()

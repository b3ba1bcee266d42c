"""A stochastic path-loss model evaluated on every step: COST-231 Hata plus log-normal shadowing as a per-step ArrayPathLoss.

The reference calls its PathLoss on every step (path_loss.py:12-25), so a model that draws a random number per call gets fresh
draws each step.  ArrayPathLoss with `per_step = True` keeps that: compute(view) runs on the GPU before every step, the step
inside reset() included, and the step kernel reads its [B, N+1, N] dB table in place.  view.normal() is the built-in
ShadowingPathLoss's normal stream (same counter, same seed rule), so the draws are reproducible and independent of how envs
are chunked or sharded.

    python examples/per_step_path_loss.py
"""
import math
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from gym_d2d_amd.envs import VecD2DEnv                                    # noqa: E402
from gym_d2d_amd.path_loss import ArrayPathLoss                           # noqa: E402


class ShadowedCostHata(ArrayPathLoss):
    """COST-231 Hata (suburban, path_loss.py:90-123) + N(0, chi^2) dB shadowing on every evaluation, the SNR's included."""
    per_step = True

    def __init__(self, carrier_freq_GHz, chi_dB=6.0):
        super().__init__(carrier_freq_GHz)
        self.chi_dB = float(chi_dB)

    def compute(self, view):
        xp, log_f = view.xp, math.log10(self.carrier_freq_GHz * 1000.0)
        h_tx = view.tx_column(lambda d: d.antenna_height_m)
        h_rx = view.rx_column(lambda d: d.antenna_height_m)
        a_hrx = (1.1 * log_f - 0.7) * h_rx - (1.56 * log_f - 0.8)
        d_km = view.distance() / 1000.0
        pl = 46.3 + 33.9 * log_f - 13.82 * xp.log10(h_tx) - a_hrx + (44.9 - 6.55 * xp.log10(h_tx)) * xp.log10(d_km)
        if xp.__name__ == 'torch':
            own = xp.diagonal(pl, dim1=1, dim2=2)
        else:
            own = xp.diagonal(pl, axis1=1, axis2=2)
        # every evaluation draws anew: the interferers' and the signal's (kind 0), and the SNR's second look (kind 1)
        return pl + self.chi_dB * view.normal(0), own + self.chi_dB * view.normal(1)


def main():
    env = VecD2DEnv({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25, 'path_loss_model': ShadowedCostHata, 'seed': 7},
                    num_envs=256)
    env.reset(seed=1)
    actions = env.action_buffer().clone()
    for k in range(3):
        _, rewards, _, info = env.step(actions)            # same actions, fresh shadowing: the SINRs move
        print(f'step {k}: mean SINR {float(info["sinr_db"].mean()):.3f} dB, mean reward {float(rewards.mean()):.3f}')
    env.close()


if __name__ == '__main__':
    main()

"""Reward plugins (mirrors gym_d2d/envs/reward_fn.py).  The three built-ins are evaluated inside the HIP step
kernel (csrc/d2d_step.hip, pass 3); `native_id` / `native_param` select the branch.  Calling a built-in with a
NativeState just re-keys the kernel's per-agent output.  A user subclass that overrides __call__ runs as Python.
DifferenceRewardFunction and GoodputRewardFunction are the array-native ones: VecD2DEnv hands them the planes of csrc/d2d_marginal.hip
and csrc/d2d_queue.hip; TableDifferenceRewardFunction gets those of csrc/d2d_tabmarg.hip on the table routes."""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Dict

from .. import _native


class RewardFunction(ABC):
    native_id = _native.REWARD_NONE

    @property
    def native_param(self) -> float:
        return 0.0

    @abstractmethod
    def __call__(self, actions, state: dict) -> Dict[str, float]:
        """Reward per 'tx:rx' agent id."""

    def _from_kernel(self, actions, state) -> Dict[str, float]:
        got = getattr(state, 'native_reward', None)
        if got is None or getattr(state, 'native_reward_key', None) != (self.native_id, float(self.native_param)):
            raise RuntimeError(f'{type(self).__name__} is evaluated by the HIP step kernel; `state` must be the '
                               'NativeState of an env configured with this reward function')
        return dict(zip(map(':'.join, getattr(actions, 'data', actions).keys()), got.tolist()))


class SystemCapacityRewardFunction(RewardFunction):
    """Mean capacity over all links, or -1 for everyone if a D2D link shares an RB with a non-D2D link whose
    capacity is <= min_capacity_mbps (reward_fn.py:22-44)."""
    native_id = _native.REWARD_SYSTEM_CAPACITY

    def __init__(self, min_capacity_mbps=0.0) -> None:
        self.min_capacity_mbps = float(min_capacity_mbps)

    @property
    def native_param(self) -> float:
        return self.min_capacity_mbps

    def __call__(self, actions, state):
        return self._from_kernel(actions, state)


class ShannonRewardFunction(RewardFunction):
    """log2(1 + SINR) per agent, -1 below min_sinr dB (reward_fn.py:47-57)."""
    native_id = _native.REWARD_SHANNON

    def __init__(self, min_sinr=-70.0) -> None:
        self.min_sinr = float(min_sinr)

    @property
    def native_param(self) -> float:
        return self.min_sinr

    def __call__(self, actions, state):
        return self._from_kernel(actions, state)


class CueSinrShannonRewardFunction(RewardFunction):
    """Own Shannon rate unless a non-D2D link on my RB has SINR below the threshold, then -1 (reward_fn.py:60-78)."""
    native_id = _native.REWARD_CUE_SINR_SHANNON

    def __init__(self, sinr_threshold_dB=0.0) -> None:
        self.sinr_threshold_dB = float(sinr_threshold_dB)

    @property
    def native_param(self) -> float:
        return self.sinr_threshold_dB

    def __call__(self, actions, state):
        return self._from_kernel(actions, state)


class DifferenceRewardFunction(RewardFunction):
    """Difference reward D_i = G(a) - G(a without link i), G the total capacity in Mbps: link i's own capacity minus the capacity
    its transmitter costs the other links of its RB (csrc/d2d_marginal.hip).  VecD2DEnv only: `needs_marginal` asks the env for
    view.difference_mbps / view.harm_mbps [B, N], one extra kernel launch per step; it is not one of the step kernel's rewards."""
    native_id = _native.REWARD_NONE
    needs_marginal = True

    def compute(self, view):
        return view.difference_mbps

    def __call__(self, actions, state):
        raise RuntimeError('DifferenceRewardFunction is computed from the batched planes of VecD2DEnv (marginal_capacity()); the '
                           'single-env dict D2DEnv does not serve it')


class TableDifferenceRewardFunction(RewardFunction):
    """DifferenceRewardFunction for the envs whose step reads a path-loss table ('channel', 'per_step', 'array' with an SNR row):
    D_i = G(a) - G(a without link i) on the table the step just read (csrc/d2d_tabmarg.hip).  VecD2DEnv only:
    `needs_table_marginal` asks the env for view.difference_mbps / view.harm_mbps [B, N], one extra kernel launch per step; an env
    without a live table, with export_actions=False or on the NumPy path refuses it at construction."""
    native_id = _native.REWARD_NONE
    needs_table_marginal = True

    def compute(self, view):
        return view.difference_mbps

    def __call__(self, actions, state):
        raise RuntimeError('TableDifferenceRewardFunction is computed from the batched planes of VecD2DEnv '
                           '(marginal_capacity_table()); the single-env dict D2DEnv does not serve it')


class GoodputRewardFunction(RewardFunction):
    """Delivered traffic per link in Mbps, less what was lost: (served_bits - drop_penalty * (expired_bits + overflow_bits)) /
    (1e6 * dt_s), float32 [B, N], formed in float64 and rounded once (VecD2DEnv(traffic=PacketTraffic(...)), csrc/d2d_queue.hip).
    A subclass sets another `drop_penalty`.  VecD2DEnv only; `needs_traffic` makes an env without traffic= refuse it at construction."""
    native_id = _native.REWARD_NONE
    needs_traffic = True
    drop_penalty = 1.0

    def compute(self, view):
        import torch
        f64 = torch.float64
        lost = view.expired_bits.to(f64) + view.overflow_bits.to(f64)
        return ((view.served_bits.to(f64) - float(self.drop_penalty) * lost) / view.traffic.bits_per_mbps_step).to(torch.float32)

    def __call__(self, actions, state):
        raise RuntimeError('GoodputRewardFunction is computed from the queue planes of VecD2DEnv(traffic=...); the single-env dict '
                           'D2DEnv does not serve it')

"""Target-SINR power control: the host side of libd2d_powerctl.so (include/d2d_powerctl.h, csrc/d2d_powerctl.hip).

`PowerControl` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds, unchanged, the
power bounds of every link's class) and launches the kernel on torch's device pointers.  `class_bounds` gives the bounds,
`encode_actions` turns the solved powers into the action tensor VecD2DEnv.step() takes.  Torch path only.  The refusal texts are the 'power_control' row of
sensing.REFUSALS; the out= check and the owned outputs (declare_outputs, outputs) and the launch prefix (launch_args) are PairKernel's.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .sensing import PairKernel, refusal_text


class PowerControlResult(NamedTuple):
    """What power_control() returns: a tuple with names."""
    power_dbm: object          # int32 [B, N]: the powers when the iteration stopped
    sinr_db: object            # float32 [B, N]: every link's SINR at those powers
    iters: object              # int32 [B]: the sweeps that changed a link; max_iters at the cap
    converged: object          # uint8 [B]: 1 - the fixed point was reached


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no power_control() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('power_control', sim, export_actions, use_torch)


def class_bounds(num_pwr_actions: dict, cue_kind: str, num_cues: int, num_due_pairs: int):
    """(p_min, p_max) int32 [N] of the default link list (CUE links first), in the dBm the step transmits.  The env's decoder takes
    a link's power as its action's level, action mod levels, and does not add due_min_tx_power_dBm back (d2d_env.py:94-96): what a
    DUE transmits runs over 0 .. due_max - due_min, a CUE over 0 .. cue_max, a base station over 0 .. mbs_max.  The bounds are the
    decoder's, so that a solved power is a power step() applies."""
    levels = np.asarray([num_pwr_actions[cue_kind]] * num_cues + [num_pwr_actions['due']] * num_due_pairs, dtype=np.int32)
    return np.zeros_like(levels), levels - 1


def encode_actions(rb, power_dbm, p_min, levels, first_agent: int = 0):
    """The action array [B, num_agents] that keeps every agent link on its RB at power_dbm: rb * levels + (power_dbm - p_min), the
    env's own layout (d2d_env.py:94-96).  rb, power_dbm: [B, N]; p_min, levels: int [num_agents], the lowest power and the number of
    power levels of every agent link's class; the agents are links first_agent .. first_agent + num_agents - 1 (links on fixed
    actions come first and have no column).  NumPy arrays or torch tensors alike; the result is int32."""
    n = first_agent + levels.shape[0]
    rb, power_dbm = rb[:, first_agent:n], power_dbm[:, first_agent:n]
    act = rb * levels + (power_dbm - p_min)
    if isinstance(act, np.ndarray):
        return act.astype(np.int32)
    import torch
    return act.to(torch.int32)


def link_values(kernel, values, num_cues: int, name: str):
    """float32 [N] on the kernel object's device from a scalar, {'cue': x, 'due': y} or [N] values (array or tensor), none of them
    NaN; `name` is what a refusal calls the argument.  The last host value is kept in kernel._target: a repeat is not uploaded again."""
    torch = kernel.torch
    if torch.is_tensor(values):
        t = values.to(device=kernel.device, dtype=torch.float32).contiguous()
        if tuple(t.shape) != (kernel.n,):
            raise ValueError(f'{name} must be a number, {{"cue": x, "due": y}} or [{kernel.n}] values')
        return t
    if isinstance(values, dict):
        if set(values) != {'cue', 'due'}:
            raise ValueError(f"{name} as a dict takes exactly the keys 'cue' and 'due'")
        host = np.asarray([values['cue']] * num_cues + [values['due']] * (kernel.n - num_cues), dtype=np.float32)
    else:
        host = np.asarray(values, dtype=np.float32)
        if host.ndim == 0:
            host = np.full(kernel.n, host, dtype=np.float32)
    if host.shape != (kernel.n,) or np.isnan(host).any():
        raise ValueError(f'{name} must be a number, {{"cue": x, "due": y}} or [{kernel.n}] values, none of them NaN')
    key = host.tobytes()
    if kernel._target is None or kernel._target[0] != key:
        kernel._target = (key, torch.as_tensor(host, device=kernel.device))
    return kernel._target[1]


class PowerControl(PairKernel):
    """The power-control kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, p_min, p_max, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='power_control', max_rbs=_native.POWERCTL_MAX_RBS)
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever adjusted
        if not (p_min.shape == p_max.shape == self.agent.shape == (self.n,)) or (p_min > p_max).any() or np.abs(p_max).max() >= 4096:
            raise ValueError('the power bounds do not match the env')
        self.declare_outputs(PowerControlResult._fields, ((self.b, self.n), (self.b, self.n), (self.b,), (self.b,)),
                             (torch.int32, torch.float32, torch.int32, torch.uint8))
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        self._target = None                          # (key, tensor) of the last call: a repeated target is not uploaded again

    def target(self, target_sinr_db, num_cues: int):
        """float32 [N] on the device from a scalar, {'cue': x, 'due': y} or [N] values (array or tensor)."""
        return link_values(self, target_sinr_db, num_cues, 'target_sinr_db')

    def adjustable(self, adjustable):
        """uint8 [N] on the device: the agent links (None), or those of them `adjustable` (bool [N], array or tensor) marks."""
        return self.agent_subset(adjustable, 'adjustable')

    def solve(self, t: dict, target, adjustable, max_iters: int, out, stream: int, env_mask=None) -> PowerControlResult:
        """target, adjustable: the tensors target() and adjustable() return."""
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 1:
            raise ValueError(f'max_iters must be an int >= 1, got {max_iters!r}')
        power, sinr, iters, conv = self.outputs(out)
        mask = self.env_mask(env_mask)               # lives until the launch is enqueued; the stream orders its release behind it
        _native.power_control(*self.launch_args(t), target.data_ptr(), self.p_min.data_ptr(), self.p_max.data_ptr(), adjustable.data_ptr(),
                              int(max_iters), 0 if mask is None else mask.data_ptr(), power.data_ptr(), sinr.data_ptr(),
                              iters.data_ptr(), conv.data_ptr(), stream)
        return PowerControlResult(power, sinr, iters, conv)

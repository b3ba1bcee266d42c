"""Sum-capacity power ascent with SINR floors: the host side of libd2d_ascent.so (include/d2d_ascent.h, csrc/d2d_ascent.hip).

`PowerAscent` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns and
sensing.fold_capacity_columns fold, unchanged, the power bounds of every link's class) and launches the ascent on torch's device
pointers: one launch per call, every turn of every round of every env inside it.  `lds_bytes` restates the header's formula.  The
floor is power_control.link_values, the action encoding is power_control.encode_actions.  Torch path only.  The refusal texts are
`REFUSAL`, power_control()'s row of sensing.REFUSALS under this name with a shadowing clause of its own; the out= check, the owned
outputs and the launch prefix are PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .power_control import link_values
from .sensing import REFUSALS, PairKernel, r16, refusal_text

REFUSAL = ('power_ascent()', *REFUSALS['power_control'][1:3],
           'ascent (the capacity a move was made for is another draw than the one the next link sees)', 'planes')
STARTS = {'held': _native.ASCENT_START_HELD, 'min': _native.ASCENT_START_MIN, 'max': _native.ASCENT_START_MAX}


class PowerAscentResult(NamedTuple):
    """What power_ascent() returns: a tuple with names."""
    power_dbm: object          # int32 [B, N]: the powers the ascent ended at
    sinr_db: object            # float32 [B, N]: evaluate()'s plane for (rb, power_dbm)
    capacity_mbps: object      # float32 [B, N]: likewise
    rounds: object             # int32 [B]: the rounds that moved a link, the largest count over the RB groups; max_rounds at the cap
    moves: object              # int32 [B]: the moves made, over all groups
    converged: object          # uint8 [B]: 1 - every group saw a round that moved nobody


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no power_ascent() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def lds_bytes(n: int, r: int, power_law: bool) -> int:
    """The LDS one workgroup of d2d_power_ascent needs: the formula of include/d2d_ascent.h."""
    n4 = (n + 3) & ~3
    return 48 * n + (r16(8 * n) if power_law else 0) + 20 * n4 + r16(4 * (r + 1)) + 64


class PowerAscent(PairKernel):
    """The ascent kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, p_min, p_max, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='power_ascent', max_rbs=_native.ASCENT_MAX_RBS, capacity=True)
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever adjusted
        if not (p_min.shape == p_max.shape == self.agent.shape == (self.n,)) or (p_min > p_max).any() \
                or max(np.abs(p_max).max(), np.abs(p_min).max()) >= 4096:
            raise ValueError('the power bounds do not match the env')
        levels = int((p_max.astype(np.int64) - p_min + 1)[self.agent].max()) if self.agent.any() else 1
        if levels > _native.ASCENT_MAX_LEVELS:
            raise ValueError(f'power_ascent() gives every power level of a link a lane of one wave: at most {_native.ASCENT_MAX_LEVELS} '
                             f'levels (D2D_ASCENT_MAX_LEVELS), got {levels}')
        need = lds_bytes(self.n, self.r, self.law != _native.ASCENT_LAW_INV_SQUARE)
        if need > _native.ASCENT_MAX_LDS_BYTES:
            raise ValueError(f'power_ascent() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} bytes, '
                             f'more than {_native.ASCENT_MAX_LDS_BYTES}')
        self.declare_outputs(PowerAscentResult._fields, ((self.b, self.n),) * 3 + ((self.b,),) * 3,
                             (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8))
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        self._target = None                          # (key, tensor) of the last host floor: a repeat is not uploaded again

    def floor(self, floor_sinr_db, num_cues: int):
        """float32 [N] on the device from None (no floors: -inf), a scalar, {'cue': x, 'due': y} or [N] values (array or tensor);
        -inf: that link has no floor."""
        return link_values(self, -np.inf if floor_sinr_db is None else floor_sinr_db, num_cues, 'floor_sinr_db')

    def adjustable(self, adjustable):
        """uint8 [N] on the device: the agent links (None), or those of them `adjustable` (bool [N], array or tensor) marks."""
        return self.agent_subset(adjustable, 'adjustable')

    def solve(self, t: dict, adjustable, floor, start: str, min_gain_mbps: float, max_rounds: int, out, stream: int,
              env_mask=None) -> PowerAscentResult:
        """adjustable, floor: the tensors adjustable() and floor() return."""
        if not isinstance(start, str) or start not in STARTS:
            raise ValueError(f"start must be one of 'held', 'min', 'max', got {start!r}")
        if isinstance(min_gain_mbps, bool) or not isinstance(min_gain_mbps, (int, float, np.integer, np.floating)) \
                or not math.isfinite(min_gain_mbps) or min_gain_mbps < 0:
            raise ValueError(f'min_gain_mbps must be a finite number >= 0, got {min_gain_mbps!r}')
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or not 1 <= max_rounds <= _native.ASCENT_MAX_ROUNDS:
            raise ValueError(f'max_rounds must be an int in [1, {_native.ASCENT_MAX_ROUNDS}], got {max_rounds!r}')
        res = self.outputs(out)
        mask = self.env_mask(env_mask)               # lives until the launch is enqueued; the stream orders its release behind it
        _native.power_ascent(*self.launch_args(t), self.p_min.data_ptr(), self.p_max.data_ptr(), adjustable.data_ptr(), floor.data_ptr(),
                             STARTS[start], float(min_gain_mbps), int(max_rounds), 0 if mask is None else mask.data_ptr(),
                             *(o.data_ptr() for o in res), stream)
        return PowerAscentResult(*res)

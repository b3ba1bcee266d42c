"""Sum-capacity RB ascent with SINR floors: the host side of libd2d_rbascent.so (include/d2d_rbascent.h, csrc/d2d_rbascent.hip).

`RbAscent` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns and
sensing.fold_capacity_columns fold, unchanged) and launches the ascent on torch's device pointers: one launch per call, every turn
of every round of every env inside it.  `lds_bytes` restates the header's formula.  The allowed mask goes through
best_response.words / pack_allowed, the floor is power_control.link_values, the action encoding is
best_response_dynamics.encode_actions.  Torch path only.  The refusal texts are `REFUSAL`, best_response_dynamics()'s row of
sensing.REFUSALS under this name with a shadowing clause of its own; the out= check, the owned outputs and the launch prefix are
PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .power_control import link_values
from .sensing import REFUSALS, PairKernel, r16, refusal_text

REFUSAL = ('rb_ascent()', *REFUSALS['best_response_dynamics'][1:3],
           'ascent (the capacity a move was made for is another draw than the one the next link sees)', 'planes')


class RbAscentResult(NamedTuple):
    """What rb_ascent() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the RBs the ascent ended at
    sinr_db: object            # float32 [B, N]: evaluate()'s plane for (rb, the held powers)
    capacity_mbps: object      # float32 [B, N]: likewise
    rounds: object             # int32 [B]: the rounds that moved a link; max_rounds at the cap
    moves: object              # int32 [B]: the moves made
    converged: object          # uint8 [B]: 1 - a round moved nobody


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no rb_ascent() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def lds_bytes(n: int, r: int, power_law: bool, allowed: bool = False) -> int:
    """The LDS one workgroup of d2d_rb_ascent needs: the formula of include/d2d_rbascent.h."""
    n4 = (n + 3) & ~3
    return (48 * n + (r16(8 * n) if power_law else 0) + 8 * n4 + (r16(4 * n * ((r + 31) // 32)) if allowed else 0)
            + r16(4 * ((n + 31) // 32) * r) + 112)


class RbAscent(PairKernel):
    """The ascent kernel bound to one env object: constants uploaded once, one launch per call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='rb_ascent', max_rbs=_native.RBASCENT_MAX_RBS, capacity=True)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever moved
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        self.need(False)                                             # a shape no call could serve is refused when the object is made
        self.declare_outputs(RbAscentResult._fields, ((self.b, self.n),) * 3 + ((self.b,),) * 3,
                             (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8))
        self._target = None                          # (key, tensor) of the last host floor: a repeat is not uploaded again

    def need(self, allowed: bool) -> int:
        """lds_bytes of this env, with or without an allowed mask; ValueError past the limit, stating the byte count."""
        need = lds_bytes(self.n, self.r, self.law != _native.RBASCENT_LAW_INV_SQUARE, allowed)
        if need > _native.RBASCENT_MAX_LDS_BYTES:
            raise ValueError(f'rb_ascent() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} bytes'
                             f'{" with an allowed mask" if allowed else ""}, more than {_native.RBASCENT_MAX_LDS_BYTES}')
        return need

    def floor(self, floor_sinr_db, num_cues: int):
        """float32 [N] on the device from None (no floors: -inf), a scalar, {'cue': x, 'due': y} or [N] values (array or tensor);
        -inf: that link has no floor."""
        return link_values(self, -np.inf if floor_sinr_db is None else floor_sinr_db, num_cues, 'floor_sinr_db')

    def movable(self, movable):
        """uint8 [N] on the device: the agent links (None), or those of them `movable` (bool [N], array or tensor) marks."""
        return self.agent_subset(movable, 'movable')

    def solve(self, t: dict, allowed, movable, floor, min_gain_mbps: float, max_rounds: int, out, stream: int,
              env_mask=None) -> RbAscentResult:
        """movable, floor: the tensors movable() and floor() return; allowed: what the caller passed."""
        if isinstance(min_gain_mbps, bool) or not isinstance(min_gain_mbps, (int, float, np.integer, np.floating)) \
                or not math.isfinite(min_gain_mbps) or min_gain_mbps < 0:
            raise ValueError(f'min_gain_mbps must be a finite number >= 0, got {min_gain_mbps!r}')
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) \
                or not 1 <= max_rounds <= _native.RBASCENT_MAX_ROUNDS:
            raise ValueError(f'max_rounds must be an int in [1, {_native.RBASCENT_MAX_ROUNDS}], got {max_rounds!r}')
        self.need(allowed is not None)
        res = self.outputs(out)
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        mask = self.env_mask(env_mask)
        _native.rb_ascent(*self.launch_args(t), 0 if words is None else words.data_ptr(), movable.data_ptr(), floor.data_ptr(),
                          float(min_gain_mbps), int(max_rounds), 0 if mask is None else mask.data_ptr(),
                          *(o.data_ptr() for o in res), stream)
        return RbAscentResult(*res)

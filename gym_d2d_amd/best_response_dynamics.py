"""Sequential best-response RB dynamics: the host side of libd2d_brdyn.so (include/d2d_brdyn.h, csrc/d2d_brdyn.hip).

`BestResponseDynamics` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds,
unchanged) and launches the kernel on torch's device pointers; the allowed mask goes through best_response.words / pack_allowed.
`encode_actions` turns the solved RBs into the action tensor VecD2DEnv.step() takes.  Torch path only.  The refusal texts are the 'best_response_dynamics' row of
sensing.REFUSALS; the out= check and the owned outputs (declare_outputs, outputs), the launch prefix (launch_args) and r16 are PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .sensing import PairKernel, r16, refusal_text


class BestResponseDynamicsResult(NamedTuple):
    """What best_response_dynamics() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the RBs when the dynamics stopped
    sinr_db: object            # float32 [B, N]: every link's SINR on those RBs
    rounds: object             # int32 [B]: the rounds that moved a link; max_rounds at the cap
    moves: object              # int32 [B]: the moves made
    converged: object          # uint8 [B]: 1 - a round moved nobody


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no best_response_dynamics() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('best_response_dynamics', sim, export_actions, use_torch)


def lds_bytes(num_links: int, num_rbs: int, power_law: bool, allowed: bool) -> int:
    """The LDS one workgroup of the kernel needs (the header's formula): at most _native.BRDYN_MAX_LDS_BYTES is served."""
    n, n4 = num_links, (num_links + 3) & ~3
    return (32 * n + (r16(8 * n) if power_law else 0) + 12 * n4 + (r16(4 * n * ((num_rbs + 31) // 32)) if allowed else 0)
            + r16(4 * ((n + 31) // 32) * num_rbs) + 80)


def encode_actions(rb, pwr, levels, first_agent: int = 0):
    """The action array [B, num_agents] that puts every agent link on rb at its current power level: rb * levels + power level, the
    env's own layout (d2d_env.py:94-96).  rb, pwr: [B, N] (the solved RBs, the decoded power plane); levels: int [num_agents], the
    power levels of every agent link's class; the agents are links first_agent .. first_agent + num_agents - 1 (links on fixed
    actions come first and have no column).  NumPy arrays or torch tensors alike; the result is int32."""
    n = first_agent + levels.shape[0]
    act = rb[:, first_agent:n] * levels + pwr[:, first_agent:n]
    if isinstance(act, np.ndarray):
        return act.astype(np.int32)
    import torch
    return act.to(torch.int32)


class BestResponseDynamics(PairKernel):
    """The dynamics kernel bound to one env object: constants uploaded once, one launch per call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='best_response_dynamics', max_rbs=_native.BRDYN_MAX_RBS)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever moved
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        self.declare_outputs(BestResponseDynamicsResult._fields, ((self.b, self.n), (self.b, self.n), (self.b,), (self.b,), (self.b,)),
                             (torch.int32, torch.float32, torch.int32, torch.int32, torch.uint8))

    def movable(self, movable):
        """uint8 [N] on the device: the agent links (None), or those of them `movable` (bool [N], array or tensor) marks."""
        return self.agent_subset(movable, 'movable')

    def solve(self, t: dict, allowed, movable, min_gain_db: float, max_rounds: int, out, stream: int,
              env_mask=None) -> BestResponseDynamicsResult:
        """movable: the tensor movable() returns; allowed: what the caller passed."""
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or not 0 <= max_rounds <= _native.BRDYN_MAX_ROUNDS:
            raise ValueError(f'max_rounds must be an int in [0, {_native.BRDYN_MAX_ROUNDS}], got {max_rounds!r}')
        if isinstance(min_gain_db, bool) or not isinstance(min_gain_db, (int, float, np.integer, np.floating)) \
                or math.isnan(min_gain_db) or min_gain_db < 0.0:
            raise ValueError(f'min_gain_db must be a number >= 0, got {min_gain_db!r}')
        need = lds_bytes(self.n, self.r, self.law != _native.BRDYN_LAW_INV_SQUARE, allowed is not None)
        if need > _native.BRDYN_MAX_LDS_BYTES:
            raise ValueError(f'best_response_dynamics() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need '
                             f'{need} bytes, more than the {_native.BRDYN_MAX_LDS_BYTES} a workgroup can have')
        rb, sinr, rounds, moves, conv = self.outputs(out)
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        mask = self.env_mask(env_mask)
        _native.best_response_dynamics(*self.launch_args(t), 0 if words is None else words.data_ptr(), movable.data_ptr(),
                                       float(min_gain_db), int(max_rounds), 0 if mask is None else mask.data_ptr(), rb.data_ptr(),
                                       sinr.data_ptr(), rounds.data_ptr(), moves.data_ptr(), conv.data_ptr(), stream)
        return BestResponseDynamicsResult(rb, sinr, rounds, moves, conv)

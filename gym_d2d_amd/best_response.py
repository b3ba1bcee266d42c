"""Best-response RB selection: the host side of libd2d_bestrb.so (include/d2d_bestrb.h, csrc/d2d_bestrb.hip).

`BestRb` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds, unchanged) and launches
the kernel on torch's device pointers.  `pack_allowed` lowers a bool [N, R] mask to the kernel's words, `encode_actions` turns the
kernel's planes into the action tensor VecD2DEnv.step() takes.  Torch path only.  The refusal texts are the 'best_rb' row of
sensing.REFUSALS; the out= check and the owned planes (declare_outputs, outputs) and the launch prefix (launch_args) are PairKernel's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .sensing import PairKernel, refusal_text


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no best_rb() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('best_rb', sim, export_actions, use_torch)


def pack_allowed(mask, xp=np):
    """bool [N, R] (link i may choose RB r) -> the kernel's words [N, ceil(R / 32)]: bit r & 31 of word r // 32.  NumPy: uint32;
    torch (xp=torch): int32 holding the same bits, on the mask's device."""
    n, r = mask.shape
    words = (r + 31) // 32
    if xp is np:
        bits = np.zeros((n, words * 32), dtype=np.uint64)
        bits[:, :r] = np.asarray(mask, dtype=bool)
        return (bits.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    bits = xp.zeros((n, words * 32), dtype=xp.int64, device=mask.device)
    bits[:, :r] = mask.to(xp.int64)
    word = (bits.view(n, words, 32) << xp.arange(32, dtype=xp.int64, device=mask.device)).sum(dim=2)
    return xp.where(word >= 1 << 31, word - (1 << 32), word).to(xp.int32)


def encode_actions(rb, pwr, best_rb, gain_db, levels, min_gain_db: float, first_agent: int = 0):
    """The action array [B, num_agents] that moves every agent link whose gain_db > min_gain_db to best_rb at its current power level
    and repeats the last action of every other one: rb * levels + power level, the env's own layout (d2d_env.py:94-96).  rb, pwr,
    best_rb, gain_db: [B, N] (the decoded planes and the kernel's); levels: int [num_agents], the power levels of every agent
    link's class; the agents are links first_agent .. first_agent + num_agents - 1 (links on fixed actions come first and have no
    column).  NaN gains (no allowed RB, an own rb outside [0, R)) compare false: such links repeat their last action.  NumPy arrays
    or torch tensors alike; the result is int32."""
    n = first_agent + levels.shape[0]
    rb, pwr, best_rb, gain_db = (a[:, first_agent:n] for a in (rb, pwr, best_rb, gain_db))
    move = gain_db > min_gain_db
    if isinstance(move, np.ndarray):
        return (np.where(move, best_rb, rb) * levels + pwr).astype(np.int32)
    import torch
    return (torch.where(move, best_rb, rb) * levels + pwr).to(torch.int32)


def words(kernel, allowed):
    """None, or the packed words of `allowed` (bool [N, R], tensor or array) as an int32 tensor on the device of `kernel` (a
    PairKernel with an RB count).  BestRb and BestResponseDynamics carry it as their method `words`."""
    if allowed is None:
        return None
    torch = kernel.torch
    mask = torch.as_tensor(allowed, device=kernel.device) if not torch.is_tensor(allowed) else allowed.to(kernel.device)
    if tuple(mask.shape) != (kernel.n, kernel.r) or mask.dtype != torch.bool:
        raise ValueError(f'allowed must be bool [{kernel.n}, {kernel.r}] (link, RB) or None')
    return pack_allowed(mask, torch).contiguous()


class BestRb(PairKernel):
    """The best-response kernel bound to one env object: constants uploaded once, one launch per call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='best_rb', max_rbs=_native.BESTRB_MAX_RBS)
        shape = (self.b, self.n)
        self.declare_outputs(('best_rb', 'best_sinr_db', 'gain_db'), (shape,) * 3, (torch.int32, torch.float32, torch.float32),
                             f'out must be (best_rb, best_sinr_db, gain_db): contiguous int32, float32, float32 tensors {list(shape)} '
                             f'on {device} that do not share memory')

    def planes(self, t: dict, allowed, out, stream: int, env_mask=None):
        best, sinr, gain = self.outputs(out)
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        _native.best_rb(*self.launch_args(t), 0 if words is None else words.data_ptr(), 0 if env_mask is None else env_mask.data_ptr(),
                        best.data_ptr(), sinr.data_ptr(), gain.data_ptr(), stream)
        return best, sinr, gain

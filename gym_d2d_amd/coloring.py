"""Conflict-graph RB colouring: the host side of libd2d_color.so (include/d2d_color.h, csrc/d2d_color.hip).

`Coloring` is bound to one env object as the other pair kernels are and launches the kernel on torch's device pointers: the score,
bias and threshold tensors are the caller's (color_graph) or the SIR graph of the literature built from coupling() and the power
plane (`sir_threshold`, color_rbs); the movable links go through PairKernel.agent_subset, the allowed mask through
best_response.words, the margins through power_control.link_values.  The solved RBs become step()'s action tensor through
best_response_dynamics.encode_actions.  Torch path only.  The refusal texts are the 'color_rbs' row of
sensing.REFUSALS; the out= check and the owned outputs (declare_outputs, outputs), the single-tensor predicate (fits) and r16 are PairKernel's.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .power_control import link_values
from .sensing import PairKernel, r16, refusal_text


class ColoringResult(NamedTuple):
    """What color_graph() and color_rbs() return: a tuple with names."""
    rb: object                 # int32 [B, N]: the colours; background links keep their RB
    conflicts: object          # int32 [B]: same-RB edges with an end that took a turn
    rbs_used: object           # int32 [B]: the distinct RBs the links that took a turn hold
    proper: object             # uint8 [B]: 1 - conflicts == 0


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no color_rbs() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('color_rbs', sim, export_actions, use_torch)


def lds_bytes(num_links: int, num_rbs: int, allowed: bool) -> int:
    """The LDS one workgroup of the kernel needs (the header's formula): at most _native.COLOR_MAX_LDS_BYTES is served."""
    n, w, words = num_links, (num_links + 31) // 32, (num_rbs + 31) // 32
    return r16(4 * n * w) + (2 if allowed else 1) * r16(4 * n * words) + 3 * r16(4 * n) + 2 * r16(4 * num_rbs) + r16(4 * words) + 64


def sir_threshold(coupling, power, margin):
    """rx_thr [B, N] of the SIR conflict graph: (coupling[b, i, i] + power[b, i]) - margin[i], float32 in exactly that association.
    Link j alone holds link i's signal-to-interference ratio under margin[i] iff coupling[b, i, j] + power[b, j] >= rx_thr[b, i]:
    the receiver gains are on both sides.  coupling float32 [B, N, N], power float32 [B, N], margin float32 [N]; NumPy arrays or
    torch tensors alike."""
    return (coupling.diagonal(0, 1, 2) + power) - margin[None, :]


class Coloring(PairKernel):
    """The colouring kernel bound to one env object: one launch per call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='color_rbs', max_rbs=_native.COLOR_MAX_RBS)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever coloured
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        self.declare_outputs(ColoringResult._fields, ((self.b, self.n), (self.b,), (self.b,), (self.b,)),
                             (torch.int32, torch.int32, torch.int32, torch.uint8))
        self._target = None                          # (key, tensor) of the last margins: a repeat is not uploaded again

    def movable(self, movable):
        """uint8 [N] on the device: the agent links (None), or those of them `movable` (bool [N], array or tensor) marks."""
        return self.agent_subset(movable, 'movable')

    def margin(self, margin_db, num_cues: int):
        """float32 [N] on the device from a number, {'cue': x, 'due': y} or [N] values (array or tensor), dB; NaN is refused - in a
        TENSOR by reading it on the host, which waits for everything queued before it on its stream."""
        t = link_values(self, margin_db, num_cues, 'margin_db')
        if self.torch.is_tensor(margin_db) and bool(self.torch.isnan(t).any()):
            raise ValueError(f'margin_db must be a number, {{"cue": x, "due": y}} or [{self.n}] values, none of them NaN')
        return t

    def plane(self, value, name: str, shape, optional: bool = False):
        """`value` if it is a contiguous float32 tensor of `shape` on the env's device (None passes with optional), else ValueError
        under `name`."""
        if value is None and optional:
            return None
        if not self.fits(value, shape, self.torch.float32):
            raise ValueError(f'{name} must be a contiguous float32 tensor {list(shape)} on {self.device}' + (' or None' if optional else ''))
        return value

    def color(self, rb, score, rx_thr, tx_bias, movable, allowed, pack, out, stream: int) -> ColoringResult:
        """rb: the env's decoded RB plane; movable: the tensor movable() returns; allowed: what the caller passed."""
        score = self.plane(score, 'score', (self.b, self.n, self.n))
        rx_thr = self.plane(rx_thr, 'rx_thr', (self.b, self.n))
        tx_bias = self.plane(tx_bias, 'tx_bias', (self.b, self.n), optional=True)
        if not isinstance(pack, (bool, int)) or pack not in (0, 1):
            raise ValueError(f'pack must be True or False, got {pack!r}')
        need = lds_bytes(self.n, self.r, allowed is not None)
        if need > _native.COLOR_MAX_LDS_BYTES:
            raise ValueError(f'color_rbs() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} '
                             f'bytes, more than the {_native.COLOR_MAX_LDS_BYTES} (D2D_COLOR_MAX_LDS_BYTES) a workgroup can have')
        res = self.outputs(out)
        mask = self.words(allowed)                   # lives until the launch is enqueued; the stream orders its release behind it
        _native.color_graph(score.data_ptr(), 0 if tx_bias is None else tx_bias.data_ptr(), rx_thr.data_ptr(), rb.data_ptr(), self.b,
                            self.n, self.r, 0 if mask is None else mask.data_ptr(), movable.data_ptr(), bool(pack),
                            *(o.data_ptr() for o in res), stream)
        return ColoringResult(*res)

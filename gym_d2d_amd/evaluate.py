"""What-if evaluation of candidate joint actions: the host side of libd2d_evaluate.so (include/d2d_evaluate.h, csrc/d2d_evaluate.hip).

`Evaluate` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds and the capacity
columns sensing.fold_capacity_columns folds, both unchanged) and launches the kernel on torch's device pointers.  `decode_actions`
turns action tensors [B, K, num_agents] in step()'s layout into the (rb, tx power) planes [B, K, N] the kernel reads - the inverse of
best_response.encode_actions / power_control.encode_actions.  Torch path only.  The refusal texts are the 'evaluate' row of
sensing.REFUSALS; the out= predicate its dict goes through (all_fit) is PairKernel's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .sensing import PairKernel, refusal_text

PLANES = ('sinr_db', 'capacity_mbps')


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no evaluate() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('evaluate', sim, export_actions, use_torch)


def decode_actions(actions, levels, fixed_rb=None, fixed_pwr=None):
    """(rb, pwr), int32 [B, K, N] each: the planes step() would decode from every candidate action set.  actions: int
    [B, K, num_agents] in step()'s layout, rb * levels + power level (d2d_env.py:94-96), so rb = a // levels and pwr = a % levels
    (floor semantics, as the step decodes); levels: int [num_agents], the power levels of every agent link's class.  Links on fixed
    actions (cue_actions='traffic') come first and have no column: fixed_rb / fixed_pwr [B, F] hold their current entries (the
    env's rb / pwr planes), broadcast over K; None: there are none, N = num_agents.  NumPy arrays or torch tensors alike."""
    if actions.ndim != 3 or actions.shape[2] != levels.shape[0]:
        raise ValueError(f'actions must be [B, K, {levels.shape[0]}] (env, candidate, agent), got {list(actions.shape)}')
    b, k, _ = actions.shape
    if (fixed_rb is None) != (fixed_pwr is None):
        raise ValueError('fixed_rb and fixed_pwr come together')
    if isinstance(actions, np.ndarray):
        if actions.dtype.kind not in 'iu':
            raise ValueError(f'actions must be integers, got {actions.dtype}')
        a = actions.astype(np.int64)
        rb, pwr = np.floor_divide(a, levels), np.mod(a, levels)
        if fixed_rb is not None:
            f = fixed_rb.shape[1]
            rb = np.concatenate([np.broadcast_to(np.asarray(fixed_rb)[:, None, :], (b, k, f)), rb], axis=2)
            pwr = np.concatenate([np.broadcast_to(np.asarray(fixed_pwr)[:, None, :], (b, k, f)), pwr], axis=2)
        return np.ascontiguousarray(rb, dtype=np.int32), np.ascontiguousarray(pwr, dtype=np.int32)
    import torch
    if actions.dtype.is_floating_point or actions.dtype == torch.bool:
        raise ValueError(f'actions must be integers, got {actions.dtype}')
    a = actions.to(torch.int64)
    lv = torch.as_tensor(levels, device=a.device).to(torch.int64)
    rb = torch.div(a, lv, rounding_mode='floor')
    pwr = a - rb * lv
    if fixed_rb is not None:
        f = fixed_rb.shape[1]
        rb = torch.cat([fixed_rb[:, None, :].expand(b, k, f).to(torch.int64), rb], dim=2)
        pwr = torch.cat([fixed_pwr[:, None, :].expand(b, k, f).to(torch.int64), pwr], dim=2)
    return rb.to(torch.int32).contiguous(), pwr.to(torch.int32).contiguous()


class Evaluate(PairKernel):
    """The what-if kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='evaluate', max_rbs=_native.EVALUATE_MAX_RBS, capacity=True)
        self.own = {}                                # the tensors this object owns, by name; reallocated when K changes
        self.own_k = 0

    def _check_in(self, x, name: str):
        torch = self.torch
        if not (torch.is_tensor(x) and x.ndim == 3 and x.shape[0] == self.b and x.shape[2] == self.n and x.shape[1] >= 1
                and x.dtype == torch.int32 and x.is_contiguous() and x.device == self.device):
            raise ValueError(f'{name} must be a contiguous int32 tensor [{self.b}, K, {self.n}] (env, candidate, link) with K >= 1 on '
                             f'{self.device}')

    def planes(self, t: dict, rb, pwr, planes, out, stream: int) -> dict:
        torch = self.torch
        self._check_in(rb, 'rb')
        self._check_in(pwr, 'power_dbm')
        if tuple(rb.shape) != tuple(pwr.shape):
            raise ValueError(f'rb and power_dbm must have one shape, got {list(rb.shape)} and {list(pwr.shape)}')
        k = int(rb.shape[1])
        if k > _native.EVALUATE_MAX_CANDIDATES:
            raise ValueError(f'evaluate() serves at most {_native.EVALUATE_MAX_CANDIDATES} candidates per call (K = {k})')
        planes = (planes,) if isinstance(planes, str) else tuple(planes)
        if any(p not in PLANES for p in planes) or len(set(planes)) != len(planes):
            raise ValueError(f'planes must be a subset of {PLANES}, got {planes!r}')
        shapes = {'total_mbps': (self.b, k), **{p: (self.b, k, self.n) for p in planes}}
        if out is None:
            if self.own_k != k:
                self.own, self.own_k = {}, k
            for name, shape in shapes.items():
                if name not in self.own:
                    self.own[name] = torch.empty(shape, dtype=torch.float32, device=self.device)
            res = {name: self.own[name] for name in shapes}
        else:
            if not (isinstance(out, dict) and set(out) == set(shapes)
                    and self.all_fit([out[name] for name in shapes], list(shapes.values()), (torch.float32,) * len(shapes))):
                raise ValueError('out must be a dict of contiguous float32 tensors on ' + str(self.device) + ' that do not share '
                                 'memory: ' + ', '.join(f'{name} {list(shape)}' for name, shape in shapes.items()))
            res = {name: out[name] for name in shapes}
        _native.evaluate(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), rb.data_ptr(), pwr.data_ptr(), *self.ptrs, self.law, self.pow_k,
                         self.b, k, self.d, self.n, self.r, res['sinr_db'].data_ptr() if 'sinr_db' in res else 0,
                         res['capacity_mbps'].data_ptr() if 'capacity_mbps' in res else 0, res['total_mbps'].data_ptr(), stream)
        return res

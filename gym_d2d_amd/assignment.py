"""Optimal one-to-one RB matching: the host side of libd2d_assign.so (include/d2d_assign.h, csrc/d2d_assign.hip).

`Assignment` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds and the capacity
columns sensing.fold_capacity_columns folds, both unchanged) and launches the two kernels on torch's device pointers: the weight
planes of every movable link on every RB, and the maximum-weight matching of any such planes.  The allowed mask goes through
best_response.words / pack_allowed; the matched RBs become step()'s action tensor through best_response_dynamics.encode_actions.
Torch path only.  The refusal texts are the 'assign_rbs' row of
sensing.REFUSALS; the out= predicate (all_fit), the launch prefix (launch_args) and r16 are PairKernel's.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .sensing import PairKernel, r16, refusal_text

OBJECTIVES = {'total': _native.ASSIGN_OBJECTIVE_TOTAL, 'own': _native.ASSIGN_OBJECTIVE_OWN}


class AssignmentResult(NamedTuple):
    """What assign_rbs() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the current RBs with the movable links on their matched ones
    value_mbps: object         # float32 [B]: the sum of the matched weights; 0.0 where infeasible
    feasible: object           # uint8 [B]: 1 - every movable link has an RB of its own


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no assign_rbs() (None: it has): the predicate of sensing.unserved under evaluate()'s texts and this name."""
    return refusal_text('assign_rbs', sim, export_actions, use_torch)


def lds_bytes(num_links: int, num_rbs: int, power_law: bool) -> int:
    """The LDS one workgroup of the weights kernel needs (the header's formula): at most _native.ASSIGN_MAX_LDS_BYTES is served."""
    n, n4 = num_links, (num_links + 3) & ~3
    return 48 * n + (r16(8 * n) if power_law else 0) + r16(8 * n4) + 3 * r16(4 * n) + r16(4 * (num_rbs + 1))


def solve_lds_bytes(num_rows: int, num_cols: int) -> int:
    """The LDS one workgroup of the matching kernel needs (the header's formula): at most _native.ASSIGN_MAX_LDS_BYTES is served."""
    return r16(8 * num_rows) + 2 * r16(8 * num_cols) + 2 * r16(4 * num_cols) + r16(4 * num_rows) + 96


class Assignment(PairKernel):
    """The matching kernels bound to one env object: constants uploaded once, one launch per plane block, one per matching."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, agent, due, torch, device, api: str = 'assign_rbs') -> None:
        super().__init__(sim, num_links, torch, device, api=api, max_rbs=_native.ASSIGN_MAX_RBS, capacity=True)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever moved
        self.due = np.asarray(due, dtype=bool)                       # the DUE-pair links: movable=None
        if self.agent.shape != (self.n,) or self.due.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        self.own = {}                                # the tensors this object owns, by (name, shape)
        self._links = None                           # (key, host int32 [M], device int32 [M]) of the last movable mask

    def links(self, movable):
        """(host int32 [M], device int32 [M]): the movable links in ascending link index - the DUE-pair links (None), or the links
        `movable` (bool [N], array or tensor) marks, every one of which must have an action column.  A TENSOR is read on the host -
        the number of movable links shapes every output - which waits for everything queued before it on its stream; a host array
        is uploaded (a synchronous copy) when it differs from the last call's, and a repeat comes from the cache."""
        torch = self.torch
        if movable is None:
            host = self.due
        else:
            host = movable.cpu().numpy() if torch.is_tensor(movable) else np.asarray(movable)
            if host.shape != (self.n,) or host.dtype != np.bool_:
                raise ValueError(f'movable must be bool [{self.n}] (link) or None')
            if (host & ~self.agent).any():
                raise ValueError(f'movable marks link {int(np.nonzero(host & ~self.agent)[0][0])}, which has no action column '
                                 '(a link on fixed actions cannot be moved)')
        if not host.any():
            raise ValueError('movable marks no link')
        key = host.tobytes()
        if self._links is None or self._links[0] != key:
            idx = np.nonzero(host)[0].astype(np.int32)
            self._links = (key, idx, torch.as_tensor(idx, device=self.device))
        return self._links[1], self._links[2]

    def _owned(self, name: str, shape, dtype):
        key = (name, tuple(shape))
        if key not in self.own:
            self.own = {k: v for k, v in self.own.items() if k[0] != name}       # one block per name: a new shape replaces the old
            self.own[key] = self.torch.empty(shape, dtype=dtype, device=self.device)
        return self.own[key]

    def _check_out(self, out, names, shapes, dtypes):
        if not self.all_fit(out, shapes, dtypes):
            raise ValueError('out must be (' + ', '.join(names) + '): contiguous tensors ' +
                             ', '.join(f'{str(dt).replace("torch.", "")} {list(s)}' for s, dt in zip(shapes, dtypes)) +
                             f' on {self.device} that do not share memory')
        return tuple(out)

    def weights(self, t: dict, movable, allowed, objective: str, harm: bool, out, stream: int):
        """(weights [B, M, R], links int32 [M][, harm [B, M, R]]) of the env's current planes."""
        torch = self.torch
        if objective not in OBJECTIVES:
            raise ValueError(f"objective must be 'total' or 'own', got {objective!r}")
        _, links = self.links(movable)
        m = int(links.shape[0])
        need = lds_bytes(self.n, self.r, self.law != _native.ASSIGN_LAW_INV_SQUARE)
        if need > _native.ASSIGN_MAX_LDS_BYTES:
            raise ValueError(f'assignment_weights() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need '
                             f'{need} bytes, more than the {_native.ASSIGN_MAX_LDS_BYTES} a workgroup can have')
        shape = (self.b, m, self.r)
        names = ('weights', 'harm') if harm else ('weights',)
        if out is None:
            planes = tuple(self._owned(name, shape, torch.float32) for name in names)
        else:
            planes = self._check_out((out,) if torch.is_tensor(out) else out, names, (shape,) * len(names), (torch.float32,) * len(names))
        mask = self.words(allowed)                   # lives until the launch is enqueued; the stream orders its release behind it
        _native.assign_weights(*self.launch_args(t), links.data_ptr(), m, 0 if mask is None else mask.data_ptr(), OBJECTIVES[objective],
                               planes[0].data_ptr(), planes[1].data_ptr() if harm else 0, stream)
        return (planes[0], links, planes[1]) if harm else (planes[0], links)

    def solve(self, weights, out, stream: int):
        """(col int32 [B, M], value_mbps float32 [B], feasible uint8 [B]) of any float32 weights [B, M, R] on the device."""
        torch = self.torch
        if not (torch.is_tensor(weights) and weights.ndim == 3 and weights.dtype == torch.float32 and weights.is_contiguous()
                and weights.device == self.device and weights.shape[1] >= 1 and weights.shape[2] >= 1):
            raise ValueError(f'weights must be a contiguous float32 tensor [B, M, R] (env, row, column) on {self.device}')
        b, m, r = (int(x) for x in weights.shape)
        if m > r:
            raise ValueError(f'{m} rows cannot be matched one-to-one to {r} columns: M = {m} must be <= R = {r}')
        if r > _native.ASSIGN_MAX_RBS:
            raise ValueError(f'solve_assignment() serves at most {_native.ASSIGN_MAX_RBS} columns (R = {r})')
        need = solve_lds_bytes(m, r)
        if need > _native.ASSIGN_MAX_LDS_BYTES:
            raise ValueError(f'solve_assignment() keeps a matching in the LDS of one workgroup: {m} rows on {r} columns need {need} '
                             f'bytes, more than the {_native.ASSIGN_MAX_LDS_BYTES} a workgroup can have')
        shapes, dtypes = ((b, m), (b,), (b,)), (torch.int32, torch.float32, torch.uint8)
        names = ('col', 'value_mbps', 'feasible')
        if out is None:
            col, value, feasible = (self._owned(name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            col, value, feasible = self._check_out(out, names, shapes, dtypes)
        _native.assign_solve(weights.data_ptr(), b, m, r, col.data_ptr(), value.data_ptr(), feasible.data_ptr(), stream)
        return col, value, feasible

    def assign(self, t: dict, movable, allowed, objective: str, out, stream: int) -> AssignmentResult:
        """The two launches and the scatter of the matched columns into a copy of the rb plane."""
        torch = self.torch
        _, links = self.links(movable)
        m = int(links.shape[0])
        if m > self.r:
            raise ValueError(f'{m} movable links cannot have an RB each on {self.r} RBs: M = {m} must be <= R = {self.r}')
        shapes, dtypes = ((self.b, self.n), (self.b,), (self.b,)), (torch.int32, torch.float32, torch.uint8)
        names = ('rb', 'value_mbps', 'feasible')
        if out is None:
            rb, value, feasible = (self._owned('assigned_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            rb, value, feasible = self._check_out(out, names, shapes, dtypes)
        w = self.weights(t, movable, allowed, objective, False, None, stream)[0]
        col = self._owned('col', (self.b, m), torch.int32)
        self.solve(w, (col, value, feasible), stream)
        idx = links.long()
        rb.copy_(t['rb'])
        rb[:, idx] = torch.where(feasible[:, None] != 0, col, t['rb'][:, idx])
        return AssignmentResult(rb, value, feasible)

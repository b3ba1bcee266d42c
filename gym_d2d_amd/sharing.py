"""Exact optimal RB sharing for small link groups: the host side of libd2d_share.so (include/d2d_share.h, csrc/d2d_share.hip).

`Sharing` is bound to one env object as the other pair kernels are, and to that env's `assignment.Assignment`: the movable links,
the allowed words, the launch prefix, the owned tensors (`_owned`) and the out= refusal (`_check_out`, PairKernel.all_fit) are that
object's.  What is stated here: the shape refusals (M, the byte budget, the LDS), the value launch, the quota's forms, the solver
launch on ANY float64 [B, R, 2^M] tensor, and the scatter of the solved columns.  The solved RBs become step()'s action tensor
through best_response_dynamics.encode_actions.  Torch path only.  The refusal texts are `REFUSAL`, assign_rbs()'s row of
sensing.REFUSALS under the name share_rbs().
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .sensing import REFUSALS, r16, refusal_text

REFUSAL = ('share_rbs()', *REFUSALS['assign_rbs'][1:])          # assign_rbs()'s reasons under its own name


class SharingValues(NamedTuple):
    """What sharing_values() returns: a tuple with names."""
    values: object             # float64 [B, R, 2^M]: the total capacity of RB r with exactly the movable links of S beside its background
    links: object              # int32 [M]: the movable links in ascending link index; bit a of S is links[a]
    closed: object             # int32 [B]: the RBs with more than SHARE_MAX_BACKGROUND background members


class SharingSolution(NamedTuple):
    """What solve_sharing() returns: a tuple with names."""
    col: object                # int32 [B, M]: the RB of mask bit a; -1 in an infeasible env
    value: object              # float64 [B]: the optimum; 0.0 in an infeasible env
    feasible: object           # int32 [B]


class ShareRbsResult(NamedTuple):
    """What share_rbs() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the current RBs with the movable links on their optimal ones
    value_mbps: object         # float32 [B]: the env's total capacity under rb; 0.0 in an infeasible env
    feasible: object           # int32 [B]
    closed: object             # int32 [B]


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no share_rbs() (None: it has): assign_rbs()'s reasons, word for word, under this name."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def block_bytes(num_envs: int, num_rbs: int, num_movable: int) -> int:
    """The bytes of the value block (float64) and the solver's choice words (uint16) of one call, [B, R, 2^M] each."""
    return num_envs * num_rbs * (10 << num_movable)


def values_lds_bytes(num_links: int, num_movable: int, power_law: bool) -> int:
    """The LDS one workgroup of the value kernel needs (the header's formula): at most _native.SHARE_MAX_LDS_BYTES is served."""
    n, big = num_links, num_links + _native.SHARE_MAX_MOVABLE
    u = min(n, _native.SHARE_MAX_BACKGROUND) + num_movable
    return r16(8 * ((n + 63) // 64)) + r16(4 * u) + r16(4 * u * (u | 1)) + 32 * big + 2 * r16(4 * big) + r16(8 * big) \
        + (r16(8 * big) if power_law else 0)


def solve_lds_bytes(num_movable: int) -> int:
    """The LDS one workgroup of the solver needs (the header's formula): two layers, the staged values and the choice words."""
    return 26 << num_movable


def check_shape(num_envs: int, num_rbs: int, num_movable: int) -> None:
    """The shapes share_rbs() refuses by name, before anything is allocated or launched: M outside 1 .. SHARE_MAX_MOVABLE, and a
    value block whose bytes, with the choice words, exceed SHARE_MAX_BLOCK_BYTES."""
    if not 1 <= num_movable <= _native.SHARE_MAX_MOVABLE:
        raise ValueError(f'share_rbs() places 1 to {_native.SHARE_MAX_MOVABLE} movable links (D2D_SHARE_MAX_MOVABLE: two layers of 2^M '
                         f'doubles live in the LDS of one workgroup), got M = {num_movable}')
    need = block_bytes(num_envs, num_rbs, num_movable)
    if need > _native.SHARE_MAX_BLOCK_BYTES:
        raise ValueError(f'share_rbs() keeps a value block and choice words of {num_envs} x {num_rbs} x 2^{num_movable} entries: {need} '
                         f'bytes, more than the {_native.SHARE_MAX_BLOCK_BYTES} (D2D_SHARE_MAX_BLOCK_BYTES) one call may hold')


class Sharing:
    """The two kernels bound to one env object and its Assignment: one launch per value block, one per solution."""

    def __init__(self, sim, num_links: int, assign, torch, device) -> None:
        if assign.sim is not sim or assign.n != int(num_links):
            raise ValueError('the Assignment object does not match the env')
        self.assign, self.torch, self.device = assign, torch, device
        self._quota = None                           # (key, tensor) of the last host quota: a repeat is not uploaded again

    def _links(self, movable):
        """The movable links, refused by count: assignment's own refusals first (shape, a link without an action column, none)."""
        k = self.assign
        try:
            host, links = k.links(movable)
        except ValueError as why:
            if 'marks no link' in str(why):
                check_shape(k.b, k.r, 0)             # M = 0, refused under this name
            raise
        check_shape(k.b, k.r, int(host.shape[0]))
        return host, links

    def values(self, t: dict, movable, allowed, power_dbm, out, stream: int) -> SharingValues:
        """The value launch and the sum of the closed flags."""
        torch, k = self.torch, self.assign
        _, links = self._links(movable)
        m = int(links.shape[0])
        need = values_lds_bytes(k.n, m, k.law != _native.SHARE_LAW_INV_SQUARE)
        if need > _native.SHARE_MAX_LDS_BYTES:
            raise ValueError(f'sharing_values() keeps an RB in the LDS of one workgroup: {k.n} links with {m} movable need {need} '
                             f'bytes, more than the {_native.SHARE_MAX_LDS_BYTES} (D2D_SHARE_MAX_LDS_BYTES) a workgroup can have')
        if power_dbm is None:
            pwr = t['pwr']
        elif not k.fits(power_dbm, (k.b, k.n), torch.int32):
            raise ValueError(f'power_dbm must be a contiguous int32 tensor [{k.b}, {k.n}] on {self.device} or None')
        else:
            pwr = power_dbm
        shape = (k.b, k.r, 1 << m)
        if out is None:
            values = k._owned('share_values', shape, torch.float64)
        else:
            values, = k._check_out((out,) if torch.is_tensor(out) else out, ('values',), (shape,), (torch.float64,))
        flags = k._owned('share_closed_rb', (k.b, k.r), torch.int32)
        closed = k._owned('share_closed', (k.b,), torch.int32)
        mask = k.words(allowed)                      # lives until the launch is enqueued; the stream orders its release behind it
        _native.share_values(*k.raw_launch_args(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), t['rb'].data_ptr(), pwr.data_ptr()),
                             links.data_ptr(), m, 0 if mask is None else mask.data_ptr(), values.data_ptr(), flags.data_ptr(), stream)
        torch.sum(flags, dim=1, dtype=torch.int32, out=closed)
        return SharingValues(values, links, closed)

    def quota(self, quota, num_movable: int, num_rbs: int):
        """None (no limit), or int32 [R] on the device: a plain int for every RB, [R] ints (list, tuple or array) each >= 0, or an
        int32 [R] tensor on the env's device, whose values are the caller's promise (the kernel reads a negative one as 0)."""
        torch = self.torch
        if quota is None:
            return None
        if torch.is_tensor(quota):
            if not self.assign.fits(quota, (num_rbs,), torch.int32):
                raise ValueError(f'quota as a tensor must be contiguous int32 [{num_rbs}] (RB) on {self.device}')
            return quota
        if isinstance(quota, (bool, np.bool_)) or (isinstance(quota, np.ndarray) and quota.dtype == np.bool_):
            host = None
        elif isinstance(quota, (int, np.integer)):
            host = np.full(num_rbs, int(quota), dtype=np.int64)
        else:
            try:
                host = np.asarray(quota)
            except (TypeError, ValueError):
                host = None
            if host is not None and (host.shape != (num_rbs,) or host.dtype.kind not in 'iu'):
                host = None
        if host is None or (host < 0).any():
            raise ValueError(f'quota must be None, an int or [{num_rbs}] ints (RB), each >= 0 (0: the RB is closed to movable links)')
        host = np.minimum(host, num_movable).astype(np.int32)           # a quota above M never binds
        key = host.tobytes()
        if self._quota is None or self._quota[0] != key:
            self._quota = (key, torch.as_tensor(host, device=self.device))
        return self._quota[1]

    def _block(self, values):
        torch = self.torch
        if not (torch.is_tensor(values) and values.ndim == 3 and values.dtype == torch.float64 and values.is_contiguous()
                and values.device == self.device and values.shape[1] >= 1):
            raise ValueError(f'values must be a contiguous float64 tensor [B, R, 2^M] (env, RB, subset) on {self.device}')
        b, r, subsets = (int(x) for x in values.shape)
        m = subsets.bit_length() - 1
        if subsets < 2 or subsets != 1 << m or m > _native.SHARE_MAX_MOVABLE:
            raise ValueError(f'solve_sharing() takes 2^M subsets with M in 1 .. {_native.SHARE_MAX_MOVABLE} (D2D_SHARE_MAX_MOVABLE), that '
                             f'is a last dimension that is a power of two in 2 .. {1 << _native.SHARE_MAX_MOVABLE}; got {subsets}')
        if r > _native.SHARE_MAX_RBS:
            raise ValueError(f'solve_sharing() serves at most {_native.SHARE_MAX_RBS} RBs (R = {r})')
        need = block_bytes(b, r, m)
        if need > _native.SHARE_MAX_BLOCK_BYTES:
            raise ValueError(f'solve_sharing() keeps choice words beside the {b} x {r} x 2^{m} values: {need} bytes together, more '
                             f'than the {_native.SHARE_MAX_BLOCK_BYTES} (D2D_SHARE_MAX_BLOCK_BYTES) one call may hold')
        need = solve_lds_bytes(m)
        if need > _native.SHARE_MAX_LDS_BYTES:
            raise ValueError(f'solve_sharing() keeps two layers in the LDS of one workgroup: M = {m} needs {need} bytes, more than the '
                             f'{_native.SHARE_MAX_LDS_BYTES} (D2D_SHARE_MAX_LDS_BYTES) a workgroup can have')
        return b, r, m

    def solve(self, values, quota, out, stream: int) -> SharingSolution:
        """The optimal placement under any float64 [B, R, 2^M] tensor on the device."""
        torch, k = self.torch, self.assign
        b, r, m = self._block(values)
        q = self.quota(quota, m, r)
        shapes, dtypes = ((b, m), (b,), (b,)), (torch.int32, torch.float64, torch.int32)
        names = SharingSolution._fields
        if out is None:
            res = tuple(k._owned('share_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            res = k._check_out(out, names, shapes, dtypes)
        choice = k._owned('share_choice', (b, r, 1 << m), torch.int16)           # the 16-bit words of the kernel
        _native.share_solve(values.data_ptr(), 0 if q is None else q.data_ptr(), b, r, m, choice.data_ptr(),
                            *(o.data_ptr() for o in res), stream)
        return SharingSolution(*res)

    def rbs(self, t: dict, movable, allowed, quota, power_dbm, out, stream: int) -> ShareRbsResult:
        """The two launches and the scatter of the solved columns into a copy of the rb plane."""
        torch, k = self.torch, self.assign
        _, links = self._links(movable)
        m = int(links.shape[0])
        q = self.quota(quota, m, k.r)                # refused before anything is launched
        shapes, dtypes = ((k.b, k.n), (k.b,), (k.b,), (k.b,)), (torch.int32, torch.float32, torch.int32, torch.int32)
        names = ShareRbsResult._fields
        if out is None:
            rb, value, feasible, closed = (k._owned('share_rbs_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            rb, value, feasible, closed = k._check_out(out, names, shapes, dtypes)
        block = self.values(t, movable, allowed, power_dbm, None, stream)
        col = k._owned('share_rbs_col', (k.b, m), torch.int32)
        best = k._owned('share_rbs_value', (k.b,), torch.float64)
        self.solve(block.values, q, (col, best, feasible), stream)
        value.copy_(best)                            # float32 of the double optimum
        closed.copy_(block.closed)
        idx = links.long()
        rb.copy_(t['rb'])
        rb[:, idx] = torch.where(feasible[:, None] != 0, col, t['rb'][:, idx])
        return ShareRbsResult(rb, value, feasible, closed)

    def close(self) -> None:
        """Nothing of its own to free: every tensor is the Assignment object's."""

"""Stable RB matching with quotas: the host side of libd2d_stable.so (include/d2d_stable.h, csrc/d2d_stable.hip).

`StableMatching` is bound to one env object as the other pair kernels are, and to that env's `assignment.Assignment`: the
preferences of stable_rbs() are the planes of assignment_weights(objective='own', harm=True), bit for bit, so the movable links, the
allowed words, the weights launch, the owned tensors (`_owned`) and the out= refusal (`_check_out`, PairKernel.all_fit) are that
object's and nothing is uploaded twice.  What is stated here: the quota's forms, the LDS formula, the matching launch on ANY pair
of preference tensors, and the scatter of the matched columns.  The matched RBs become step()'s action tensor through
best_response_dynamics.encode_actions.  Torch path only.  The refusal texts are `REFUSAL`, assign_rbs()'s row of sensing.REFUSALS
under the name stable_rbs().
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .sensing import REFUSALS, r16, refusal_text

REFUSAL = ('stable_rbs()', *REFUSALS['assign_rbs'][1:])         # assign_rbs()'s reasons under its own name
RB_PREFS = ('harm', 'total')


class StableMatchingResult(NamedTuple):
    """What solve_stable_matching() returns: a tuple with names."""
    col: object                # int32 [B, M]: the RB of row a; -1: unmatched
    load: object               # int32 [B, R]: the rows matched to r; load <= quota
    proposals: object          # int32 [B]: the proposals deferred acceptance makes, in any order
    unmatched: object          # int32 [B]: the rows with col -1


class StableRbsResult(NamedTuple):
    """What stable_rbs() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the current RBs with the matched movable links on their RB
    unmatched: object          # int32 [B]: the movable links left without one; they keep their current RB
    proposals: object          # int32 [B]


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no stable_rbs() (None: it has): assign_rbs()'s reasons, word for word, under this name."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def lds_bytes(num_rows: int, num_rbs: int) -> int:
    """The LDS one workgroup of the kernel needs (the header's formula): at most _native.STABLE_MAX_LDS_BYTES is served."""
    return 2 * r16(8 * num_rows) + 4 * r16(4 * num_rows) + 4 * r16(4 * num_rbs) + 16


class StableMatching:
    """The matching kernel bound to one env object and its Assignment: one launch per matching."""

    def __init__(self, sim, num_links: int, assign, torch, device) -> None:
        if assign.sim is not sim or assign.n != int(num_links):
            raise ValueError('the Assignment object does not match the env')
        self.assign, self.torch, self.device = assign, torch, device
        self._quota = None                           # (key, tensor) of the last host quota: a repeat is not uploaded again

    def quota(self, quota, num_rows: int, num_rbs: int):
        """int32 [R] on the device: a plain int for every RB, [R] ints (list, tuple or array) each in [0, M], or an int32 [R] tensor
        on the env's device, whose values are the caller's promise (the kernel reads a negative one as 0)."""
        torch = self.torch
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
        if host is None or (host < 0).any() or (host > num_rows).any():
            raise ValueError(f'quota must be an int or [{num_rbs}] ints (RB), each in [0, {num_rows}] (0: the RB is closed)')
        key = (num_rows, host.astype(np.int32).tobytes())
        if self._quota is None or self._quota[0] != key:
            self._quota = (key, torch.as_tensor(host.astype(np.int32), device=self.device))
        return self._quota[1]

    def _prefs(self, link_pref, rb_pref):
        torch = self.torch
        ok = lambda t: torch.is_tensor(t) and t.ndim == 3 and t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device
        if not (ok(link_pref) and ok(rb_pref) and link_pref.shape == rb_pref.shape and link_pref.shape[1] >= 1
                and link_pref.shape[2] >= 1):
            raise ValueError('link_pref and rb_pref must be contiguous float32 tensors of one shape [B, M, R] (env, link, RB) on '
                             f'{self.device}')
        b, m, r = (int(x) for x in link_pref.shape)
        if m > _native.STABLE_MAX_LINKS or r > _native.STABLE_MAX_RBS:
            raise ValueError(f'solve_stable_matching() serves at most {_native.STABLE_MAX_LINKS} rows and {_native.STABLE_MAX_RBS} '
                             f'columns (M = {m}, R = {r})')
        need = lds_bytes(m, r)
        if need > _native.STABLE_MAX_LDS_BYTES:
            raise ValueError(f'solve_stable_matching() keeps a matching in the LDS of one workgroup: {m} rows on {r} columns need '
                             f'{need} bytes, more than the {_native.STABLE_MAX_LDS_BYTES} (D2D_STABLE_MAX_LDS_BYTES) a workgroup '
                             'can have')
        return b, m, r

    def solve(self, link_pref, rb_pref, quota, out, stream: int) -> StableMatchingResult:
        """The link-optimal stable matching of any pair of float32 [B, M, R] tensors on the device."""
        torch = self.torch
        b, m, r = self._prefs(link_pref, rb_pref)
        q = self.quota(quota, m, r)
        shapes, dtypes = ((b, m), (b, r), (b,), (b,)), (torch.int32,) * 4
        names = StableMatchingResult._fields
        if out is None:
            res = tuple(self.assign._owned('stable_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            res = self.assign._check_out(out, names, shapes, dtypes)
        _native.stable_match(link_pref.data_ptr(), rb_pref.data_ptr(), q.data_ptr(), b, m, r, *(o.data_ptr() for o in res), stream)
        return StableMatchingResult(*res)

    def rbs(self, t: dict, movable, allowed, quota, rb_pref: str, out, stream: int) -> StableRbsResult:
        """The weights launch, the RBs' preferences by one torch op, the matching launch and the scatter of the matched columns
        into a copy of the rb plane."""
        torch, k = self.torch, self.assign
        if rb_pref not in RB_PREFS:
            raise ValueError(f"rb_pref must be 'harm' or 'total', got {rb_pref!r}")
        _, links = k.links(movable)
        m = int(links.shape[0])
        q = self.quota(quota, m, k.r)                # refused before anything is launched
        shapes, dtypes = ((k.b, k.n), (k.b,), (k.b,)), (torch.int32,) * 3
        names = StableRbsResult._fields
        if out is None:
            rb, unmatched, proposals = (k._owned('stable_rbs_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            rb, unmatched, proposals = k._check_out(out, names, shapes, dtypes)
        own, _, harm = k.weights(t, movable, allowed, 'own', True, None, stream)
        pref = k._owned('stable_rbs_pref', tuple(own.shape), torch.float32)
        if rb_pref == 'harm':
            torch.neg(harm, out=pref)                # the RB prefers whoever hurts its background least
        else:
            torch.sub(own, harm, out=pref)           # assignment_weights(objective='total'), formed in float32
        col = k._owned('stable_rbs_col', (k.b, m), torch.int32)
        load = k._owned('stable_rbs_load', (k.b, k.r), torch.int32)
        self.solve(own, pref, q, (col, load, proposals, unmatched), stream)
        idx = links.long()
        rb.copy_(t['rb'])
        rb[:, idx] = torch.where(col >= 0, col, t['rb'][:, idx])
        return StableRbsResult(rb, unmatched, proposals)

    def close(self) -> None:
        """Nothing of its own to free: every tensor is the Assignment object's."""

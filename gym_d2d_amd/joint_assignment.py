"""Joint RB and power matching with SINR floors: the host side of libd2d_assignpwr.so (include/d2d_assignpwr.h,
csrc/d2d_assignpwr.hip).

`JointAssignment` is assignment.Assignment - the same movable links, allowed words, owned tensors and matching launch - with the
power alphabet of every link's class (power_control.class_bounds) and the launch that scans it: every movable link's best admissible
power on every RB and the weight it has there.  The floors take the three forms power_control() takes its targets in.  The matched
RBs and powers become step()'s action tensor through power_control.encode_actions.  Torch path only.  The refusal texts are the
'assign_rbs_power' row of sensing.REFUSALS, assign_rbs()'s under this name; `lds_bytes` is assignment's.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import _native, assignment
from .power_control import link_values
from .sensing import refusal_text


class JointAssignmentResult(NamedTuple):
    """What assign_rbs_power() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the current RBs with the movable links on their matched ones
    power_dbm: object          # int32 [B, N]: the current powers with the movable links at their matched entry's power
    value_mbps: object         # float32 [B]: the sum of the matched weights; 0.0 where infeasible
    feasible: object           # uint8 [B]: 1 - every movable link has an RB of its own and an admissible power there


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no assign_rbs_power() (None: it has): assign_rbs()'s reasons, word for word, under this name."""
    return refusal_text('assign_rbs_power', sim, export_actions, use_torch)


# the LDS one workgroup of the kernel needs is d2d_assign_weights's formula (the floors ride in words that kernel has too): at most
# _native.ASSIGNPWR_MAX_LDS_BYTES is served
lds_bytes = assignment.lds_bytes


def check_alphabet(p_min, p_max, links=None) -> None:
    """ValueError, by name, for power bounds the kernel does not scan: p_min > p_max, |p| >= 4096, and - for the links `links` lists
    (None: every link) - more than _native.ASSIGNPWR_MAX_LEVELS levels.  The bounds live on the device for the kernel, which cannot
    refuse by name; this is where they are still host arrays."""
    p_min, p_max = np.asarray(p_min, dtype=np.int64), np.asarray(p_max, dtype=np.int64)
    if p_min.shape != p_max.shape or p_min.ndim != 1:
        raise ValueError('p_min and p_max must be int [N] arrays of one length')
    who = np.arange(len(p_min)) if links is None else np.asarray(links, dtype=np.int64)
    who = who[(who >= 0) & (who < len(p_min))]
    lo, hi = p_min[who], p_max[who]
    if (lo > hi).any():
        j = int(who[np.nonzero(lo > hi)[0][0]])
        raise ValueError(f'p_min > p_max for link {j} ({int(p_min[j])} > {int(p_max[j])}): p_min must be <= p_max')
    if len(who) and max(np.abs(lo).max(), np.abs(hi).max()) >= 4096:
        raise ValueError('the power bounds must be whole dBm with |p| < 4096')
    if (hi - lo + 1 > _native.ASSIGNPWR_MAX_LEVELS).any():
        j = int(who[np.nonzero(hi - lo + 1 > _native.ASSIGNPWR_MAX_LEVELS)[0][0]])
        raise ValueError(f'link {j} has {int(p_max[j] - p_min[j] + 1)} power levels, more than the {_native.ASSIGNPWR_MAX_LEVELS} '
                         'assign_rbs_power() scans per movable link (D2D_ASSIGNPWR_MAX_LEVELS)')


class JointAssignment(assignment.Assignment):
    """The joint kernel bound to one env object: constants and bounds uploaded once, one launch per plane pair, the matching
    through the launch assign_rbs() uses."""

    def __init__(self, sim, num_links: int, agent, due, p_min, p_max, torch, device) -> None:
        super().__init__(sim, num_links, agent, due, torch, device, api='assign_rbs_power')
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        if not (p_min.shape == p_max.shape == (self.n,)):
            raise ValueError('the power bounds do not match the env')
        check_alphabet(p_min, p_max, np.nonzero(self.agent)[0])          # the links that can ever be movable
        self.p_min_host, self.p_max_host = p_min, p_max
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        self._target = None                          # (key, tensor) of the last floors: a repeat is not uploaded again

    def floors(self, min_sinr_db, num_cues: int):
        """None (no floors), or float32 [N] on the device from a number, {'cue': x, 'due': y} or [N] values (array or tensor), dB;
        -inf: no floor for that link."""
        return None if min_sinr_db is None else link_values(self, min_sinr_db, num_cues, 'min_sinr_db')

    def power_weights(self, t: dict, movable, allowed, floors, out, stream: int):
        """(weights float32 [B, M, R], power_dbm int32 [B, M, R], links int32 [M]) of the env's current planes; floors: what
        floors() returns."""
        torch = self.torch
        _, links = self.links(movable)
        m = int(links.shape[0])
        need = lds_bytes(self.n, self.r, self.law != _native.ASSIGNPWR_LAW_INV_SQUARE)
        if need > _native.ASSIGNPWR_MAX_LDS_BYTES:
            raise ValueError(f'joint_assignment_weights() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs '
                             f'need {need} bytes, more than the {_native.ASSIGNPWR_MAX_LDS_BYTES} a workgroup can have')
        shape = (self.b, m, self.r)
        names, dtypes = ('weights', 'power_dbm'), (torch.float32, torch.int32)
        if out is None:
            w, pw = (self._owned('joint_' + name, shape, dt) for name, dt in zip(names, dtypes))
        else:
            w, pw = self._check_out(out, names, (shape, shape), dtypes)
        mask = self.words(allowed)                   # lives until the launch is enqueued; the stream orders its release behind it
        _native.assign_power_weights(*self.launch_args(t), links.data_ptr(), m, 0 if mask is None else mask.data_ptr(),
                                     self.p_min.data_ptr(), self.p_max.data_ptr(), 0 if floors is None else floors.data_ptr(),
                                     w.data_ptr(), pw.data_ptr(), stream)
        return w, pw, links

    def assign_power(self, t: dict, movable, allowed, floors, out, stream: int) -> JointAssignmentResult:
        """The joint launch, the matching launch, the gather of every matched entry's power and the two scatters."""
        torch = self.torch
        _, links = self.links(movable)
        m = int(links.shape[0])
        if m > self.r:
            raise ValueError(f'{m} movable links cannot have an RB each on {self.r} RBs: M = {m} must be <= R = {self.r}')
        shapes = ((self.b, self.n), (self.b, self.n), (self.b,), (self.b,))
        dtypes = (torch.int32, torch.int32, torch.float32, torch.uint8)
        names = ('rb', 'power_dbm', 'value_mbps', 'feasible')
        if out is None:
            rb, power, value, feasible = (self._owned('joint_assigned_' + name, s, dt) for name, s, dt in zip(names, shapes, dtypes))
        else:
            rb, power, value, feasible = self._check_out(out, names, shapes, dtypes)
        w, pw, _ = self.power_weights(t, movable, allowed, floors, None, stream)
        col = self._owned('col', (self.b, m), torch.int32)
        self.solve(w, (col, value, feasible), stream)
        idx = links.long()
        ok = feasible[:, None] != 0
        matched = pw.gather(2, col.clamp(min=0).long().unsqueeze(2)).squeeze(2)      # an infeasible env's col is -1: not used
        rb.copy_(t['rb'])
        rb[:, idx] = torch.where(ok, col, t['rb'][:, idx])
        power.copy_(t['pwr'])
        power[:, idx] = torch.where(ok, matched, t['pwr'][:, idx])
        return JointAssignmentResult(rb, power, value, feasible)

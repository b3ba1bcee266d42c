"""Unilateral-deviation gains over every (RB, power) action: the host side of libd2d_deviate.so (include/d2d_deviate.h,
csrc/d2d_deviate.hip).

`Deviation` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns and
sensing.fold_capacity_columns fold, unchanged, the power bounds of every link's class) and launches the two entry points on torch's
device pointers: the table of d2d_deviation_gains, or the reduction of d2d_best_deviation, one call each.  `lds_bytes` and
`table_bytes` restate the header's formulas.  The allowed mask goes through best_response.words / pack_allowed, the floor is
power_control.link_values, the action encoding is power_control.encode_actions.  Torch path only.  The refusal texts are `REFUSAL`,
a row of the form of sensing.REFUSALS kept here; the out= checks, the owned outputs and the launch prefix are PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .power_control import link_values
from .sensing import PairKernel, r16, refusal_text

REFUSAL = ('deviation_gains()', 'reads the decoded (rb, tx power) planes, which export_actions=False does not write',
           'its kernel can evaluate for the actions no step has applied',
           'counterfactual (what another action would have given is another draw)', 'table and planes')


class BestDeviationResult(NamedTuple):
    """What best_deviation() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: every selected link's best RB, or the held one
    power_dbm: object          # int32 [B, N]: likewise, its power
    gain_mbps: object          # float64 [B, N]: what the total gains if that link alone moves there; 0.0 where it stays
    regret_mbps: object        # float64 [B]: the largest gain_mbps of the env
    leader: object             # int32 [B]: the lowest link that has it; -1: nobody would move


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no deviation_gains() (None: it has): the predicate of sensing.unserved under texts of its own - refused
    where rb_ascent() is."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def lds_bytes(n: int, r: int, allowed: bool = False) -> int:
    """The LDS one workgroup of d2d_deviation_gains / d2d_best_deviation needs: the formula of include/d2d_deviate.h."""
    return 80 * n + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 5216


def table_bytes(b: int, m: int, r: int, levels: int) -> int:
    """The bytes of the float32 table [B, M, R, Lmax]."""
    return 4 * b * m * r * levels


class Deviation(PairKernel):
    """The deviation kernels bound to one env object: constants uploaded once, one call of the library per method call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, p_min, p_max, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='deviation_gains', max_rbs=_native.DEVIATE_MAX_RBS, capacity=True)
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever selected
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        if not (p_min.shape == p_max.shape == (self.n,)) or (p_min > p_max).any() or max(np.abs(p_max).max(), np.abs(p_min).max()) >= 4096:
            raise ValueError('the power bounds do not match the env')
        self.levels = (p_max.astype(np.int64) - p_min + 1)           # L_i of every link
        most = int(self.levels[self.agent].max()) if self.agent.any() else 1
        if most > _native.DEVIATE_MAX_LEVELS:
            raise ValueError(f'deviation_gains() serves at most {_native.DEVIATE_MAX_LEVELS} power levels per link '
                             f'(D2D_DEVIATE_MAX_LEVELS), got {most}')
        self.need(False)                                             # a shape no call could serve is refused when the object is made
        self.declare_outputs(BestDeviationResult._fields, ((self.b, self.n),) * 3 + ((self.b,),) * 2,
                             (torch.int32, torch.int32, torch.float64, torch.float64, torch.int32))
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        self._target = None                          # (key, tensor) of the last host floor: a repeat is not uploaded again
        self._links = None                           # (key, links tensor, levels tensor, Lmax) of the last selection
        self._table = None                           # the table this object owns, of the last shape asked for

    def need(self, allowed: bool) -> int:
        """lds_bytes of this env, with or without an allowed mask; ValueError past the limit, stating the byte count."""
        need = lds_bytes(self.n, self.r, allowed)
        if need > _native.DEVIATE_MAX_LDS_BYTES:
            raise ValueError(f'deviation_gains() keeps an env in the LDS of every workgroup: {self.n} links on {self.r} RBs need {need} '
                             f'bytes{" with an allowed mask" if allowed else ""}, more than {_native.DEVIATE_MAX_LDS_BYTES}')
        return need

    def floor(self, floor_sinr_db, num_cues: int):
        """float32 [N] on the device from None (no floors: -inf), a scalar, {'cue': x, 'due': y} or [N] values (array or tensor);
        -inf: that link has no floor."""
        return link_values(self, -np.inf if floor_sinr_db is None else floor_sinr_db, num_cues, 'floor_sinr_db')

    def select(self, links):
        """(links int32 [M] on the device, levels int32 [M] on the device, Lmax) of `links`: None (the agent links), or host ints
        (a list or an array), ascending and distinct, agent links all.  A repeat of the last selection is not uploaded again."""
        torch = self.torch
        what = f'links must be None or ascending, distinct ints in [0, {self.n}) (a list or an array), at least one'
        if links is None:
            host = np.nonzero(self.agent)[0]
        else:
            if torch.is_tensor(links) or isinstance(links, (bool, str)):
                raise ValueError(what + ('; a tensor would have to be read on the host' if torch.is_tensor(links) else ''))
            host = np.asarray(links)
            if host.ndim != 1 or host.dtype.kind not in 'iu':
                raise ValueError(what)
        host = host.astype(np.int64)
        if host.size == 0 or host.min() < 0 or host.max() >= self.n or (np.diff(host) <= 0).any():
            raise ValueError(what)
        if not self.agent[host].all():
            fixed = [int(i) for i in host[~self.agent[host]]]
            raise ValueError(f"links on fixed actions (cue_actions='traffic') have no action to deviate to and may not be selected: {fixed}")
        key = host.tobytes()
        if self._links is None or self._links[0] != key:
            lv = self.levels[host]
            self._links = (key, torch.as_tensor(host.astype(np.int32), device=self.device),
                           torch.as_tensor(lv.astype(np.int32), device=self.device), int(lv.max()))
        return self._links[1:]

    def gains(self, t: dict, links, allowed, floor, out, stream: int, env_mask=None):
        """floor: the tensor floor() returns; links, allowed: what the caller passed.  Returns (gain_mbps float32 [B, M, R, Lmax],
        links int32 [M], levels int32 [M])."""
        torch = self.torch
        sel, levels, lmax = self.select(links)
        m = int(sel.shape[0])
        shape = (self.b, m, self.r, lmax)
        nbytes = table_bytes(*shape)
        if nbytes > _native.DEVIATE_MAX_TABLE_BYTES:
            raise ValueError(f'deviation_gains() would write a table of {nbytes} bytes (float32 {list(shape)}), more than '
                             f'{_native.DEVIATE_MAX_TABLE_BYTES}: select fewer links, or take best_deviation(), which writes none')
        self.need(allowed is not None)
        if out is None:
            if self._table is None or tuple(self._table.shape) != shape:
                self._table = torch.empty(shape, dtype=torch.float32, device=self.device)
            out = self._table
        elif not self.fits(out, shape, torch.float32):
            raise ValueError(f'out must be a contiguous float32 {list(shape)} tensor on {self.device}')
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        mask = self.env_mask(env_mask)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        _native.deviation_gains(*self.launch_args(t), self.p_min.data_ptr(), self.p_max.data_ptr(), sel.data_ptr(), m, lmax, ptr(words),
                                floor.data_ptr(), ptr(mask), out.data_ptr(), stream)
        return out, sel, levels

    def best(self, t: dict, links, allowed, floor, min_gain_mbps: float, out, stream: int, env_mask=None) -> BestDeviationResult:
        """floor: the tensor floor() returns; links, allowed: what the caller passed."""
        if isinstance(min_gain_mbps, bool) or not isinstance(min_gain_mbps, (int, float, np.integer, np.floating)) \
                or not math.isfinite(min_gain_mbps) or min_gain_mbps < 0:
            raise ValueError(f'min_gain_mbps must be a finite number >= 0, got {min_gain_mbps!r}')
        sel, _, lmax = self.select(links)
        self.need(allowed is not None)
        res = self.outputs(out)
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        mask = self.env_mask(env_mask)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        _native.best_deviation(*self.launch_args(t), self.p_min.data_ptr(), self.p_max.data_ptr(), sel.data_ptr(), int(sel.shape[0]), lmax,
                               ptr(words), floor.data_ptr(), float(min_gain_mbps), ptr(mask), *(o.data_ptr() for o in res), stream)
        return BestDeviationResult(*res)

"""Max-min SINR balancing with protected links: the host side of libd2d_balance.so (include/d2d_balance.h, csrc/d2d_balance.hip).

`SinrBalance` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns folds, unchanged, the
power bounds of every link's class) and launches the search on torch's device pointers: one launch per call, every probe of every
env inside it.  `margin_grid` validates the grid of levels, `lds_bytes` restates the header's formula.  The base and the floor are
power_control.link_values, the action encoding is power_control.encode_actions.  Torch path only.  The refusal texts are the
'balance_sinr' row of sensing.REFUSALS; the out= check, the owned outputs and the launch prefix are PairKernel's.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .power_control import link_values
from .sensing import PairKernel, r16, refusal_text

DEFAULT_MARGINS_DB = np.arange(-20.0, 41.0, dtype=np.float32)        # -20, -19, ..., 40


class SinrBalanceResult(NamedTuple):
    """What balance_sinr() returns: a tuple with names."""
    power_dbm: object          # int32 [B, N]: the least powers that give the balanced level (probe 0's where infeasible)
    sinr_db: object            # float32 [B, N]: every link's SINR at those powers
    margin_db: object          # float32 [B]: margins_db[level]; -inf where infeasible
    level: object              # int32 [B]: the largest level of the grid the search found to pass; -1 where level 0 fails
    probes: object             # int32 [B]: the power-control solves the search ran


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no balance_sinr() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('balance_sinr', sim, export_actions, use_torch)


def lds_bytes(n: int, r: int, law: int) -> int:
    """The LDS one workgroup of d2d_balance_sinr needs: the formula of include/d2d_balance.h."""
    n4 = (n + 3) & ~3
    return 32 * n + (2 + (law != _native.BALANCE_LAW_INV_SQUARE)) * r16(8 * n) + 28 * n4 + r16(4 * (r + 1)) + 64


def margin_grid(margins_db) -> np.ndarray:
    """float32 [K] from host values: 1-D, finite, strictly ascending as float32, 1 <= K <= BALANCE_MAX_MARGINS; else ValueError."""
    try:
        m = np.asarray(margins_db, dtype=np.float32)
    except (TypeError, ValueError):
        m = np.empty((0, 0), dtype=np.float32)
    if m.ndim != 1 or not 1 <= m.shape[0] <= _native.BALANCE_MAX_MARGINS or not np.isfinite(m).all() or not (np.diff(m) > 0).all():
        raise ValueError(f'margins_db must be 1 to {_native.BALANCE_MAX_MARGINS} finite values in strictly ascending order (float32), '
                         'or a float32 tensor of them on the device')
    return np.ascontiguousarray(m)


class SinrBalance(PairKernel):
    """The balancing kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, p_min, p_max, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='balance_sinr', max_rbs=_native.BALANCE_MAX_RBS)
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever adjusted
        if not (p_min.shape == p_max.shape == self.agent.shape == (self.n,)) or (p_min > p_max).any() or np.abs(p_max).max() >= 4096:
            raise ValueError('the power bounds do not match the env')
        need = lds_bytes(self.n, self.r, self.law)
        if need > _native.BALANCE_MAX_LDS_BYTES:
            raise ValueError(f'balance_sinr() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} bytes, '
                             f'more than {_native.BALANCE_MAX_LDS_BYTES}')
        self.declare_outputs(SinrBalanceResult._fields, ((self.b, self.n), (self.b, self.n), (self.b,), (self.b,), (self.b,)),
                             (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32))
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        # link_values keeps the last host value of ONE argument in `_target`: the base and the floor each get a holder of their own
        self._base, self._floor = (SimpleNamespace(torch=torch, device=device, n=self.n, _target=None) for _ in range(2))
        self._margins = None                         # (key, tensor) of the last host grid: a repeated grid is not uploaded again

    def base(self, base_sinr_db, num_cues: int):
        """float32 [N] on the device from a scalar, {'cue': x, 'due': y} or [N] values (array or tensor)."""
        return link_values(self._base, base_sinr_db, num_cues, 'base_sinr_db')

    def floor(self, floor_sinr_db, num_cues: int):
        """None (no floors), or float32 [N] on the device as base() makes it; -inf: that link has no floor."""
        return None if floor_sinr_db is None else link_values(self._floor, floor_sinr_db, num_cues, 'floor_sinr_db')

    def margins(self, margins_db):
        """float32 [K] on the device: the default grid (None), a host array checked by margin_grid(), or a device tensor whose
        dtype, shape and device are checked and whose order is the caller's promise (reading it would synchronise)."""
        torch = self.torch
        if torch.is_tensor(margins_db):
            if margins_db.dtype != torch.float32 or margins_db.dim() != 1 or margins_db.device != self.device \
                    or not 1 <= margins_db.shape[0] <= _native.BALANCE_MAX_MARGINS:
                raise ValueError(f'margins_db as a tensor must be float32 [K], 1 <= K <= {_native.BALANCE_MAX_MARGINS}, on {self.device}')
            return margins_db.contiguous()
        host = DEFAULT_MARGINS_DB if margins_db is None else margin_grid(margins_db)
        key = host.tobytes()
        if self._margins is None or self._margins[0] != key:
            self._margins = (key, torch.as_tensor(host, device=self.device))
        return self._margins[1]

    def adjustable(self, adjustable):
        """uint8 [N] on the device: the agent links (None), or those of them `adjustable` (bool [N], array or tensor) marks."""
        return self.agent_subset(adjustable, 'adjustable')

    def solve(self, t: dict, base, margins, floor, adjustable, max_iters: int, out, stream: int, env_mask=None) -> SinrBalanceResult:
        """base, margins, floor, adjustable: the tensors base(), margins(), floor() and adjustable() return."""
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 1:
            raise ValueError(f'max_iters must be an int >= 1, got {max_iters!r}')
        power, sinr, margin, level, probes = self.outputs(out)
        mask = self.env_mask(env_mask)               # lives until the launch is enqueued; the stream orders its release behind it
        _native.balance_sinr(*self.launch_args(t), base.data_ptr(), 0 if floor is None else floor.data_ptr(), margins.data_ptr(),
                             int(margins.shape[0]), self.p_min.data_ptr(), self.p_max.data_ptr(), adjustable.data_ptr(), int(max_iters),
                             0 if mask is None else mask.data_ptr(), power.data_ptr(), sinr.data_ptr(), margin.data_ptr(),
                             level.data_ptr(), probes.data_ptr(), stream)
        return SinrBalanceResult(power, sinr, margin, level, probes)

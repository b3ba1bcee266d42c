"""What-if evaluation of candidate joint actions on a path-loss table: the host side of libd2d_evaltab.so (include/d2d_evaltab.h,
csrc/d2d_evaltab.hip).

evaluate.Evaluate serves the native power-law models: its kernel evaluates a law at the positions.  `TableEvaluate` serves the envs
whose step reads a dB table by (tx link, rx link) - the 'channel' route, the 'per_step' route, 'array' with an SNR row - and, through
table=, any env at all: it hands the kernel the table as it stands in device memory, with the columns the step folds in its table
modes (csrc/d2d_capi.hip, refresh_tables: a_tx = a_rx = 0) and the capacity columns sensing.fold_capacity_columns folds.  The planes
are decoded by evaluate.decode_actions.  Torch path only.  The refusal texts are this module's own rows in the form
sensing.refusal_text takes; the out= predicate (all_fit) is PairKernel's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .evaluate import PLANES
from .path_loss_table import ARRAY, CHANNEL, PER_STEP
from .sensing import PairKernel, fold_capacity_columns, r16, refusal_text

LIVE_ROUTES = (CHANNEL, PER_STEP, ARRAY)         # the routes that can have a live [B, N+1, N] dB table ('array': with an SNR row)
# rows of sensing.REFUSALS' form: (subject, what it does with the decoded planes, -, -, which results are device tensors).  A table
# needs no law and no draw, so the route and shadowing texts of refusal_text never come from these rows: no_live_table words the
# one refusal of a route.
ROW = ('evaluate_table()', 'takes its (rb, tx power) planes from the caller', '', '', 'planes')
ROW_ACTIONS = ('evaluate_table_actions()', 'works in the units of the decoded (rb, tx power) planes and reads them for the links on '
               'fixed actions, and export_actions=False does not write them', '', '', 'planes')


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no evaluate_table() (None: it has): the torch path is all it asks of an env - the table comes with the
    call (no_live_table), and no decoded plane is read (fixed_links_refusal: evaluate_table_actions() with links on fixed actions)."""
    return refusal_text(ROW, sim, True, use_torch) if not use_torch else None


def fixed_links_refusal(sim, export_actions: bool) -> Optional[str]:
    """Why evaluate_table_actions() cannot fill in the links on fixed actions (None: it can)."""
    return refusal_text(ROW_ACTIONS, sim, False) if not export_actions else None


def live_table(sim):
    """The env's live dB table [B, N+1, N] as the last fill left it, or None: the route has none bound."""
    t = sim.path_loss_table
    live = t.live if t.route in LIVE_ROUTES else None
    n = len(sim.link_tx)
    return live if live is not None and tuple(live.shape) == (sim.num_envs, n + 1, n) else None


def no_live_table(sim) -> str:
    """The refusal of table=None on a route without a live table."""
    route = sim.path_loss_table.route
    return (f"evaluate_table() has no live dB table to read on the '{route}' path-loss route (the 'channel' and 'per_step' routes "
            "have one, and 'array' when compute() returns the SNR row): pass table=, a float32 or float64 tensor [B, N, N] or "
            '[B, N+1, N] in dB by (tx link, rx link)')


def out_message(device, shapes: dict) -> str:
    """The refusal of an out= that does not fit: evaluate()'s form under this API's name."""
    return ('evaluate_table(): out must be a dict of contiguous float32 tensors (domain: int32) on ' + str(device) + ' that do not '
            'share memory: ' + ', '.join(f'{name} {list(shape)}' for name, shape in shapes.items()))


def lds_bytes(n: int, r: int) -> int:
    """The dynamic LDS one launch asks for, by the layout written in csrc/d2d_evaltab.hip: per link 16 (tx constant, bandwidth,
    rx_lin, noise) + 4 (sensitivity) staged once, 8 (power, link index) + 4 (key) + 4 (RB) per candidate; start[R + 1]; four wave
    sums and four wave flags."""
    n4 = (n + 3) & ~3
    return 16 * n + r16(4 * n) + r16(8 * n) + 4 * n4 + r16(4 * n) + r16(4 * (r + 1)) + 32 + 16


def fold_table_columns(budget: dict) -> np.ndarray:
    """cols float32 [3, D] of d2d_evaluate_table from link_budget_columns(): tx_lin, rx_lin, noise_mw, in double and rounded once -
    rows 0, 2 and 3 of the step's columns in its table modes, where the path loss carries no per-device constant."""
    cols = np.zeros((3, len(budget['noise_dbm'])), dtype=np.float32)
    with np.errstate(over='ignore'):
        for row, name in enumerate(('eirp_off_db', 'rx_off_db', 'noise_dbm')):
            cols[row] = 10.0 ** (np.asarray(budget[name], dtype=np.float64) / 10.0)
    if not ((cols >= 1.0e-30) & (cols <= 1.0e30)).all():
        raise ValueError('a link-budget constant is outside the float32 linear range 1e-30 .. 1e30 (a term beyond +-300 dB)')
    return cols


class TableEvaluate(PairKernel):
    """The table what-if kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch, device) -> None:
        # PairKernel's opening without the law (a table route has none to fold): the same fields, this kernel's columns
        from .device import link_budget_columns
        self.sim, self.torch, self.device = sim, torch, device
        self.b, self.d, self.n = sim.num_envs, sim.handle.num_devices, int(num_links)
        self.r = int(sim.config.num_rbs)
        if self.r > _native.EVALTAB_MAX_RBS:
            raise ValueError(f'evaluate_table() serves at most {_native.EVALTAB_MAX_RBS} RBs (num_rbs = {self.r})')
        tx, rx = np.asarray(sim.link_tx, dtype=np.int32), np.asarray(sim.link_rx, dtype=np.int32)
        if len(tx) != self.n or tx.min() < 0 or tx.max() >= self.d or rx.min() < 0 or rx.max() >= self.d:
            raise ValueError('the link list does not match the env')
        budget = link_budget_columns(sim._dev_list)
        host = {'tx': tx, 'rx': rx, 'cols': fold_table_columns(budget), 'cap_cols': fold_capacity_columns(budget)}
        for name, a in host.items():
            setattr(self, name, torch.as_tensor(a, device=device))
        self.ptrs = tuple(getattr(self, name).data_ptr() for name in host)
        self.own = {}                                # the tensors this object owns, by name; reallocated when K changes
        self.own_k = 0

    def _check_in(self, x, name: str):
        torch = self.torch
        if not (torch.is_tensor(x) and x.ndim == 3 and x.shape[0] == self.b and x.shape[2] == self.n and x.shape[1] >= 1
                and x.dtype == torch.int32 and x.is_contiguous() and x.device == self.device):
            raise ValueError(f'{name} must be a contiguous int32 tensor [{self.b}, K, {self.n}] (env, candidate, link) with K >= 1 on '
                             f'{self.device}')

    def table(self, table):
        """(tensor, entry type, rows per env) of table= (None: the env's live table), or ValueError."""
        torch = self.torch
        if table is None:
            table = live_table(self.sim)
            if table is None:
                raise ValueError(no_live_table(self.sim))
        if not (torch.is_tensor(table) and table.ndim == 3 and table.shape[0] == self.b and table.shape[2] == self.n
                and table.shape[1] in (self.n, self.n + 1) and table.dtype in (torch.float32, torch.float64) and table.is_contiguous()
                and table.device == self.device):
            raise ValueError(f'table must be a contiguous float32 or float64 tensor [{self.b}, {self.n}, {self.n}] or [{self.b}, '
                             f'{self.n + 1}, {self.n}] (env, tx link, rx link) in dB on {self.device}, or None')
        return table, _native.EVALTAB_F64 if table.dtype == torch.float64 else _native.EVALTAB_F32, int(table.shape[1])

    def planes(self, rb, pwr, table, planes, out, stream: int) -> dict:
        torch = self.torch
        self._check_in(rb, 'rb')
        self._check_in(pwr, 'power_dbm')
        if tuple(rb.shape) != tuple(pwr.shape):
            raise ValueError(f'rb and power_dbm must have one shape, got {list(rb.shape)} and {list(pwr.shape)}')
        k = int(rb.shape[1])
        if k > _native.EVALTAB_MAX_CANDIDATES:
            raise ValueError(f'evaluate_table() serves at most {_native.EVALTAB_MAX_CANDIDATES} candidates per call (K = {k})')
        planes = (planes,) if isinstance(planes, str) else tuple(planes)
        if any(p not in PLANES for p in planes) or len(set(planes)) != len(planes):
            raise ValueError(f'planes must be a subset of {PLANES}, got {planes!r}')
        tab, dtype, rows = self.table(table)
        shapes = {'total_mbps': (self.b, k), 'domain': (self.b, k), **{p: (self.b, k, self.n) for p in planes}}
        dtypes = {name: torch.int32 if name == 'domain' else torch.float32 for name in shapes}
        if out is None:
            if self.own_k != k:
                self.own, self.own_k = {}, k
            for name, shape in shapes.items():
                if name not in self.own:
                    self.own[name] = torch.empty(shape, dtype=dtypes[name], device=self.device)
            res = {name: self.own[name] for name in shapes}
        else:
            if not (isinstance(out, dict) and set(out) == set(shapes)
                    and self.all_fit([out[name] for name in shapes], list(shapes.values()), [dtypes[name] for name in shapes])):
                raise ValueError(out_message(self.device, shapes))
            res = {name: out[name] for name in shapes}
        _native.evaluate_table(tab.data_ptr(), dtype, rows, rb.data_ptr(), pwr.data_ptr(), *self.ptrs, self.b, k, self.d, self.n, self.r,
                               res['sinr_db'].data_ptr() if 'sinr_db' in res else 0,
                               res['capacity_mbps'].data_ptr() if 'capacity_mbps' in res else 0, res['total_mbps'].data_ptr(),
                               res['domain'].data_ptr(), stream)
        return res

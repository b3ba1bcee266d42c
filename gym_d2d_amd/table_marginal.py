"""Difference rewards (leave-one-out capacity) on a path-loss table: the host side of libd2d_tabmarg.so (include/d2d_tabmarg.h,
csrc/d2d_tabmarg.hip).

marginal.MarginalCapacity serves the native power-law models: its kernel evaluates a law at the positions.  `TableMarginal` serves
the envs whose step reads a dB table by (tx link, rx link) - the 'channel' route, the 'per_step' route, 'array' with an SNR row - and,
through table=, any env at all.  It is a table_evaluate.TableEvaluate - the same constants (the columns the step folds in its table
modes, the capacity columns), the same table= check - with one launch per call and no work space: the entries are read in place.
`lds_bytes` restates the header's formula.  Torch path only.  The refusal texts are this module's own rows in the form
sensing.refusal_text takes; the out= check and the owned outputs are PairKernel's.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

from . import _native, table_evaluate
from .sensing import r16, refusal_text
from .table_evaluate import TableEvaluate, live_table

# a row of sensing.REFUSALS' form (table_evaluate.ROW's): a table needs no law and no draw, so only the torch-path text comes from it
ROW = ('marginal_capacity_table()', 'takes its (rb, tx power) planes from the caller', '', '', 'planes')
API = 'marginal_capacity_table()'


class TableMarginalResult(NamedTuple):
    """What marginal_capacity_table() returns: a tuple with names."""
    difference_mbps: object    # float32 [B, N]: evaluate_table()'s capacity_mbps - harm_mbps
    harm_mbps: object          # float32 [B, N]: what the other links of the link's RB would gain if it alone went off the air
    domain: object             # int32 [B]: 1 - an entry read for this state is NaN or -inf


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no marginal_capacity_table() (None: it has): the torch path is all it asks of an env - the table comes with
    the call (no_live_table) and so may the planes (no_start_state)."""
    return refusal_text(ROW, sim, True, use_torch) if not use_torch else None


def no_live_table(sim) -> str:
    """The refusal of table=None on a route without a live table: table_evaluate.no_live_table under this API's name."""
    return table_evaluate.no_live_table(sim).replace('evaluate_table()', API, 1)


def no_start_state(api: str = API) -> str:
    """The refusal of rb=None / power_dbm=None on an env that does not export its decoded planes."""
    return (f'{api} reads the decoded (rb, tx power) planes of the last step, which export_actions=False does not write: '
            'build the env with export_actions=True, or pass rb= and power_dbm=, contiguous int32 [B, N] tensors')


def reward_refusal(sim, export_actions: bool, use_torch: bool, who: str) -> Optional[str]:
    """Why an env cannot hand `who` (a reward or obs function's class name) the table difference rewards on every step (None: it
    can): the step's launch takes the live table and the decoded planes, so the env must have both, on the torch path."""
    if not use_torch:
        return f'{who} needs the torch path (use_torch): {API} works on device tensors'
    if sim.path_loss_table.route not in table_evaluate.LIVE_ROUTES:
        return (f"{who} needs a live dB table, which the '{sim.path_loss_table.route}' path-loss route does not have (the 'channel' and "
                "'per_step' routes have one, and 'array' when compute() returns the SNR row): use DifferenceRewardFunction on the "
                'native power-law models')
    if not export_actions:
        return f'{who}: ' + no_start_state()
    return None


def lds_bytes(n: int, r: int) -> int:
    """The LDS one workgroup of the kernel needs: the formula of include/d2d_tabmarg.h."""
    n4 = (n + 3) & ~3
    return 16 * n + r16(8 * n) + 8 * n4 + 3 * r16(4 * n) + r16(4 * (r + 1)) + 16


class TableMarginal(TableEvaluate):
    """The table difference-reward kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch, device) -> None:
        if int(sim.config.num_rbs) > _native.TABMARG_MAX_RBS:
            raise ValueError(f'{API} serves at most {_native.TABMARG_MAX_RBS} RBs (num_rbs = {int(sim.config.num_rbs)})')
        super().__init__(sim, num_links, torch, device)
        if self.n > _native.TABMARG_MAX_LINKS:
            raise ValueError(f'{API} serves at most {_native.TABMARG_MAX_LINKS} links (num_links = {self.n})')
        need = lds_bytes(self.n, self.r)
        if need > _native.TABMARG_MAX_LDS_BYTES:     # no shape within the two limits gets here: stated for a limit that moves
            raise ValueError(f'{API} keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} bytes, more '
                             f'than {_native.TABMARG_MAX_LDS_BYTES}')
        self.declare_outputs(TableMarginalResult._fields, ((self.b, self.n), (self.b, self.n), (self.b,)),
                             (torch.float32, torch.float32, torch.int32))

    def table(self, table):
        """TableEvaluate.table() with the refusal of a route without a live table under this API's name."""
        if table is None and live_table(self.sim) is None:
            raise ValueError(no_live_table(self.sim))
        return super().table(table)

    def start(self, x, name: str):
        """An explicit plane: a contiguous int32 tensor [B, N] on the env's device, or ValueError."""
        if not self.fits(x, (self.b, self.n), self.torch.int32):
            raise ValueError(f'{name} must be a contiguous int32 tensor [{self.b}, {self.n}] (env, link) on {self.device}, or None')
        return x

    def marginal(self, table, rb, pwr, out, stream: int) -> TableMarginalResult:
        """table: what the caller passed (None: the live table); rb, pwr: the planes, checked by start() or the env's own."""
        tab, dtype, rows = self.table(table)
        diff, harm, domain = self.outputs(out)
        _native.table_marginal(tab.data_ptr(), dtype, rows, rb.data_ptr(), pwr.data_ptr(), *self.ptrs, self.b, self.d, self.n, self.r,
                               harm.data_ptr(), diff.data_ptr(), domain.data_ptr(), stream)
        return TableMarginalResult(diff, harm, domain)

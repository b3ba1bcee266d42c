"""Sum-capacity RB ascent with SINR floors on a path-loss table: the host side of libd2d_tabascent.so (include/d2d_tabascent.h,
csrc/d2d_tabascent.hip).

rb_ascent.RbAscent serves the native power-law models: its kernel evaluates a law at the positions.  `TableRbAscent` serves the envs
whose step reads a dB table by (tx link, rx link) and, through table=, any env at all.  It is a table_evaluate.TableEvaluate - the
same constants (the columns the step folds in its table modes, the capacity columns), the same table= check - that also owns the
kernel's WORK SPACE: the table converted once per call into float32 linear gains, `4 B N N` bytes, allocated by the first call and
kept (4.3 GB at 4096 envs x 512 links).  `lds_bytes` restates the header's formula.  The allowed mask goes through
best_response.words / pack_allowed, the floor is power_control.link_values, the movable set PairKernel.agent_subset, the action
encoding best_response_dynamics.encode_actions.  Torch path only.  The out= check and the owned outputs are PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native, table_evaluate
from .best_response import words
from .power_control import link_values
from .sensing import r16, refusal_text
from .table_evaluate import TableEvaluate, live_table

# a row of sensing.REFUSALS' form (table_evaluate.ROW's): a table needs no law and no draw, so only the torch-path text comes from it
ROW = ('rb_ascent_table()', 'takes its (rb, tx power) planes from the caller', '', '', 'planes')


class TableRbAscentResult(NamedTuple):
    """What rb_ascent_table() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the RBs the ascent ended at
    sinr_db: object            # float32 [B, N]: evaluate_table()'s plane for (rb, the given powers) on the table
    capacity_mbps: object      # float32 [B, N]: likewise
    rounds: object             # int32 [B]: the rounds that moved a link; max_rounds at the cap
    moves: object              # int32 [B]: the moves made
    converged: object          # uint8 [B]: 1 - a round moved nobody
    domain: object             # int32 [B]: 1 - an entry [j, i], j, i < N, of the env's block is NaN or -inf


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no rb_ascent_table() (None: it has): the torch path is all it asks of an env - the table comes with the call
    (no_live_table) and so may the start state (no_start_state)."""
    return refusal_text(ROW, sim, True, use_torch) if not use_torch else None


def no_live_table(sim) -> str:
    """The refusal of table=None on a route without a live table: table_evaluate.no_live_table under this API's name."""
    return table_evaluate.no_live_table(sim).replace('evaluate_table()', 'rb_ascent_table()', 1)


def no_start_state(api: str = 'rb_ascent_table()') -> str:
    """The refusal of rb=None / power_dbm=None on an env that does not export its decoded planes."""
    return (f'{api} starts from the decoded (rb, tx power) planes of the last step, which export_actions=False does not write: '
            'build the env with export_actions=True, or pass rb= and power_dbm=, contiguous int32 [B, N] tensors')


def lds_bytes(n: int, r: int, allowed: bool = False) -> int:
    """The LDS one workgroup of the ascent kernel needs: the formula of include/d2d_tabascent.h."""
    n4 = (n + 3) & ~3
    return (16 * n + 2 * r16(4 * n) + 8 * n4 + (r16(4 * n * ((r + 31) // 32)) if allowed else 0)
            + r16(4 * ((n + 31) // 32) * r) + 112)


def work_space_bytes(b: int, n: int) -> int:
    """The bytes of the float32 gain block the object owns: 4 B N N."""
    return 4 * b * n * n


class TableRbAscent(TableEvaluate):
    """The table ascent bound to one env object: constants uploaded once, the work space allocated by the first call, one call of
    the library (two kernel launches) per solve."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, agent, torch, device) -> None:
        if int(sim.config.num_rbs) > _native.TABASCENT_MAX_RBS:
            raise ValueError(f'rb_ascent_table() serves at most {_native.TABASCENT_MAX_RBS} RBs (num_rbs = {int(sim.config.num_rbs)})')
        super().__init__(sim, num_links, torch, device)
        if self.n > _native.TABASCENT_MAX_LINKS:
            raise ValueError(f'rb_ascent_table() serves at most {_native.TABASCENT_MAX_LINKS} links (num_links = {self.n})')
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever moved
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        self._subset = None                          # PairKernel.agent_subset()'s cache
        self._agent_dev = None
        self._target = None                          # (key, tensor) of the last host floor: a repeat is not uploaded again
        self.need(False)                             # a shape no call could serve is refused when the object is made
        self.declare_outputs(TableRbAscentResult._fields, ((self.b, self.n),) * 3 + ((self.b,),) * 4,
                             (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8, torch.int32))
        self.gains = None                            # the work space, float32 [B, N, N]: allocated by the first call

    def need(self, allowed: bool) -> int:
        """lds_bytes of this env, with or without an allowed mask; ValueError past the limit, stating the byte count."""
        need = lds_bytes(self.n, self.r, allowed)
        if need > _native.TABASCENT_MAX_LDS_BYTES:
            raise ValueError(f'rb_ascent_table() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} '
                             f'bytes{" with an allowed mask" if allowed else ""}, more than {_native.TABASCENT_MAX_LDS_BYTES}')
        return need

    def table(self, table):
        """TableEvaluate.table() with the refusal of a route without a live table under this API's name."""
        if table is None and live_table(self.sim) is None:
            raise ValueError(no_live_table(self.sim))
        return super().table(table)

    def start(self, x, name: str):
        """An explicit start plane: a contiguous int32 tensor [B, N] on the env's device, or ValueError."""
        if not self.fits(x, (self.b, self.n), self.torch.int32):
            raise ValueError(f'{name} must be a contiguous int32 tensor [{self.b}, {self.n}] (env, link) on {self.device}, or None')
        return x

    def floor(self, floor_sinr_db, num_cues: int):
        """float32 [N] on the device from None (no floors: -inf), a scalar, {'cue': x, 'due': y} or [N] values (array or tensor);
        -inf: that link has no floor."""
        return link_values(self, -np.inf if floor_sinr_db is None else floor_sinr_db, num_cues, 'floor_sinr_db')

    def movable(self, movable):
        """uint8 [N] on the device: the agent links (None), or those of them `movable` (bool [N], array or tensor) marks."""
        return self.agent_subset(movable, 'movable')

    def solve(self, table, rb, pwr, allowed, movable, floor, min_gain_mbps: float, max_rounds: int, out, stream: int,
              env_mask=None) -> TableRbAscentResult:
        """table: what the caller passed (None: the live table); rb, pwr: the start planes, checked by start() or the env's own;
        movable, floor: the tensors movable() and floor() return; allowed: what the caller passed."""
        if isinstance(min_gain_mbps, bool) or not isinstance(min_gain_mbps, (int, float, np.integer, np.floating)) \
                or not math.isfinite(min_gain_mbps) or min_gain_mbps < 0:
            raise ValueError(f'min_gain_mbps must be a finite number >= 0, got {min_gain_mbps!r}')
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) \
                or not 1 <= max_rounds <= _native.TABASCENT_MAX_ROUNDS:
            raise ValueError(f'max_rounds must be an int in [1, {_native.TABASCENT_MAX_ROUNDS}], got {max_rounds!r}')
        self.need(allowed is not None)
        tab, dtype, rows = self.table(table)
        res = self.outputs(out)
        words = self.words(allowed)                  # lives until the launch is enqueued; the stream orders its release behind it
        mask = self.env_mask(env_mask)
        if self.gains is None:
            self.gains = self.torch.empty((self.b, self.n, self.n), dtype=self.torch.float32, device=self.device)
        _native.table_rb_ascent(tab.data_ptr(), dtype, rows, rb.data_ptr(), pwr.data_ptr(), *self.ptrs, self.b, self.d, self.n, self.r,
                                0 if words is None else words.data_ptr(), movable.data_ptr(), floor.data_ptr(), float(min_gain_mbps),
                                int(max_rounds), 0 if mask is None else mask.data_ptr(), self.gains.data_ptr(),
                                *(o.data_ptr() for o in res), stream)
        return TableRbAscentResult(*res)

    def close(self) -> None:
        self.gains = None
        super().close()

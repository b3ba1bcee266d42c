"""Queue-aware goodput ascent over RBs and powers: the host side of libd2d_goodput.so (include/d2d_goodput.h, csrc/d2d_goodput.hip).

`GoodputAscent` owns the device-side constants of one env object (link lists, the columns sensing.fold_columns and
sensing.fold_capacity_columns fold, unchanged, the power bounds of every link's class) and launches the ascent on torch's device
pointers: one launch per call, every turn of every round of every env inside it.  `lds_bytes` restates the header's formula.  The
allowed mask goes through best_response.words / pack_allowed, the floor is power_control.link_values, the action encoding is
power_control.encode_actions on the solved RBs and powers.  Torch path only.  The refusal texts are `REFUSAL`,
best_response_dynamics()'s row of sensing.REFUSALS under this name with a shadowing clause of its own, as rb_ascent.REFUSAL is; the
out= check, the owned outputs and the launch prefix are PairKernel's.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .best_response import words
from .power_control import link_values
from .sensing import REFUSALS, PairKernel, r16, refusal_text

REFUSAL = ('goodput_ascent()', *REFUSALS['best_response_dynamics'][1:3],
           'ascent (the capacity a move was made for is another draw than the one the next link sees)', 'planes')
MOVES = {'rb': _native.GOODPUT_MOVE_RB, 'power': _native.GOODPUT_MOVE_POWER}
INT32_MAX = (1 << 31) - 1


class GoodputAscentResult(NamedTuple):
    """What goodput_ascent() returns: a tuple with names."""
    rb: object                 # int32 [B, N]: the RBs the ascent ended at
    power_dbm: object          # int32 [B, N]: the powers it ended at
    sinr_db: object            # float32 [B, N]: evaluate()'s plane for (rb, power_dbm)
    capacity_mbps: object      # float32 [B, N]: likewise
    served_bits: object        # int32 [B, N]: min(budget(capacity_mbps), demand_bits)
    value: object              # int64 [B]: the sum of weight * served_bits over all links
    rounds: object             # int32 [B]: the rounds that moved a link; max_rounds at the cap
    moves: object              # int32 [B]: the moves made
    converged: object          # uint8 [B]: 1 - a round moved nobody


def refusal(sim, export_actions: bool, use_torch: bool = True) -> Optional[str]:
    """Why this env has no goodput_ascent() (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text(REFUSAL, sim, export_actions, use_torch)


def lds_bytes(n: int, r: int, allowed: bool = False) -> int:
    """The LDS one workgroup of d2d_goodput_ascent needs: the formula of include/d2d_goodput.h."""
    return 96 * n + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 208


def move_mask(move) -> int:
    """The move_mask word of `move`, a non-empty collection of 'rb' and 'power' (or one of the two names)."""
    names = (move,) if isinstance(move, str) else move
    if not isinstance(names, (tuple, list, set, frozenset)) or len(names) == 0 or not all(isinstance(m, str) and m in MOVES for m in names):
        raise ValueError(f"move must name 'rb', 'power' or both, got {move!r}")
    mask = 0
    for m in names:
        mask |= MOVES[m]
    return mask


class GoodputAscent(PairKernel):
    """The ascent kernel bound to one env object: constants uploaded once, one launch per call."""
    words = words                                # best_response.words, as a method: self.words(allowed)

    def __init__(self, sim, num_links: int, p_min, p_max, agent, torch, device) -> None:
        super().__init__(sim, num_links, torch, device, api='goodput_ascent', max_rbs=_native.GOODPUT_MAX_RBS, capacity=True)
        p_min, p_max = np.asarray(p_min, dtype=np.int32), np.asarray(p_max, dtype=np.int32)
        self.agent = np.asarray(agent, dtype=bool)                   # links that have an action column: the only ones ever moved
        if self.agent.shape != (self.n,):
            raise ValueError('the agent mask does not match the env')
        if not (p_min.shape == p_max.shape == (self.n,)) or (p_min > p_max).any() or max(np.abs(p_max).max(), np.abs(p_min).max()) >= 4096:
            raise ValueError('the power bounds do not match the env')
        levels = int((p_max.astype(np.int64) - p_min + 1)[self.agent].max()) if self.agent.any() else 1
        if levels > _native.GOODPUT_MAX_LEVELS:
            raise ValueError(f'goodput_ascent() packs a power level into six bits of its choice: at most {_native.GOODPUT_MAX_LEVELS} '
                             f'levels (D2D_GOODPUT_MAX_LEVELS), got {levels}')
        self.need(False)                                             # a shape no call could serve is refused when the object is made
        self.declare_outputs(GoodputAscentResult._fields, ((self.b, self.n),) * 5 + ((self.b,),) * 4,
                             (torch.int32, torch.int32, torch.float32, torch.float32, torch.int32, torch.int64, torch.int32, torch.int32,
                              torch.uint8))
        self.p_min, self.p_max = (torch.as_tensor(a, device=device) for a in (p_min, p_max))
        self._target = None                          # (key, tensor) of the last host floor: a repeat is not uploaded again

    def need(self, allowed: bool) -> int:
        """lds_bytes of this env, with or without an allowed mask; ValueError past the limit, stating the byte count."""
        need = lds_bytes(self.n, self.r, allowed)
        if need > _native.GOODPUT_MAX_LDS_BYTES:
            raise ValueError(f'goodput_ascent() keeps an env in the LDS of one workgroup: {self.n} links on {self.r} RBs need {need} bytes'
                             f'{" with an allowed mask" if allowed else ""}, more than {_native.GOODPUT_MAX_LDS_BYTES}')
        return need

    def floor(self, floor_sinr_db, num_cues: int):
        """float32 [N] on the device from None (no floors: -inf), a scalar, {'cue': x, 'due': y} or [N] values (array or tensor);
        -inf: that link has no floor."""
        return link_values(self, -np.inf if floor_sinr_db is None else floor_sinr_db, num_cues, 'floor_sinr_db')

    def movable(self, movable):
        """uint8 [N] on the device: the agent links (None), or those of them `movable` (bool [N], array or tensor) marks."""
        return self.agent_subset(movable, 'movable')

    def plane(self, values, name: str, lo: int, hi: int):
        """None, or int32 [B, N] on the device from an int scalar, [N] or [B, N] values (array or tensor), broadcast.  Host values
        outside [lo, hi] are a ValueError; a tensor is never read on the host (nothing is synchronised): it is refused by its
        metadata, and what the kernel makes of a word outside the range is the header's."""
        torch = self.torch
        shapes = ((), (self.n,), (self.b, self.n))
        what = f'{name} must be None or ints, a scalar, [{self.n}] or [{self.b}, {self.n}]'
        if values is None:
            return None
        if torch.is_tensor(values):
            if tuple(values.shape) not in shapes or values.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
                raise ValueError(what)
            t = values.to(self.device)
            if t.dtype == torch.int64:
                t = t.clamp(-INT32_MAX - 1, INT32_MAX)
            return t.to(torch.int32).expand(self.b, self.n).contiguous()
        if isinstance(values, bool):
            raise ValueError(what)
        host = np.asarray(values)
        if host.shape not in shapes or host.dtype.kind not in 'iu':
            raise ValueError(what)
        if host.size and (int(host.min()) < lo or int(host.max()) > hi):
            raise ValueError(f'{name} must lie in [{lo}, {hi}], got {int(host.min())} .. {int(host.max())}')
        return torch.as_tensor(np.array(np.broadcast_to(host, (self.b, self.n)), dtype=np.int32, order='C'), device=self.device)

    def solve(self, t: dict, demand_bits, weight, bits_per_mbps: float, move, allowed, movable, floor, min_gain_bits: int, max_rounds: int,
              out, stream: int, env_mask=None) -> GoodputAscentResult:
        """movable, floor: the tensors movable() and floor() return; demand_bits, weight, allowed, move: what the caller passed."""
        mask_word = move_mask(move)
        if isinstance(bits_per_mbps, bool) or not isinstance(bits_per_mbps, (int, float, np.integer, np.floating)) \
                or not math.isfinite(bits_per_mbps) or not bits_per_mbps > 0:
            raise ValueError(f'bits_per_mbps must be a finite number > 0, got {bits_per_mbps!r}')
        if isinstance(min_gain_bits, bool) or not isinstance(min_gain_bits, (int, np.integer)) or not 0 <= min_gain_bits < 1 << 62:
            raise ValueError(f'min_gain_bits must be an int in [0, 2^62), got {min_gain_bits!r}')
        if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) \
                or not 1 <= max_rounds <= _native.GOODPUT_MAX_ROUNDS:
            raise ValueError(f'max_rounds must be an int in [1, {_native.GOODPUT_MAX_ROUNDS}], got {max_rounds!r}')
        self.need(allowed is not None)
        res = self.outputs(out)
        # these live until the launch is enqueued; the stream orders their release behind it
        dem = self.plane(demand_bits, 'demand_bits', -INT32_MAX - 1, INT32_MAX)
        wgt = self.plane(weight, 'weight', 0, _native.GOODPUT_MAX_WEIGHT)
        words = self.words(allowed)
        mask = self.env_mask(env_mask)
        ptr = lambda x: 0 if x is None else x.data_ptr()
        _native.goodput_ascent(*self.launch_args(t), self.p_min.data_ptr(), self.p_max.data_ptr(), ptr(wgt), ptr(dem), float(bits_per_mbps),
                               ptr(words), movable.data_ptr(), floor.data_ptr(), mask_word, int(min_gain_bits), int(max_rounds), ptr(mask),
                               *(o.data_ptr() for o in res), stream)
        return GoodputAscentResult(*res)

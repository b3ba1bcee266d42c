"""Difference rewards (leave-one-out capacity): the host side of libd2d_marginal.so (include/d2d_marginal.h, csrc/d2d_marginal.hip).

`fold_capacity_columns` (stated in sensing.py, next to fold_columns) lowers what the capacity needs beyond sensing.fold_columns'
block - the transmitter's bandwidth and the receiver's threshold - by the rules the step's own records follow (csrc/d2d_capi.hip,
refresh_tables), so that the capacity the kernel forms for a link is the step's plane.  `MarginalCapacity` owns the device-side
constants of one env object and launches the kernel on device pointers: torch tensors on the torch path, plain HIP allocations on
the NumPy path.  The refusal texts are the 'marginal_capacity' row of
sensing.REFUSALS; the torch path's out= predicate (fits) and the launch prefix (launch_args) are PairKernel's.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import _native
from .sensing import PairKernel, fold_capacity_columns, refusal_text      # fold_capacity_columns stays a name of this module too


def refusal(sim, export_actions: bool) -> Optional[str]:
    """Why this env has no difference rewards (None: it has): the predicate of sensing.unserved under texts of its own."""
    return refusal_text('marginal_capacity', sim, export_actions)


class MarginalCapacity(PairKernel):
    """The difference-reward kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch=None, device=None) -> None:
        super().__init__(sim, num_links, torch, device, api='marginal_capacity', max_rbs=_native.MARGINAL_MAX_RBS, capacity=True)
        self.own = None                              # the (difference, harm) pair this object owns, allocated by the first call without out=

    def _check_out(self, out, is_plane, what: str) -> Tuple:
        if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(is_plane(o) for o in out) or out[0] is out[1]:
            raise ValueError(f'out must be (difference_mbps, harm_mbps), two {what}')
        return tuple(out)

    def torch_planes(self, t: dict, out, stream: int):
        torch = self.torch
        shape = (self.b, self.n)
        if out is None:
            if self.own is None:
                self.own = tuple(torch.empty(shape, dtype=torch.float32, device=self.device) for _ in range(2))
            out = self.own
        else:
            out = self._check_out(out, lambda o: self.fits(o, shape, torch.float32),
                                  f'contiguous float32 tensors {list(shape)} on {self.device}')
            if out[0].data_ptr() == out[1].data_ptr():
                raise ValueError('out must be (difference_mbps, harm_mbps), two tensors that do not share memory')
        diff, harm = out
        _native.marginal_capacity(*self.launch_args(t), harm.data_ptr(), diff.data_ptr(), stream)
        return diff, harm

    def numpy_planes(self, out):
        h = self.sim.handle
        shape = (self.b, self.n)
        if out is not None:
            out = self._check_out(out, lambda o: isinstance(o, np.ndarray) and o.shape == shape and o.dtype == np.float32
                                  and o.flags.c_contiguous, f'C-contiguous float32 ndarrays {list(shape)}')
        h.synchronize()                               # the planes are the last step's; the kernel runs on the null stream
        planes = [h.get_buffer(w)[0] for w in (_native.BUF_POS_X, _native.BUF_POS_Y, _native.BUF_RB, _native.BUF_PWR)]
        if self.own is None:
            self.own = tuple(self.mem.alloc(self.b * self.n * 4) for _ in range(2))
        _native.marginal_capacity(*self.raw_launch_args(*planes), self.own[1], self.own[0], 0)
        res = out if out is not None else tuple(np.empty(shape, dtype=np.float32) for _ in range(2))
        for dev, host in zip(self.own, res):
            self.mem.download(dev, host)              # synchronous on the null stream: behind the kernel
        return res

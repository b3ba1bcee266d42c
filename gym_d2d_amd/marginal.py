"""Difference rewards (leave-one-out capacity): the host side of libd2d_marginal.so (include/d2d_marginal.h, csrc/d2d_marginal.hip).

`fold_capacity_columns` (stated in sensing.py, next to fold_columns) lowers what the capacity needs beyond sensing.fold_columns'
block - the transmitter's bandwidth and the receiver's threshold - by the rules the step's own records follow (csrc/d2d_capi.hip,
refresh_tables), so that the capacity the kernel forms for a link is the step's plane.  `MarginalCapacity` owns the device-side constants of one env object and launches the
kernel on device pointers: torch tensors on the torch path, plain HIP allocations on the NumPy path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import _native
from .sensing import PairKernel, fold_capacity_columns, unserved      # fold_capacity_columns stays a name of this module too


def refusal(sim, export_actions: bool) -> Optional[str]:
    """Why this env has no difference rewards (None: it has): the predicate of sensing.unserved under texts of its own."""
    why = unserved(sim, export_actions)
    if why is None:
        return None
    kind, route = why
    return {
        'export_actions': 'marginal_capacity() reads the decoded (rb, tx power) planes, which export_actions=False does not write: '
                          'build the env with export_actions=True',
        'route': f"marginal_capacity() does not serve the '{route}' path-loss route (a table, not a law its kernel can evaluate "
                 'from the transmitter\'s side); it serves the native power-law models',
        'shadowing': 'marginal_capacity() does not serve ShadowingPathLoss: a fresh draw per evaluation has no counterfactual (the '
                     'step without one link would be another draw)',
        'pinned': 'marginal_capacity() does not serve pinned device_config coordinates that float32 cannot hold: their low parts '
                  'live inside the handle (float64 positions)',
    }[kind]


class MarginalCapacity(PairKernel):
    """The difference-reward kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch=None, device=None) -> None:
        super().__init__(sim, num_links, torch, device, api='marginal_capacity', max_rbs=_native.MARGINAL_MAX_RBS, capacity=True)
        self.own = None                              # the (difference, harm) pair this object owns, allocated by the first call without out=

    def launch(self, pos_x: int, pos_y: int, rb: int, pwr: int, harm: int, diff: int, stream: int = 0) -> None:
        _native.marginal_capacity(pos_x, pos_y, rb, pwr, *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n, self.r, harm, diff,
                                  stream)

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
            out = self._check_out(out, lambda o: torch.is_tensor(o) and tuple(o.shape) == shape and o.dtype == torch.float32
                                  and o.is_contiguous() and o.device == self.device,
                                  f'contiguous float32 tensors {list(shape)} on {self.device}')
            if out[0].data_ptr() == out[1].data_ptr():
                raise ValueError('out must be (difference_mbps, harm_mbps), two tensors that do not share memory')
        diff, harm = out
        self.launch(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), t['rb'].data_ptr(), t['pwr'].data_ptr(), harm.data_ptr(),
                    diff.data_ptr(), stream)
        return diff, harm

    def numpy_planes(self, out):
        h = self.sim.handle
        shape = (self.b, self.n)
        if out is not None:
            out = self._check_out(out, lambda o: isinstance(o, np.ndarray) and o.shape == shape and o.dtype == np.float32
                                  and o.flags.c_contiguous, f'C-contiguous float32 ndarrays {list(shape)}')
        h.synchronize()                               # the planes are the last step's; the kernel runs on the null stream
        ptr = {w: h.get_buffer(w)[0] for w in (_native.BUF_POS_X, _native.BUF_POS_Y, _native.BUF_RB, _native.BUF_PWR)}
        if self.own is None:
            self.own = tuple(self.mem.alloc(self.b * self.n * 4) for _ in range(2))
        self.launch(ptr[_native.BUF_POS_X], ptr[_native.BUF_POS_Y], ptr[_native.BUF_RB], ptr[_native.BUF_PWR], self.own[1], self.own[0])
        res = out if out is not None else tuple(np.empty(shape, dtype=np.float32) for _ in range(2))
        for dev, host in zip(self.own, res):
            self.mem.download(dev, host)              # synchronous on the null stream: behind the kernel
        return res

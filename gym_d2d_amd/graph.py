"""The interference graph: the host side of libd2d_graph.so (include/d2d_graph.h, csrc/d2d_graph.hip).

    coupling_db[b, i, j] = eirp_off_db[tx_j] - PL(tx_j -> rx_i)      dBm received at rx_i per 0 dBm of tx power of link j

INDEX ORDER: [b, i, j] is receiver-major - i is the receiving link (the agent), j the transmitting one, one agent's row contiguous.
The path-loss tables elsewhere in the project are [b, j, i].  `NeighborGraph` owns the device-side constants of one env object (link
lists, the columns `sensing.fold_columns` folds, so a pair has the bits the step and sense() give it) and the env's own result
blocks, and launches the three kernels on device pointers: torch tensors on the torch path, plain HIP allocations on the NumPy path.
The refusal texts are the 'graph' row of sensing.REFUSALS; the torch path's out= predicate (fits) is PairKernel's.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .sensing import PairKernel, refusal_text


def refusal(sim, export_actions: bool) -> Optional[str]:
    """Why this env has no neighbour graph (None: it has one): the predicate of sensing.unserved under the graph's own texts."""
    return refusal_text('graph', sim, export_actions)


def check_k(k, num_links: int) -> int:
    """k as an int in 1 .. min(N - 1, 64), or ValueError."""
    top = min(num_links - 1, _native.GRAPH_MAX_K)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= top:
        raise ValueError(f'k must be an int in 1 .. min(N - 1, {_native.GRAPH_MAX_K}) = {top} (N = {num_links} links), got {k!r}')
    return int(k)


class NeighborGraph(PairKernel):
    """The graph kernels bound to one env object: constants uploaded once, one launch per call.  Index order [b, i, j] / [b, i, m]:
    receiver i first (module docstring)."""

    def __init__(self, sim, num_links: int, torch=None, device=None) -> None:
        super().__init__(sim, num_links, torch, device)              # no RB cap: the graph reads no RB
        self.own = {}                                # the result blocks this object owns, by name, allocated on first use

    # ------------------------------------------------------------------ torch path
    def _out_torch(self, name: str, out, shape, dtype):
        torch = self.torch
        if out is None:
            if name not in self.own:
                self.own[name] = torch.empty(shape, dtype=dtype, device=self.device)
            return self.own[name]
        if not self.fits(out, shape, dtype):
            kind = 'int32' if dtype == torch.int32 else 'float32'
            raise ValueError(f'out must be a contiguous {kind} tensor {list(shape)} on {self.device}')
        return out

    def coupling_torch(self, t: dict, out, stream: int):
        out = self._out_torch('coupling', out, (self.b, self.n, self.n), self.torch.float32)
        _native.graph_coupling(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n,
                               out.data_ptr(), stream)
        return out

    def neighbors_torch(self, t: dict, k: int, out, stream: int, env_mask=None):
        torch = self.torch
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError('out must be a pair (idx, coupling_db)')
        shape = (self.b, self.n, k)
        idx = self._out_torch(f'idx{k}', None if out is None else out[0], shape, torch.int32)
        cdb = self._out_torch(f'cdb{k}', None if out is None else out[1], shape, torch.float32)
        _native.graph_neighbors(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n,
                                k, 0 if env_mask is None else env_mask.data_ptr(), idx.data_ptr(), cdb.data_ptr(), stream)
        return idx, cdb

    def obs_torch(self, t: dict, k: int, idx, cdb, stream: int):
        out = self._out_torch(f'obs{k}', None, (self.b, self.n, 4 * (k + 1)), self.torch.float32)
        _native.graph_neighbor_obs(idx.data_ptr(), cdb.data_ptr(), t['rb'].data_ptr(), t['pwr'].data_ptr(), t['sinr_db'].data_ptr(),
                                   t['snr_db'].data_ptr(), self.b, self.n, k, out.data_ptr(), stream)
        return out

    # ------------------------------------------------------------------ NumPy path
    def _out_numpy(self, out, shape, dtype):
        if out is None:
            return np.empty(shape, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.shape != tuple(shape) or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f'out must be a C-contiguous {np.dtype(dtype).name} ndarray {list(shape)}')
        return out

    def _dev(self, name: str, nbytes: int) -> int:
        if name not in self.own:
            self.own[name] = self.mem.alloc(nbytes)
        return self.own[name]

    def _positions(self):
        h = self.sim.handle
        h.synchronize()                               # the state is the last step's; the kernels run on the null stream
        return h.get_buffer(_native.BUF_POS_X)[0], h.get_buffer(_native.BUF_POS_Y)[0]

    def coupling_numpy(self, out):
        res = self._out_numpy(out, (self.b, self.n, self.n), np.float32)
        px, py = self._positions()
        dev = self._dev('coupling', res.nbytes)
        _native.graph_coupling(px, py, *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n, dev)
        self.mem.download(dev, res)                   # synchronous on the null stream: behind the kernel
        return res

    def neighbors_numpy(self, k: int, out):
        if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
            raise ValueError('out must be a pair (idx, coupling_db)')
        shape = (self.b, self.n, k)
        idx = self._out_numpy(None if out is None else out[0], shape, np.int32)
        cdb = self._out_numpy(None if out is None else out[1], shape, np.float32)
        px, py = self._positions()
        d_idx, d_cdb = self._dev(f'idx{k}', idx.nbytes), self._dev(f'cdb{k}', cdb.nbytes)
        _native.graph_neighbors(px, py, *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n, k, 0, d_idx, d_cdb)
        self.mem.download(d_idx, idx)
        self.mem.download(d_cdb, cdb)
        return idx, cdb

    def obs_numpy(self, k: int):
        """The observation from the device-side idx / coupling_db the last neighbors_numpy(k) left."""
        h = self.sim.handle
        h.synchronize()
        ptr = {w: h.get_buffer(w)[0] for w in (_native.BUF_RB, _native.BUF_PWR, _native.BUF_SINR_DB, _native.BUF_SNR_DB)}
        res = np.empty((self.b, self.n, 4 * (k + 1)), dtype=np.float32)
        dev = self._dev(f'obs{k}', res.nbytes)
        _native.graph_neighbor_obs(self.own[f'idx{k}'], self.own[f'cdb{k}'], ptr[_native.BUF_RB], ptr[_native.BUF_PWR],
                                   ptr[_native.BUF_SINR_DB], ptr[_native.BUF_SNR_DB], self.b, self.n, k, dev)
        self.mem.download(dev, res)
        return res

    def close(self) -> None:
        super().close()
        self.own.clear()

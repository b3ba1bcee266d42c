"""Per-RB interference sensing: the host side of libd2d_sense.so (include/d2d_sense.h, csrc/d2d_sense.hip), and what the host
modules of all the stateless pair kernels share.

`fold_columns` lowers the per-device link-budget and power-law columns to the float32 block the kernel reads, in double precision
and by the rules the step's own records follow (csrc/d2d_capi.hip, refresh_tables), so that the sensed column of a link's own RB is
the step's sinr_db.  `unserved` is the one predicate of what these kernels cannot serve and `refusal_text` the one place that words
it: every module's `refusal` is a row of `REFUSALS`.  `PairKernel` is the opening every kernel's class shares: it owns the
device-side constants of one env object (link lists, columns) - torch tensors on the torch path, plain HIP allocations on the NumPy
path - and states once the out= predicate (`fits`, `all_fit`), the owned result tuple (`declare_outputs`, `outputs`) and the leading
launch arguments (`launch_args`).  `RbSensor` derives from it and launches the sensing kernel on device pointers.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _native
from .path_loss_table import NATIVE

WHAT = {'sinr_db': _native.SENSE_SINR_DB, 'interference_mw': _native.SENSE_INTERFERENCE_MW}


def fold_columns(budget: dict, law: dict, link_tx: np.ndarray) -> Tuple[np.ndarray, int, int]:
    """(cols float32 [6, D], law id, pow_k) of d2d_sense_rb from link_budget_columns() and PathLoss.power_law_columns()."""
    a_tx, a_rx, expo = (np.asarray(law[k], dtype=np.float64) for k in ('a_tx_db', 'a_rx_db', 'exponent'))
    d = len(a_tx)
    cols = np.zeros((6, d), dtype=np.float32)
    with np.errstate(over='ignore'):
        cols[0] = 10.0 ** ((np.asarray(budget['eirp_off_db'], dtype=np.float64) - a_tx) / 10.0)
        cols[1] = 10.0 ** (-a_rx / 10.0)
        cols[2] = 10.0 ** (np.asarray(budget['rx_off_db'], dtype=np.float64) / 10.0)
        cols[3] = 10.0 ** (np.asarray(budget['noise_dbm'], dtype=np.float64) / 10.0)
    if not ((cols[:4] >= 1.0e-30) & (cols[:4] <= 1.0e30)).all():
        raise ValueError('a link-budget constant is outside the float32 linear range 1e-30 .. 1e30 (a term beyond +-300 dB)')
    if (expo == 2.0).all():
        return cols, _native.SENSE_LAW_INV_SQUARE, 0
    # every link transmitter's exponent within 1/2 of one integer k in 1 .. 8: (d^2)^(-k/2) by reciprocals times (d^2)^phi
    tx_expo = expo[np.asarray(link_tx, dtype=np.int64)]
    k0 = int(np.floor(tx_expo[0] + 0.5)) if len(tx_expo) else 0        # lround: half away from zero for the positive exponents here
    for k in (k0, k0 + 1, k0 - 1):
        if 1 <= k <= 8 and len(tx_expo) and (np.abs(tx_expo - k) <= 0.5).all():
            cols[4] = -0.5 * (expo - k)
            return cols, _native.SENSE_LAW_POW_K, k
    # the general split: -exponent / 2 as a head with 12 leading mantissa bits and the rest of the double as the tail
    hd = -0.5 * expo
    head = (hd.astype(np.float32).view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)
    cols[4] = head
    cols[5] = hd - head.astype(np.float64)
    return cols, _native.SENSE_LAW_POWER, 0


def fold_capacity_columns(budget: dict) -> np.ndarray:
    """cap_cols float32 [2, D] of d2d_marginal_capacity from link_budget_columns(): bw_mhz (1e-6 * Hz, in double, rounded once) and
    sens_db."""
    bw = np.asarray(budget['bw_hz'], dtype=np.float64)
    cols = np.zeros((2, len(bw)), dtype=np.float32)
    cols[0] = 1e-6 * bw
    cols[1] = np.asarray(budget['sens_dbm'], dtype=np.float64)
    return cols


def unserved(sim, export_actions: bool) -> Optional[Tuple[str, str]]:
    """What about this env the stateless pair kernels (sensing, the neighbour graph) cannot serve, as (kind, detail), or None:
    'export_actions', 'route' (detail: the route's name), 'shadowing', 'pinned'.  The one predicate behind every refusal text."""
    if not export_actions:
        return 'export_actions', ''
    route = sim.path_loss_table.route
    if route != NATIVE:
        return 'route', route
    if sim.path_loss_table.law.get('shadowing'):
        return 'shadowing', ''
    mask, xy = sim.fixed_positions()
    if mask.any() and (xy != xy.astype(np.float32)).any():
        return 'pinned', ''
    return None


# What differs between the APIs' refusal texts, by API: (subject, what it does with the decoded planes that export_actions=False
# does not write, what cannot evaluate a table route, what a fresh shadowing draw per evaluation does not have, which of its
# results are device tensors - None where the API has a NumPy path).  A new family adds its row here.
_READS = 'reads the decoded (rb, tx power) planes, which export_actions=False does not write'
_UNITS = 'works in the units of the decoded (rb, tx power) planes and reads them for the {}, and export_actions=False does not write them'
_PAIRS = 'its kernel can evaluate for the pairs no step reads'
_OTHER_RB = 'counterfactual (what another RB would have given is another draw)'
_OTHER_ASSIGNMENT = 'counterfactual (what another assignment would have given is another draw)'
REFUSALS = {
    'sense': ('sense()', _READS, 'the sensing kernel can evaluate for the pairs no step reads', _OTHER_RB, None),
    'graph': ('the neighbour graph',
              'feeds an observation that gathers the decoded (rb, tx power) planes, which export_actions=False does not write',
              'its kernels can evaluate', 'strongest interferer that holds between resets', None),
    'marginal_capacity': ('marginal_capacity()', _READS, "its kernel can evaluate from the transmitter's side",
                          'counterfactual (the step without one link would be another draw)', None),
    'best_rb': ('best_rb()', _READS, _PAIRS, _OTHER_RB, 'planes'),
    'power_control': ('power_control()', _READS, 'its kernel can evaluate for the powers no step has applied',
                      'fixed point (the SINR a power was solved for is another draw than the one the next step sees)', 'planes'),
    'best_response_dynamics': ('best_response_dynamics()', _READS, 'its kernel can evaluate for the RBs no step has applied',
                               'best response (the SINR a move was made for is another draw than the one the next link sees)',
                               'planes'),
    'evaluate': ('evaluate()', _UNITS.format('links on fixed actions'), _PAIRS, _OTHER_ASSIGNMENT, 'planes'),
    'assign_rbs': ('assign_rbs()', _UNITS.format('background links'), _PAIRS, _OTHER_ASSIGNMENT, 'planes'),
    'color_rbs': ('color_rbs()', _READS, 'coupling() can evaluate for the pairs no step reads',
                  'conflict graph (the pair a colour was chosen for is another draw than the one the next step sees)',
                  'graph and planes'),
}
REFUSALS['assign_rbs_power'] = ('assign_rbs_power()', *REFUSALS['assign_rbs'][1:])      # assign_rbs()'s reasons under its own name
REFUSALS['balance_sinr'] = ('balance_sinr()', _READS, 'its kernel can evaluate for the powers no step has applied',
                            'balanced level (the SINR a probe was solved for is another draw than the one the next step sees)', 'planes')


def refusal_text(api, sim, export_actions: bool, use_torch: Optional[bool] = None) -> Optional[str]:
    """Why this env cannot have `api`, a key of REFUSALS or a row of its form that a module keeps itself (None: it can).  Each text
    names the route or the switch; use_torch is passed by the APIs that have the torch path only."""
    subject, planes, law, draw, tensors = REFUSALS[api] if isinstance(api, str) else api
    if use_torch is not None and not use_torch:
        return f'{subject} needs the torch path (use_torch): its {tensors} are device tensors'
    why = unserved(sim, export_actions)
    if why is None:
        return None
    kind, route = why
    if kind == 'export_actions':
        return f'{subject} {planes}: build the env with export_actions=True'
    if kind == 'route':
        return f"{subject} does not serve the '{route}' path-loss route (a table, not a law {law}); it serves the native power-law models"
    if kind == 'shadowing':
        return f'{subject} does not serve ShadowingPathLoss: a fresh draw per evaluation has no {draw}'
    return (f'{subject} does not serve pinned device_config coordinates that float32 cannot hold: their low parts live inside the '
            'handle (float64 positions)')


def refusal(sim, export_actions: bool) -> Optional[str]:
    """Why this env cannot be sensed (None: it can)."""
    return refusal_text('sense', sim, export_actions)


def r16(x: int) -> int:
    """x rounded up to a multiple of 16, as the kernels lay out their LDS (round16 of csrc/d2d_same_rb.h): for the lds_bytes
    functions."""
    return (x + 15) & ~15


class _HipMemory:
    """The few HIP runtime calls the NumPy path needs for memory of its own (the torch path allocates through torch)."""

    def __init__(self) -> None:
        self.hip = C.CDLL('libamdhip64.so')
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.blocks = []

    def _ok(self, rc: int, what: str) -> None:
        if rc != 0:
            raise _native.NativeError(rc, f'{what} failed (hipError_t {rc})')

    def alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._ok(self.hip.hipMalloc(C.byref(p), max(int(nbytes), 4)), 'hipMalloc')
        self.blocks.append(p.value)
        return p.value

    def upload(self, array: np.ndarray) -> int:
        a = np.ascontiguousarray(array)
        p = self.alloc(a.nbytes)
        self._ok(self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1), 'hipMemcpy')          # hipMemcpyHostToDevice; synchronous
        return p

    def download(self, ptr: int, out: np.ndarray) -> None:
        self._ok(self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2), 'hipMemcpy')    # hipMemcpyDeviceToHost; synchronous

    def free(self, ptr: int) -> None:
        self.blocks.remove(ptr)
        self._ok(self.hip.hipFree(ptr), 'hipFree')

    def close(self) -> None:
        for p in list(self.blocks):
            self.free(p)


class PairKernel:
    """What the class of every stateless pair kernel opens with, bound to one env object: the env's shape (b, d, n and, with an RB
    cap, r), the link lists and the folded columns, uploaded once - tx, rx, cols[, cap_cols] tensors on the torch path, plain HIP
    allocations of `mem` on the NumPy path (torch None) - and their device pointers in `ptrs`, in the kernels' argument order."""

    def __init__(self, sim, num_links: int, torch, device, *, api: Optional[str] = None, max_rbs: Optional[int] = None,
                 capacity: bool = False) -> None:
        from .device import link_budget_columns
        self.sim, self.torch, self.device = sim, torch, device
        self.b, self.d, self.n = sim.num_envs, sim.handle.num_devices, int(num_links)
        if max_rbs is not None:
            self.r = int(sim.config.num_rbs)
            if self.r > max_rbs:
                raise ValueError(f'{api}() serves at most {max_rbs} RBs (num_rbs = {self.r})')
        tx, rx = np.asarray(sim.link_tx, dtype=np.int32), np.asarray(sim.link_rx, dtype=np.int32)
        if len(tx) != self.n or tx.min() < 0 or tx.max() >= self.d or rx.min() < 0 or rx.max() >= self.d:
            raise ValueError('the link list does not match the env')
        budget = link_budget_columns(sim._dev_list)
        cols, self.law, self.pow_k = fold_columns(budget, sim.path_loss_table.law, tx)
        host = {'tx': tx, 'rx': rx, 'cols': cols, **({'cap_cols': fold_capacity_columns(budget)} if capacity else {})}
        if torch is not None:
            for name, a in host.items():
                setattr(self, name, torch.as_tensor(a, device=device))
            self.ptrs = tuple(getattr(self, name).data_ptr() for name in host)
        else:
            self.mem = _HipMemory()
            self.ptrs = tuple(self.mem.upload(a) for a in host.values())
        self._subset = None                          # (key, tensor) of the last agent_subset(): a repeated mask is not uploaded again
        self._agent_dev = None                       # self.agent on the device, for an agent_subset() that is given a tensor

    def env_mask(self, env_mask):
        """None, or `env_mask` (bool / uint8 [B], tensor or array) as a contiguous uint8 tensor on the device."""
        torch = self.torch
        if env_mask is None:
            return None
        m = env_mask if torch.is_tensor(env_mask) else torch.as_tensor(np.asarray(env_mask))
        if tuple(m.shape) != (self.b,) or m.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'env_mask must be bool or uint8 [{self.b}] or None')
        return m.to(device=self.device, dtype=torch.uint8).contiguous()

    def agent_subset(self, subset, name: str):
        """uint8 [N] on the device: the links of `self.agent` (None), or those of them `subset` (bool [N], array or tensor) marks;
        `name` is what a refusal calls the argument.  A tensor is never read on the host: it is refused by its metadata and
        `subset & agent` is formed on the device, a fresh tensor per call, on the current stream (nothing is synchronised).  A host
        array is uploaded when it differs from the last one - a synchronous copy - and a repeat comes from the cache."""
        torch = self.torch
        if torch.is_tensor(subset):
            if tuple(subset.shape) != (self.n,) or subset.dtype != torch.bool:
                raise ValueError(f'{name} must be bool [{self.n}] (link) or None')
            if self._agent_dev is None:              # uploaded once, by the first call that passes a tensor
                self._agent_dev = torch.as_tensor(self.agent, device=self.device)
            return (subset.to(self.device) & self._agent_dev).to(torch.uint8)
        if subset is None:
            host = self.agent
        else:
            host = np.asarray(subset)
            if host.shape != (self.n,) or host.dtype != np.bool_:
                raise ValueError(f'{name} must be bool [{self.n}] (link) or None')
            host = host & self.agent
        key = host.tobytes()
        if self._subset is None or self._subset[0] != key:
            self._subset = (key, torch.as_tensor(host.astype(np.uint8), device=self.device))
        return self._subset[1]

    # ------------------------------------------------------------------ out=, the owned results and the launch prefix, stated once
    def fits(self, o, shape, dtype) -> bool:
        """Is `o` a contiguous tensor of this shape and dtype on the env's device?  The single-tensor form of the out= predicate."""
        return self.torch.is_tensor(o) and tuple(o.shape) == tuple(shape) and o.dtype == dtype and o.is_contiguous() \
            and o.device == self.device

    def all_fit(self, out, shapes, dtypes) -> bool:
        """The out= predicate: is `out` a tuple or list of len(shapes) tensors, each of which fits() its slot and no two of which
        share memory?  What is no sequence is refused before anything is asked of its entries."""
        return isinstance(out, (tuple, list)) and len(out) == len(shapes) \
            and all(self.fits(o, s, dt) for o, s, dt in zip(out, shapes, dtypes)) and len({o.data_ptr() for o in out}) == len(shapes)

    def declare_outputs(self, names, shapes, dtypes, message: Optional[str] = None) -> None:
        """What a class with a fixed result tuple states once, in __init__: the slots of outputs() and what its refusal says -
        `message`, or the shared format made from the declaration."""
        self.out_shapes, self.out_dtypes = tuple(shapes), tuple(dtypes)
        kinds = [f'{str(dt).replace("torch.", "")} {list(s)}' for s, dt in zip(shapes, dtypes)]
        self.out_message = message or (f'out must be ({", ".join(names)}): contiguous {", ".join(kinds[:-1])} and {kinds[-1]} tensors '
                                       f'on {self.device} that do not share memory')
        self.own = None                              # the result tuple this object owns, allocated by the first call without out=

    def outputs(self, out) -> tuple:
        """The declared result tuple: the one this object owns (None), or `out` if it passes all_fit(), else ValueError."""
        if out is None:
            if self.own is None:
                self.own = tuple(self.torch.empty(s, dtype=dt, device=self.device) for s, dt in zip(self.out_shapes, self.out_dtypes))
            return self.own
        if not self.all_fit(out, self.out_shapes, self.out_dtypes):
            raise ValueError(self.out_message)
        return tuple(out)

    def raw_launch_args(self, pos_x: int, pos_y: int, rb: int, pwr: int) -> tuple:
        """The arguments every kernel that reads the four planes begins with, from their device pointers."""
        return (pos_x, pos_y, rb, pwr, *self.ptrs, self.law, self.pow_k, self.b, self.d, self.n, self.r)

    def launch_args(self, t: dict) -> tuple:
        """raw_launch_args of the planes dict `t` of the torch path."""
        return self.raw_launch_args(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), t['rb'].data_ptr(), t['pwr'].data_ptr())

    def close(self) -> None:
        if self.torch is None:
            self.mem.close()


class RbSensor(PairKernel):
    """The sensing kernel bound to one env object: constants uploaded once, one launch per call."""

    def __init__(self, sim, num_links: int, torch=None, device=None) -> None:
        super().__init__(sim, num_links, torch, device, api='sense', max_rbs=_native.SENSE_MAX_RBS)
        self.own = None                              # the result block this object owns, allocated by the first call without out=

    def sense_torch(self, t: dict, what: int, out, stream: int):
        torch = self.torch
        shape = (self.b, self.n, self.r)
        if out is None:
            if self.own is None:
                self.own = torch.empty(shape, dtype=torch.float32, device=self.device)
            out = self.own
        elif not self.fits(out, shape, torch.float32):
            raise ValueError(f'out must be a contiguous float32 tensor {list(shape)} on {self.device}')
        _native.sense_rb(*self.launch_args(t), what, out.data_ptr(), stream)
        return out

    def sense_numpy(self, what: int, out):
        h = self.sim.handle
        shape = (self.b, self.n, self.r)
        if out is not None and (not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != np.float32
                                or not out.flags.c_contiguous):
            raise ValueError(f'out must be a C-contiguous float32 ndarray {list(shape)}')
        h.synchronize()                               # the planes are the last step's; the kernel runs on the null stream
        planes = [h.get_buffer(w)[0] for w in (_native.BUF_POS_X, _native.BUF_POS_Y, _native.BUF_RB, _native.BUF_PWR)]
        if self.own is None:
            self.own = self.mem.alloc(self.b * self.n * self.r * 4)
        _native.sense_rb(*self.raw_launch_args(*planes), what, self.own, 0)
        res = out if out is not None else np.empty(shape, dtype=np.float32)
        self.mem.download(self.own, res)              # synchronous on the null stream: behind the kernel
        return res

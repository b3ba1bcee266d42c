"""PathLoss plugins (mirrors gym_d2d/path_loss.py) and their lowering to the HIP kernels.

Plugin contract (unchanged from the reference): a PathLoss class is passed in env_config['path_loss_model'],
is constructed with one positional argument (carrier_freq_GHz) and is callable as model(tx, rx) -> dB.

Lowering: every built-in model is a power law in distance,
    PL_dB(tx, rx) = a_tx[tx] + a_rx[rx] + 10 * n[tx] * log10(d_m),
so `power_law_columns(devices)` returns the three per-device float64 columns for d2d_set_path_loss_power_law()
and the kernel evaluates gain = 10^(-(a_tx+a_rx)/10) * d^-n in the linear domain (one v_rcp per pair when n == 2).
A user subclass that only defines __call__ is evaluated on the host once per episode into a [D,D] table
(`table_db`, d2d_set_path_loss_table) - legal because positions are static between resets (simulator.py:61-75).
For batches a per-object __call__ is B x N x N Python calls per reset (1.1e9 at 4096 x 512): `ArrayPathLoss` is the
array-native form of the same plugin - compute(view) -> pl_db[B,N,N] on whole arrays (torch CUDA tensors in a batch, NumPy
for a single pair), handed to the library from device memory (d2d_set_path_loss_link_table_dev).  An ArrayPathLoss with
`per_step = True` is evaluated before EVERY step instead (a stochastic model: shadowing, fading), into a table the step kernel
reads in place (D2D_PL_TABLE_LIVE); its view carries the step counter and the built-in shadowing's normal stream.
`SpatialChannelPathLoss` is the native stochastic channel: a power-law median, spatially correlated shadowing and block fading,
filled into the same live table by a HIP kernel of its own before every step (include/d2d_channel.h).
"""
from __future__ import annotations

import math
import random
import warnings
from abc import ABC, abstractmethod
from enum import Enum
from random import gauss
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from .device import Device

SPEED_OF_LIGHT = 299792458  # m/s


class PathLoss(ABC):
    def __init__(self, carrier_freq_GHz: float) -> None:
        self.carrier_freq_GHz = float(carrier_freq_GHz)

    @abstractmethod
    def __call__(self, tx: Device, rx: Device) -> float:
        """Path loss in dB from `tx` to `rx`."""

    # ---- lowering hooks -------------------------------------------------------------------------------
    def power_law_columns(self, devices: Sequence[Device]) -> Optional[Dict[str, np.ndarray]]:
        """Per-device columns {'a_tx_db', 'a_rx_db', 'exponent'} if the model is a power law in distance,
        else None (the table route is used)."""
        return None

    def table_db(self, devices: Sequence[Device], tx_indices: Optional[Sequence[int]] = None,
                 rx_indices: Optional[Sequence[int]] = None) -> np.ndarray:
        """Host evaluation of the model: out[tx_index, rx_index] in dB (float64, as the plugin returns it).  Only the pairs
        (tx in tx_indices) x (rx in rx_indices) are evaluated - the transmitters and receivers of the links that act: the
        step reads PL(tx of link j, rx of link i) and nothing else (simulator.py:93,100,114), which at 256 CUE + 256 DUE
        pairs is 512 x 257 calls instead of 769 x 769.  None = every device.  Everything else stays NaN, as does a pair the
        model cannot evaluate (zero distance -> ValueError in math.log10); the env raises if such a pair is ever used,
        which is when the reference would have raised."""
        devs = list(devices)
        out = np.full((len(devs), len(devs)), np.nan, dtype=np.float64)
        txs = range(len(devs)) if tx_indices is None else sorted(set(int(i) for i in tx_indices))
        rxs = range(len(devs)) if rx_indices is None else sorted(set(int(j) for j in rx_indices))
        for i in txs:
            tx = devs[i]
            for j in rxs:
                if i == j:
                    continue
                try:
                    out[i, j] = self(tx, devs[j])
                except (ValueError, ZeroDivisionError):
                    pass
        return out


class PathLossView:
    """What ArrayPathLoss.compute sees: the transmitter and receiver coordinates of the links that act, as arrays, plus the
    Device objects for their static attributes.

        xp                    the array module: torch (batch on the GPU) or numpy (a single pair, or no torch)
        tx_x, tx_y            [B, N]  transmitter of link j            rx_x, rx_y   [B, N]  receiver of link i
        tx_devices, rx_devices   length-N lists of Device (antenna gains, heights, ... - the attributes device.py:85-173 exposes)
        distance()            [B, N, N] float64   d[b, j, i] = |tx of link j - rx of link i| (position.py:11-12)
        tx_column(fn) / rx_column(fn)   fn(device) per transmitter / receiver as an array shaped [1, N, 1] / [1, 1, N]
        step                  steps enqueued since the model was installed (the reset's initial step included; not reset between
                              episodes) - the counter the built-in ShadowingPathLoss draws by
        first_env             global index of the view's env 0 (the env offset of a sharded run plus the chunk start)
        seed                  the model's seed: env_config['seed'], else (per_step) one random.getrandbits(63) at construction, as
                              ShadowingPathLoss's (a once-per-reset model without a seed takes one from the OS)
        normal(kind=0)        standard normals, float64: kind 0 [B, N, N] by (tx link j, rx link i), kind 1 [B, N] (the SNR's
                              own-link draws) - on the GPU the built-in ShadowingPathLoss's stream exactly (Box-Muller of
                              Philox4x32-10, counter (first_env + b, step, j | i << 16, kind), key seed: libd2d_plugin.so), so
                              pl + chi * where(d > d0, view.normal(), 0) draws what the built-in model draws; a single-pair NumPy
                              view draws fresh values from NumPy's global generator

    pl_db[b, j, i] = PathLoss(tx of link j, rx of link i): j == i is the link's own signal path (simulator.py:93,114), j != i
    an interferer's (simulator.py:97-101) - the pairs d2d_set_path_loss_link_table names."""

    def __init__(self, xp, tx_x, tx_y, rx_x, rx_y, tx_devices, rx_devices, like=None, *, step: int = 0, first_env: int = 0,
                 seed: int = 0, columns: Optional[dict] = None):
        self.xp = xp
        self.tx_x, self.tx_y, self.rx_x, self.rx_y = tx_x, tx_y, rx_x, rx_y
        self.tx_devices, self.rx_devices = list(tx_devices), list(rx_devices)
        self._like = like if like is not None else tx_x
        self.step, self.first_env, self.seed = int(step), int(first_env), int(seed)
        self._columns = columns if columns is not None else {}     # uploaded columns by value: the caller's, kept from view to view

    def normal(self, kind: int = 0):
        b, n = tuple(self.tx_x.shape)
        if kind not in (0, 1):
            raise ValueError('kind must be 0 (tx link j, rx link i) or 1 (own link i, the SNR)')
        shape = (b, n, n) if kind == 0 else (b, n)
        if self.xp.__name__ != 'torch':
            return np.random.standard_normal(shape)
        from . import _native
        dev = self._like.device
        out = self.xp.empty(shape, dtype=self.xp.float64, device=dev)
        if out.numel():
            with self.xp.cuda.device(dev):
                stream = self.xp.cuda.current_stream(dev).cuda_stream
                _native.plugin_normal(out.data_ptr(), _native.F64, b, self.first_env, n if kind == 0 else 1, n, self.step, kind,
                                      self.seed, stream)
        return out

    def _f64(self, a):
        return a.double() if self.xp.__name__ == 'torch' else np.asarray(a, dtype=np.float64)

    def distance(self):
        dx = self._f64(self.tx_x)[:, :, None] - self._f64(self.rx_x)[:, None, :]       # float32 coordinates subtract exactly in float64
        dy = self._f64(self.tx_y)[:, :, None] - self._f64(self.rx_y)[:, None, :]
        return self.xp.sqrt(dx * dx + dy * dy)

    def _column(self, devices, fn, shape):
        vals = np.array([float(fn(d)) for d in devices], dtype=np.float64).reshape(shape)
        if self.xp.__name__ == 'torch':
            # a column is uploaded (a synchronous copy) when its values are new; a repeat is a device-side copy of the kept one,
            # so that a per-step model's evaluation stays enqueue-only and the caller still gets a tensor of its own
            key = (vals.tobytes(), vals.shape, str(self._like.device))
            if key not in self._columns:
                if len(self._columns) >= 64:         # a model whose columns change from step to step: keep the dict bounded
                    self._columns.clear()
                self._columns[key] =self.xp.as_tensor(vals, device=self._like.device)
            return self._columns[key].clone()
        return vals

    def tx_column(self, fn):
        return self._column(self.tx_devices, fn, (1, -1, 1))

    def rx_column(self, fn):
        return self._column(self.rx_devices, fn, (1, 1, -1))


class ArrayPathLoss(PathLoss):
    """Array-native PathLoss plugin (the batched counterpart of path_loss.py:12-25, as ArrayObsFunction is of ObsFunction):
    subclasses define compute(view) -> pl_db [B, N, N] with the array module `view.xp`.  The per-object call the reference's
    contract asks for (`model(tx, rx) -> dB`) is derived from it - one pair through the same compute - so the single-env D2DEnv
    and a batch run the same formula:

        class TwoSlope(ArrayPathLoss):
            def compute(self, view):
                d = view.distance()
                near = 20 * view.xp.log10(d) + 38.0
                far = 35 * view.xp.log10(d) - 15 * math.log10(50.0) + 38.0
                return view.xp.where(d <= 50.0, near, far) - view.tx_column(lambda t: t.tx_antenna_gain_dBi)

    A batch evaluates it once per reset on the GPU (torch) and hands the result to the library from device memory
    (d2d_set_path_loss_link_table_dev): no host table, no Python loop.

    per_step = True: a stochastic model (the reference calls its PathLoss on every step, path_loss.py:12-25, simulator.py:93,
    97-101,114).  compute(view) then runs before every step - VecD2DEnv, Simulator.step_arrays and the single-env D2DEnv, the
    step inside reset() included - into a [B, N+1, N] float64 table the step kernel reads in place (D2D_PL_TABLE_LIVE); torch
    with a GPU is required.  compute may return pl_db or (pl_db, snr_pl_db[B, N]): the SNR's own evaluation of the signal
    path (simulator.py:114 calls the model again: an independent draw for a stochastic model); omitted, the diagonal of pl_db.

    env_chunk: compute runs on env slices of this many envs, each written into the table as it comes (None: as many as keep one
    [b, N, N] float64 temporary within about 1 GiB); the results do not depend on it."""

    per_step: bool = False
    env_chunk: Optional[int] = None

    @abstractmethod
    def compute(self, view: PathLossView):
        """pl_db[b, j, i] in dB for the transmitter of link j and the receiver of link i, shape [B, N, N]."""

    def __call__(self, tx: Device, rx: Device) -> float:
        one = lambda v: np.array([[float(v)]], dtype=np.float64)
        view = PathLossView(np, one(tx.position.x), one(tx.position.y), one(rx.position.x), one(rx.position.y), [tx], [rx])
        out = np.asarray(self.compute(view), dtype=np.float64).reshape(-1)
        if out.size != 1 or not np.isfinite(out[0]):
            raise ValueError('math domain error')          # what math.log10(0) raises in a per-object model (path_loss.py:66)
        return float(out[0])


def is_deterministic(model: Callable, tx: Device, rx: Device) -> bool:
    """Two calls of a per-object model on one pair give the same value (NaN == NaN; a pair it refuses counts as the same).
    Python's and NumPy's global random states are put back, so checking consumes no draw the model would otherwise see."""
    py_state, np_state = random.getstate(), np.random.get_state()
    try:
        vals = []
        for _ in range(2):
            try:
                vals.append(float(model(tx, rx)))
            except (ValueError, ZeroDivisionError):
                vals.append(None)
    finally:
        random.setstate(py_state)
        np.random.set_state(np_state)
    a, b = vals
    if a is None or b is None:
        return a is b
    return a == b or (math.isnan(a) and math.isnan(b))


def warn_if_stochastic(model: Callable, tx: Device, rx: Device) -> bool:
    """UserWarning when a per-object PathLoss gives two values for one pair: its table is evaluated once per reset, so every
    draw would stay frozen for the episode.  Returns whether it warned."""
    if is_deterministic(model, tx, rx):
        return False
    warnings.warn(f'{type(model).__name__} returned two different path losses for one (tx, rx) pair: a per-object PathLoss is '
                  'evaluated once per reset and its draws stay frozen for the whole episode.  Write it as an ArrayPathLoss with '
                  'per_step = True to have it evaluated on every step.', UserWarning, stacklevel=3)
    return True


def pl_constant_dB(carrier_freq_GHz: float, ple: float) -> float:
    """Distance-independent part of the log-distance model: 10 n log10(f_Hz) + 10 n log10(4 pi / c)."""
    scale = 10 * ple
    return scale * math.log10(carrier_freq_GHz * 1e9) + scale * math.log10((4 * math.pi) / SPEED_OF_LIGHT)


class LogDistancePathLoss(PathLoss):
    """PL = 10 n log10(d) + 10 n log10(f) + 10 n log10(4 pi / c)   (path_loss.py:42-66)."""

    def __init__(self, carrier_freq_GHz: float, ple=2.0) -> None:
        super().__init__(carrier_freq_GHz)
        self.ple = float(ple)   # 2.0 = free space, ~3.5 = cluttered
        self.pl_constant_dB = pl_constant_dB(carrier_freq_GHz, ple)

    def _log_distance_path_loss(self, dist_m: float) -> float:
        return 10 * self.ple * math.log10(dist_m) + self.pl_constant_dB

    def __call__(self, tx: Device, rx: Device) -> float:
        return self._log_distance_path_loss(tx.position.distance(rx.position))

    def power_law_columns(self, devices):
        if type(self).__call__ not in (LogDistancePathLoss.__call__, getattr(ShadowingPathLoss, '__call__', None)):
            return None     # a subclass changed the formula: evaluate it on the host instead
        n = len(devices)
        return {'a_tx_db': np.full(n, self.pl_constant_dB), 'a_rx_db': np.zeros(n), 'exponent': np.full(n, self.ple)}


class FreeSpacePathLoss(LogDistancePathLoss):
    """Free-space (Friis) loss = log-distance with exponent 2 (the reference's own comment, path_loss.py:45).
    Not present in the reference snapshot; named by BASELINE.json config 4."""

    def __init__(self, carrier_freq_GHz: float) -> None:
        super().__init__(carrier_freq_GHz, ple=2.0)


class ShadowingPathLoss(LogDistancePathLoss):
    """Log-distance with log-normal shadowing beyond a close-in distance (path_loss.py:69-81).  A fresh Gaussian
    is drawn on every call, so this model cannot be frozen into a table."""

    def __init__(self, carrier_freq_GHz: float, ple=2.0, d0_m=100.0, chi_dB=2.7) -> None:
        super().__init__(carrier_freq_GHz, ple)
        self.d0_m = float(d0_m)
        self.chi_dB = float(chi_dB)

    def __call__(self, tx: Device, rx: Device) -> float:
        d = tx.position.distance(rx.position)
        if d <= self.d0_m:
            return self._log_distance_path_loss(d)
        anchor = self._log_distance_path_loss(self.d0_m)
        return anchor + 10 * self.ple * math.log10(d / self.d0_m) + gauss(0, self.chi_dB)

    def power_law_columns(self, devices):
        if type(self).__call__ is not ShadowingPathLoss.__call__:
            return None
        cols = LogDistancePathLoss.power_law_columns(self, devices) if \
            type(self)._log_distance_path_loss is LogDistancePathLoss._log_distance_path_loss else None
        if cols is not None:
            # LD(d0) + 10 n log10(d/d0) == LD(d): the deterministic part is the plain log-distance law; the kernel
            # adds the per-evaluation Gaussian beyond d0 (csrc/d2d_step.hip, PL_SHADOW)
            cols['shadowing'] = {'d0_m': self.d0_m, 'chi_dB': self.chi_dB}
        return cols


_UNSET = object()
_U64 = (1 << 64) - 1
SHADOW_SEED_MIX = 0x736861646F77696E     # 'shadowin': the three streams of one seed (mobility.SEED_MIX is the third) never coincide
FADING_SEED_MIX = 0x666164696E676368     # 'fadingch'


class SpatialChannelPathLoss(PathLoss):
    """A spatially consistent stochastic channel, evaluated on the GPU before every step (csrc/d2d_channel.hip, one fill of the live
    dB table the step kernel reads; include/d2d_channel.h states the model completely, counters included):

        pl_db[b, j, i] = M(u, v) + S(p_u, p_v) + F(u, v)        u the transmitter DEVICE of link j, v the receiver device of link i

    M: the median - any model that is a power law in distance (power_law_columns: LogDistancePathLoss with any exponent,
       FreeSpacePathLoss, CostHataPathLoss), built as median(carrier_freq_GHz, **median_kwargs).
    S: log-normal shadowing of standard deviation shadow_std_dB, a sum of num_sinusoids (8, 16 or 32) plane waves over the joint
       (transmitter position, receiver position) space, redrawn per (env, episode) and never per step, with
       E[S S'] = shadow_std_dB^2 exp(-(|dp_u| + |dp_v|) / decorrelation_m): a pair that stands still keeps its shadow, two receivers
       a metre apart see nearly the same one, and with mobility= the shadow changes only as far as the devices move.
       shadow_std_dB = 0: no shadowing work is launched.
    F: block fading -10 log10 |h|^2, independent per step and per DEVICE pair: 'rayleigh' (|h|^2 ~ Exp(1)), 'rician' with
       K = 10^(rician_k_dB / 10), or None.  Keyed by device pair, not link pair: every link the base station receives sees one
       channel from a given transmitter.

    The SNR's own evaluation of the signal path (row N of the live table, simulator.py:114) is the diagonal entry: the SAME physical
    channel, not a second draw - unlike the built-in ShadowingPathLoss, which follows the reference in drawing again for the SNR.

    table_dtype: 'float64' (default) or 'float32', the live table's entries.  A float32 entry above 128 dB (COST-Hata urban at a few
    hundred metres) has an ulp of 1.5e-5 dB, so storing it alone costs up to 7.6e-6 dB - most of the project's 1e-5 bar where a step's
    sinr_db is near 0 dB; float64 entries keep the step within the bar at twice the table's bytes (8.6 GB at 4096 x 512).

    Stateless: a pure function of (seed, global env index, episode, step in the episode, device positions), so autoreset, sharding
    and mobility= reproduce the lockstep single-GPU values bit for bit.  seed None: the env's seed; the shadowing and fading keys
    are that seed XOR two constants of their own.  VecD2DEnv on the torch path only: the model needs the env's episode clock, and
    it is a field over an env - it has no value for one isolated pair, so the per-object call raises NotImplementedError.

    Reference plugin construction: one positional carrier_freq_GHz; everything else by keyword or as subclass attributes."""

    median = LogDistancePathLoss
    median_kwargs: Optional[dict] = None
    shadow_std_dB = 8.0
    decorrelation_m = 20.0
    num_sinusoids = 16
    fading: Optional[str] = 'rayleigh'
    rician_k_dB = 6.0
    seed: Optional[int] = None
    table_dtype = 'float64'

    def __init__(self, carrier_freq_GHz: float, median=_UNSET, median_kwargs=_UNSET, shadow_std_dB=_UNSET, decorrelation_m=_UNSET,
                 num_sinusoids=_UNSET, fading=_UNSET, rician_k_dB=_UNSET, seed=_UNSET, table_dtype=_UNSET) -> None:
        super().__init__(carrier_freq_GHz)
        for name, v in (('median', median), ('median_kwargs', median_kwargs), ('shadow_std_dB', shadow_std_dB),
                        ('decorrelation_m', decorrelation_m), ('num_sinusoids', num_sinusoids), ('fading', fading),
                        ('rician_k_dB', rician_k_dB), ('seed', seed), ('table_dtype', table_dtype)):
            if v is not _UNSET:
                setattr(self, name, v)
        for name in ('shadow_std_dB', 'decorrelation_m', 'rician_k_dB'):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f'{name} must be a finite number, got {v!r}')
            setattr(self, name, float(v))
        if self.shadow_std_dB < 0:
            raise ValueError(f'shadow_std_dB must be >= 0, got {self.shadow_std_dB!r}')
        if self.decorrelation_m <= 0:
            raise ValueError(f'decorrelation_m must be > 0, got {self.decorrelation_m!r}')
        if isinstance(self.num_sinusoids, bool) or self.num_sinusoids not in (8, 16, 32):
            raise ValueError(f'num_sinusoids must be 8, 16 or 32, got {self.num_sinusoids!r}')
        self.num_sinusoids = int(self.num_sinusoids)
        if self.fading not in ('rayleigh', 'rician', None):
            raise ValueError(f"fading must be 'rayleigh', 'rician' or None, got {self.fading!r}")
        if self.table_dtype not in ('float32', 'float64'):
            raise ValueError(f"table_dtype must be 'float32' or 'float64', got {self.table_dtype!r}")
        s = self.seed
        if s is not None and (isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) <= _U64):
            raise ValueError(f'seed must be None or an int in [0, 2^64), got {s!r}')
        self.seed = None if s is None else int(s)
        if not (isinstance(self.median, type) and issubclass(self.median, PathLoss)) or issubclass(self.median, SpatialChannelPathLoss):
            raise ValueError(f'median must be a PathLoss class that is a power law in distance, got {self.median!r}')
        self.median_model = self.median(carrier_freq_GHz, **dict(self.median_kwargs or {}))

    def __call__(self, tx: Device, rx: Device) -> float:
        raise NotImplementedError('SpatialChannelPathLoss is a field over an env (its shadowing is a function of every position of the '
                                  'env, its draws are keyed by env, episode and step): it has no value for one isolated (tx, rx) pair. '
                                  'Use it as the path_loss_model of a VecD2DEnv')

    def median_columns(self, devices: Sequence[Device]) -> Dict[str, np.ndarray]:
        """The median's power-law columns, or ValueError: a median the fill kernel cannot evaluate per pair."""
        cols = self.median_model.power_law_columns(devices)
        if cols is None:
            raise ValueError(f'SpatialChannelPathLoss: median={type(self.median_model).__name__} is not a power law in distance '
                             '(its power_law_columns is None); the median must be LogDistancePathLoss, FreeSpacePathLoss, '
                             'CostHataPathLoss or another model with columns')
        if 'shadowing' in cols:
            raise ValueError(f'SpatialChannelPathLoss: median={type(self.median_model).__name__} draws a shadowing of its own per '
                             'evaluation; the median must be deterministic (shadow_std_dB is this model\'s shadowing)')
        return cols

    def constants(self):
        """(num_sinusoids or 0, shadow_amp_db, wave_scale, fading id, rician_mu, rician_s) as the kernel takes them: formed in
        double, the float32 ones rounded once."""
        m = self.num_sinusoids if self.shadow_std_dB > 0 else 0
        amp = float(np.float32(self.shadow_std_dB * math.sqrt(2.0 / self.num_sinusoids)))
        k = 10.0 ** (self.rician_k_dB / 10.0)
        mu, s = float(np.float32(math.sqrt(k / (k + 1.0)))), float(np.float32(math.sqrt(1.0 / (2.0 * (k + 1.0)))))
        return m, amp, 1.0 / (2.0 * math.pi * self.decorrelation_m), {None: 0, 'rayleigh': 1, 'rician': 2}[self.fading], mu, s

    def stream_seeds(self, env_seed: int):
        """(shadowing key, fading key) for an env seeded env_seed."""
        base = self.seed if self.seed is not None else int(env_seed)
        return (base ^ SHADOW_SEED_MIX) & _U64, (base ^ FADING_SEED_MIX) & _U64


class AreaType(Enum):
    RURAL = 0
    SUBURBAN = 1
    URBAN = 2


class CostHataPathLoss(PathLoss):
    """COST-231 Hata (path_loss.py:90-123):
       L = 46.3 + 33.9 log10(f_MHz) - 13.82 log10(h_tx) - a(h_rx) + (44.9 - 6.55 log10(h_tx)) log10(d_km) + C."""

    def __init__(self, carrier_freq_GHz: float, area_type=AreaType.SUBURBAN) -> None:
        super().__init__(carrier_freq_GHz)
        self.area_type: AreaType = area_type

    def _ms_h_correction(self, f: float, h_rx: float) -> float:
        """Mobile-station antenna height correction a(h_rx) for carrier f in MHz."""
        if self.area_type != AreaType.URBAN:
            return (1.1 * math.log10(f) - 0.7) * h_rx - (1.56 * math.log10(f) - 0.8)
        if f >= 200:
            return 8.29 * math.log10(1.54 * h_rx) ** 2 - 1.1
        return 3.2 * math.log10(11.75 * h_rx) ** 2 - 4.97

    def _slope(self, h_tx: float) -> float:
        return 44.9 - 6.55 * math.log10(h_tx)

    def __call__(self, tx: Device, rx: Device) -> float:
        f = self.carrier_freq_GHz * 1000
        d_km = tx.position.distance(rx.position) / 1000
        h_tx, h_rx = tx.antenna_height_m, rx.antenna_height_m
        metro = 3 if self.area_type == AreaType.URBAN else 0
        return (46.3 + 33.9 * math.log10(f) - 13.82 * math.log10(h_tx) - self._ms_h_correction(f, h_rx)
                + self._slope(h_tx) * math.log10(d_km) + metro)

    def power_law_columns(self, devices):
        if type(self).__call__ is not CostHataPathLoss.__call__:
            return None
        f = self.carrier_freq_GHz * 1000
        metro = 3 if self.area_type == AreaType.URBAN else 0
        a_tx, a_rx, expo = [], [], []
        for dev in devices:
            h = dev.antenna_height_m
            slope = self._slope(h)
            # log10(d_km) = log10(d_m) - 3: fold the -3*slope into the tx constant
            a_tx.append(46.3 + 33.9 * math.log10(f) - 13.82 * math.log10(h) + metro - 3.0 * slope)
            a_rx.append(-self._ms_h_correction(f, h))
            expo.append(slope / 10.0)
        return {'a_tx_db': np.array(a_tx), 'a_rx_db': np.array(a_rx), 'exponent': np.array(expo)}

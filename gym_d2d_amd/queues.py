"""Packet traffic: the host side of libd2d_queue.so (include/d2d_queue.h, csrc/d2d_queue.hip).

`PacketTraffic` is the model a user hands to VecD2DEnv(traffic=...): every link has an on/off source that, while on, receives a
Poisson number of packets per step; packets wait in a finite buffer (tail drop), are served oldest first by what the step's
capacity_mbps carries in dt_s seconds, and expire deadline_steps steps after they arrived.  `Queues` owns the planes and the deadline
ring of one env object and launches the kernel on torch's tensors.  The model is all integers - bits and steps - so the kernel, the
NumPy restatement of the tests and a sharded run agree bit for bit.

Simplification: a link whose buffer is empty still transmits and interferes in the step kernel, which has no off state; the queue only
decides how many of the bits the link could carry were there to be carried.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

from . import _native

SEED_MIX = 0x7061636B65747321            # 'packets!': keeps the default stream apart from mobility's and the channel's for the same seed
MAX_RATE = 16.0                          # packets per step: the Poisson mass beyond the table's 64 entries stays far below 2^-32
PLANES = ('arrived_bits', 'served_bits', 'expired_bits', 'overflow_bits', 'backlog_bits', 'hol_age_steps', 'mean_delay_steps', 'on')
_U32, _U64 = (1 << 32) - 1, (1 << 64) - 1


def _threshold(p: float) -> int:
    """min(2^32 - 1, floor(p * 2^32)): a draw word below it happens with probability p."""
    return min(_U32, int(math.floor(p * 4294967296.0)))


def _number(name, v) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f'{name} must be a finite number, got {v!r}')


def _integer(name, v) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f'{name} must be an int, got {v!r}')


class PacketTraffic:
    """packets_per_step: the Poisson mean of an ON link's arrivals per step, (cue, due) or one number for both, each in [0, 16];
    packet_bits: the size of every packet; deadline_steps: D in [1, 32] - a packet that has not been served within D steps of its
    arrival expires; buffer_bits: what a link's buffer holds (None: 64 packets; whole packets are admitted while the backlog stays
    within it, the rest of a burst drops); dt_s: seconds per env step - a link carries capacity_mbps * 1e6 * dt_s bits per step;
    p_on_to_off, p_off_to_on: the per-step switching probabilities of the on/off source (p_on_to_off = 0: always on);
    seed: the traffic stream's own seed (None: the env's seed, mixed with a constant of its own)."""

    def __init__(self, packets_per_step=1.0, packet_bits: int = 12000, deadline_steps: int = 8, buffer_bits: Optional[int] = None,
                 dt_s: float = 1e-3, p_on_to_off: float = 0.0, p_off_to_on: float = 1.0, seed: Optional[int] = None) -> None:
        rates = packets_per_step if isinstance(packets_per_step, (tuple, list)) else (packets_per_step, packets_per_step)
        if len(rates) != 2:
            raise ValueError(f'packets_per_step must be a number or a (cue, due) pair, got {packets_per_step!r}')
        for r in rates:
            _number('packets_per_step', r)
            if not 0 <= r <= MAX_RATE:
                raise ValueError(f'packets_per_step must be in [0, {MAX_RATE:g}], got {r!r}')
        _integer('packet_bits', packet_bits)
        if not 1 <= packet_bits or packet_bits * _native.QUEUE_TABLE >= 1 << 31:
            raise ValueError(f'packet_bits must be >= 1 with 64 * packet_bits below 2^31, got {packet_bits!r}')
        _integer('deadline_steps', deadline_steps)
        if not 1 <= deadline_steps <= _native.QUEUE_MAX_DEADLINE:
            raise ValueError(f'deadline_steps must be in [1, {_native.QUEUE_MAX_DEADLINE}], got {deadline_steps!r}')
        if buffer_bits is None:
            buffer_bits = min(_native.QUEUE_TABLE * int(packet_bits), (1 << 31) - 1)
        _integer('buffer_bits', buffer_bits)
        if not 0 <= buffer_bits < 1 << 31:
            raise ValueError(f'buffer_bits must be in [0, 2^31), got {buffer_bits!r}')
        _number('dt_s', dt_s)
        if dt_s <= 0:
            raise ValueError(f'dt_s must be > 0, got {dt_s!r}')
        for name, p in (('p_on_to_off', p_on_to_off), ('p_off_to_on', p_off_to_on)):
            _number(name, p)
            if not 0 <= p <= 1:
                raise ValueError(f'{name} must be in [0, 1], got {p!r}')
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _U64):
            raise ValueError(f'seed must be None or an int in [0, 2^64), got {seed!r}')
        self.packets_per_step = (float(rates[0]), float(rates[1]))
        self.packet_bits, self.deadline_steps, self.buffer_bits = int(packet_bits), int(deadline_steps), int(buffer_bits)
        self.dt_s, self.p_on_to_off, self.p_off_to_on = float(dt_s), float(p_on_to_off), float(p_off_to_on)
        self.seed = None if seed is None else int(seed)

    @property
    def bits_per_mbps_step(self) -> float:
        """What 1 Mbps carries in one step, the double the kernel multiplies capacity_mbps by."""
        return 1e6 * self.dt_s

    @property
    def on_share(self) -> float:
        """The stationary probability of the ON state."""
        if self.p_on_to_off == 0.0:
            return 1.0
        return self.p_off_to_on / (self.p_on_to_off + self.p_off_to_on)

    def thresholds(self) -> np.ndarray:
        """uint32 [2, 64]: the Poisson CDFs of the CUE and the DUE links scaled to 2^32, T_k = min(2^32 - 1, floor(c_k 2^32)) with
        c_k the running sum of p_0 = exp(-lambda), p_k = p_{k-1} lambda / k in float64.  An ON link receives as many packets as its
        table has entries <= the draw word."""
        tab = np.empty((2, _native.QUEUE_TABLE), dtype=np.uint32)
        for c, lam in enumerate(self.packets_per_step):
            p = math.exp(-lam)
            acc = 0.0
            for k in range(_native.QUEUE_TABLE):
                if k:
                    p = p * lam / k
                acc += p
                tab[c, k] = _threshold(acc)
        return tab

    def switch_thresholds(self) -> Tuple[int, int, int]:
        """(p_on_to_off, p_off_to_on, p_start_on) as the kernel compares draw words against them."""
        return _threshold(self.p_on_to_off), _threshold(self.p_off_to_on), _threshold(self.on_share)

    def stream_seed(self, env_seed: int) -> int:
        """The Philox key of the draws for an env seeded env_seed."""
        return self.seed if self.seed is not None else (int(env_seed) ^ SEED_MIX) & _U64

    def __repr__(self) -> str:
        return (f'PacketTraffic(packets_per_step={self.packets_per_step}, packet_bits={self.packet_bits}, '
                f'deadline_steps={self.deadline_steps}, buffer_bits={self.buffer_bits}, dt_s={self.dt_s}, '
                f'p_on_to_off={self.p_on_to_off}, p_off_to_on={self.p_off_to_on}, seed={self.seed})')


def refusal(use_torch: bool) -> Optional[str]:
    """Why this env cannot have packet traffic (None: it can).  It reads capacity_mbps only: every path-loss route serves it."""
    if not use_torch:
        return ("traffic= needs the torch path (use_torch): the queue planes and the deadline ring are device tensors and the "
                "queue step runs on torch's stream - the NumPy path has no such hook")
    return None


class Queues:
    """The queue kernel bound to one env object: the eight planes [B, N], the ring [D, B, N] and the constants; one launch per call."""

    def __init__(self, model: PacketTraffic, num_envs: int, num_cues: int, num_due_pairs: int, torch, device, first_env: int,
                 per_env: bool) -> None:
        if not isinstance(model, PacketTraffic):
            raise TypeError(f'traffic must be a PacketTraffic or None, got {type(model).__name__}')
        _native.load_queue_library()                 # a missing library is an error here, not inside the first step
        self.model, self.first_env = model, int(first_env)
        self.b, self.cues, self.pairs = int(num_envs), int(num_cues), int(num_due_pairs)
        n = self.cues + self.pairs
        self.tables = model.thresholds()
        self.switches = model.switch_thresholds()
        for name in PLANES:
            dtype = torch.float32 if name == 'mean_delay_steps' else torch.uint8 if name == 'on' else torch.int32
            setattr(self, name, torch.zeros((self.b, n), dtype=dtype, device=device))
        self.ring = torch.zeros((model.deadline_steps, self.b, n), dtype=torch.int32, device=device)
        # the per-env clock (autoreset): what `elapsed` was when an env's queues were started
        self.start = torch.zeros(self.b, dtype=torch.int32, device=device) if per_env else None

    def planes(self) -> SimpleNamespace:
        """The planes as a namespace (the env's own tensors, updated in place by every step), plus the ring."""
        return SimpleNamespace(**{name: getattr(self, name) for name in PLANES}, ring=self.ring)

    def _launch(self, capacity, env_seed: int, stream: int, **clock) -> None:
        m = self.model
        _native.queue_step(capacity.data_ptr(), self.ring.data_ptr(), *(getattr(self, name).data_ptr() for name in PLANES), self.tables,
                           self.b, self.cues, self.pairs, m.deadline_steps, m.packet_bits, m.buffer_bits, m.bits_per_mbps_step,
                           *self.switches, self.first_env, m.stream_seed(env_seed), stream_ptr=stream, **clock)

    def start_episode(self, t: dict, env_seed: int, episode: int, stream: int) -> None:
        """Every env's start of episode `episode`: cleared rings, zero planes, the on/off states drawn (behind the reset's step)."""
        self._launch(t['capacity_mbps'], env_seed, stream, step=0, episode=episode)
        if self.start is not None:
            self.start.copy_(t['elapsed'])

    def step(self, t: dict, env_seed: int, step: int, episode: int, stream: int) -> None:
        """Lockstep: step `step` (1, 2, ...) of episode `episode`, behind the step kernel that wrote capacity_mbps."""
        self._launch(t['capacity_mbps'], env_seed, stream, step=step, episode=episode)

    def step_per_env(self, t: dict, env_seed: int, stream: int) -> None:
        """Autoreset: pending envs start their next episode, every other env steps by its own clock (before episode_advance)."""
        self._launch(t['capacity_mbps'], env_seed, stream, elapsed_ptr=t['elapsed'].data_ptr(), start_ptr=self.start.data_ptr(),
                     episode_ptr=t['episode'].data_ptr(), reset_ptr=t['pending'].data_ptr())

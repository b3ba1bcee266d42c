"""Device mobility: the host side of libd2d_mobility.so (include/d2d_mobility.h, csrc/d2d_mobility.hip).

`GaussMarkovMobility` is the model a user hands to VecD2DEnv(mobility=...): every device has a velocity that follows a first-order
Gauss-Markov process, v <- a v + sigma sqrt(1 - a^2) n, and moves by v dt before every step, held inside the cell by a hard wall and, a
DUE receiver, within d2d_radius of its transmitter.  `Mobility` owns the velocity planes and the device-side constants of one env
object and launches the kernel on torch's tensors.  What a device-side change of positions inside step() cannot serve is decided by
path_loss_table.positions_move_unserved, the predicate autoreset's refusals go through too; `refusal` puts mobility's texts on it.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from . import _native
from .path_loss_table import positions_move_unserved

SEED_MIX = 0x6D6F62696C697479            # 'mobility': keeps the default stream apart from the shadowing model's for the same seed
_U64 = (1 << 64) - 1


class GaussMarkovMobility:
    """speed_std_mps: the standard deviation sigma of each velocity component, m/s (stationary: every step's velocities have it);
    memory: the correlation a of a velocity with itself one step earlier, in [0, 1) - 0 is a fresh velocity every step, towards 1 a
    straight line; dt_s: seconds of movement per env step; seed: the mobility stream's own seed (None: the env's seed, mixed with a
    constant so that the stream is not the shadowing model's)."""

    def __init__(self, speed_std_mps: float = 1.5, memory: float = 0.75, dt_s: float = 1.0, seed: Optional[int] = None) -> None:
        for name, v in (('speed_std_mps', speed_std_mps), ('memory', memory), ('dt_s', dt_s)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f'{name} must be a finite number, got {v!r}')
        if speed_std_mps < 0:
            raise ValueError(f'speed_std_mps must be >= 0, got {speed_std_mps!r}')
        if not 0 <= memory < 1:
            raise ValueError(f'memory must be in [0, 1), got {memory!r}')
        if dt_s <= 0:
            raise ValueError(f'dt_s must be > 0, got {dt_s!r}')
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _U64):
            raise ValueError(f'seed must be None or an int in [0, 2^64), got {seed!r}')
        self.speed_std_mps, self.memory, self.dt_s = float(speed_std_mps), float(memory), float(dt_s)
        self.seed = None if seed is None else int(seed)

    def constants(self) -> Tuple[float, float, float, float]:
        """(a, s, sigma, dt) as the kernel takes them: formed in double, each rounded once to float32."""
        a, sigma = self.memory, self.speed_std_mps
        return tuple(float(np.float32(x)) for x in (a, sigma * math.sqrt(1.0 - a * a), sigma, self.dt_s))

    def stream_seed(self, env_seed: int) -> int:
        """The Philox key of the draws for an env seeded env_seed."""
        return self.seed if self.seed is not None else (int(env_seed) ^ SEED_MIX) & _U64

    def __repr__(self) -> str:
        return (f'GaussMarkovMobility(speed_std_mps={self.speed_std_mps}, memory={self.memory}, dt_s={self.dt_s}, '
                f'seed={self.seed})')


def refusal(sim, use_torch: bool) -> Optional[str]:
    """Why this env cannot have mobility (None: it can).  Each text names the switch or the route."""
    why = positions_move_unserved(sim, use_torch)
    if why is None:
        return None
    kind, route = why
    return {
        'numpy': 'mobility= needs the torch path (use_torch): the velocity planes are device tensors and the move runs on '
                 "torch's stream",
        'route': f"mobility= cannot serve the '{route}' path-loss route: its table is evaluated once per reset, and devices that "
                 'move before every step would need the host to evaluate it again (use a per-step ArrayPathLoss or a native model)',
        'pinned': 'mobility= cannot pin device_config coordinates that float32 cannot hold: d2d_positions_changed drops their low '
                  'parts after the first move',
    }[kind]


class Mobility:
    """The move kernel bound to one env object: the velocity planes, the fixed mask and the constants; one launch per call."""

    def __init__(self, model: GaussMarkovMobility, sim, torch, device, first_env: int, per_env: bool) -> None:
        if not isinstance(model, GaussMarkovMobility):
            raise TypeError(f'mobility must be a GaussMarkovMobility or None, got {type(model).__name__}')
        _native.load_mobility_library()              # a missing library is an error here, not inside the first step
        cfg, h = sim.config, sim.handle
        self.model, self.first_env = model, int(first_env)
        self.b, self.cues, self.pairs = sim.num_envs, int(cfg.num_cues), int(cfg.num_due_pairs)
        self.consts = model.constants()
        self.radii = (float(np.float32(cfg.cell_radius_m)), float(np.float32(cfg.d2d_radius_m)))
        self.vel_x = torch.zeros((self.b, h.num_devices), dtype=torch.float32, device=device)
        self.vel_y = torch.zeros_like(self.vel_x)
        mask, _ = sim.fixed_positions()
        self.fixed = torch.as_tensor(mask.astype(np.uint8), device=device) if mask.any() else None
        # the per-env clock (autoreset): what `elapsed` was when an env's velocities were drawn
        self.start = torch.zeros(self.b, dtype=torch.int32, device=device) if per_env else None

    def _launch(self, t: dict, env_seed: int, stream: int, **clock) -> None:
        _native.mobility_move(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), self.vel_x.data_ptr(), self.vel_y.data_ptr(),
                              0 if self.fixed is None else self.fixed.data_ptr(), self.b, self.cues, self.pairs, self.first_env,
                              self.model.stream_seed(env_seed), *self.consts, *self.radii, stream_ptr=stream, **clock)

    def start_episode(self, t: dict, env_seed: int, episode: int, stream: int) -> None:
        """Every env's start-of-episode velocities at `episode` (after the reset sampler; positions are not touched)."""
        self._launch(t, env_seed, stream, step=0, episode=episode)
        if self.start is not None:
            self.start.copy_(t['elapsed'])

    def move(self, t: dict, env_seed: int, step: int, episode: int, stream: int) -> None:
        """Lockstep: step `step` (1, 2, ...) of episode `episode`."""
        self._launch(t, env_seed, stream, step=step, episode=episode)

    def move_per_env(self, t: dict, env_seed: int, stream: int) -> None:
        """Autoreset: pending envs get their next episode's start-of-episode velocities, every other env moves by its own clock."""
        self._launch(t, env_seed, stream, elapsed_ptr=t['elapsed'].data_ptr(), start_ptr=self.start.data_ptr(),
                     episode_ptr=t['episode'].data_ptr(), reset_ptr=t['pending'].data_ptr())

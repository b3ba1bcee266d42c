"""The mobility model of include/d2d_mobility.h restated in float64 NumPy - the yardstick of test_gpu_mobility.py, checked on its own
by test_mobility_cpu.py.  Built on the oracle's Philox4x32-10 and the Box-Muller of ShadowSpec.normals (oracle/d2d_oracle.py), whose
counter (env, step, j | i << 16, kind) is read here as (global env index, episode, step in the episode, 2 device + axis)."""
import numpy as np

from oracle import d2d_oracle as orc

SEED_MIX = 0x6D6F62696C697479
NEAR_M = 1e-3                      # a wall or tether decision closer than this may legitimately fall differently in float32


def ulp32(x):
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(np.inf)) - x)


def stream_seed(env_seed, seed=None):
    return int(seed) if seed is not None else (int(env_seed) ^ SEED_MIX) & (2 ** 64 - 1)


def normals(seed, first_env, episode, t, num_envs, num_dev):
    """n[b, d, axis], float64: the draws of step t (0: the start-of-episode draw) of episode `episode`."""
    assert 0 <= t < 65536
    b = np.arange(num_envs)[:, None, None]
    kind = 2 * np.arange(num_dev)[None, :, None] + np.arange(2)[None, None, :]
    return orc.ShadowSpec(seed=seed, step=episode, first_env=first_env).normals(b, t, 0, kind)


def constants(speed_std_mps, memory, dt_s):
    """(a, s, sigma, dt): formed in double, each rounded once to float32 (and used here as those values, in double)."""
    return tuple(float(np.float32(x)) for x in (memory, speed_std_mps * np.sqrt(1.0 - memory * memory), speed_std_mps, dt_s))


class Restatement:
    """One batch of envs from the start of an episode on: pos [B, D, 2] (the reset's positions), fixed bool [D] (the base station
    is fixed whatever the mask says).  step() moves once; `near` [B, D] marks the devices whose wall or tether decision came within
    NEAR_M at this step or an earlier one.

    tether_target None: the model as stated - a tethered device is pulled onto the circle of d2d_radius.  A radius: the kernel's
    float32 rule (include/d2d_mobility.h) - pulled onto that radius (d2d_radius - ulp32(cell_radius)) where it stands outside
    d2d_radius, and tested and pulled once more, velocity untouched, where the wall moved it."""

    def __init__(self, pos, num_cues, num_due_pairs, fixed=None, *, speed_std_mps=1.5, memory=0.75, dt_s=1.0, seed=0, first_env=0,
                 episode=0, cell_radius=500.0, d2d_radius=20.0, tether_target=None):
        self.pos = np.array(pos, dtype=np.float64)
        self.b, self.d = self.pos.shape[:2]
        assert self.d == 1 + num_cues + 2 * num_due_pairs
        self.fixed = np.zeros(self.d, dtype=bool) if fixed is None else np.array(fixed, dtype=bool)
        self.fixed[0] = True
        self.a, self.s, self.sigma, self.dt = constants(speed_std_mps, memory, dt_s)
        self.seed, self.first_env, self.episode = seed, first_env, episode
        self.cell_radius, self.d2d_radius = float(np.float32(cell_radius)), float(np.float32(d2d_radius))
        self.tether_target = None if tether_target is None else float(tether_target)
        self.tx = 1 + num_cues + 2 * np.arange(num_due_pairs)
        self.rx = self.tx + 1
        self.t = 0
        self.vel = self.sigma * normals(seed, first_env, episode, 0, self.b, self.d)
        self.vel[:, self.fixed] = 0.0
        self.near = np.zeros((self.b, self.d), dtype=bool)
        self.hits = {'wall': 0, 'tether': 0}

    def _pull(self, who, centre, radius, what, only=None):
        """Devices `who` onto the circle around `centre` [B, len(who), 2] where they stand further than `radius` from it; velocity
        negated.  only [B, len(who)] bool: the kernel's second test of the tether - those devices alone, velocity untouched."""
        off = self.pos[:, who] - centre
        dist = np.hypot(off[..., 0], off[..., 1])
        hit = dist > radius
        if only is None:
            self.near[:, who] |= np.abs(dist - radius) < NEAR_M
            self.hits[what] += int(hit.sum())
        else:
            hit &= only
        onto = self.tether_target if what == 'tether' and self.tether_target is not None else radius
        scale = np.where(hit, onto / np.where(hit, dist, 1.0), 1.0)
        self.pos[:, who] = np.where(hit[..., None], centre + off * scale[..., None], self.pos[:, who])
        if only is None:
            self.vel[:, who] = np.where(hit[..., None], -self.vel[:, who], self.vel[:, who])
        return hit

    def _tether_and_wall(self, who, anchor):
        self._pull(who, self.pos[:, anchor], self.d2d_radius, 'tether')
        wall = self._pull(who, np.zeros(2), self.cell_radius, 'wall')
        if self.tether_target is not None:
            self._pull(who, self.pos[:, anchor], self.d2d_radius, 'tether', only=wall)

    def step(self):
        self.t += 1
        n = normals(self.seed, self.first_env, self.episode, self.t, self.b, self.d)
        mv = ~self.fixed
        self.vel[:, mv] = self.a * self.vel[:, mv] + self.s * n[:, mv]
        self.pos[:, mv] += self.vel[:, mv] * self.dt
        origin = np.zeros(2)
        # everything but the receivers first: a transmitter whose receiver is pinned is tethered to it
        back = self.tx[mv[self.tx] & self.fixed[self.rx]]
        if len(back):
            self._tether_and_wall(back, back + 1)
        first = np.flatnonzero(mv & ~np.isin(np.arange(self.d), self.rx) & ~np.isin(np.arange(self.d), back))
        self._pull(first, origin, self.cell_radius, 'wall')
        # the receivers, against their transmitters' new positions, then the wall
        rx = self.rx[mv[self.rx]]
        if len(rx):
            self._tether_and_wall(rx, rx - 1)
        return self.pos, self.vel

    def radius(self):
        return np.hypot(self.pos[..., 0], self.pos[..., 1])

    def pair_distance(self):
        off = self.pos[:, self.rx] - self.pos[:, self.tx]
        return np.hypot(off[..., 0], off[..., 1])

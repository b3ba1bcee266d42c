"""What the reset tests share (test_reset_cpu.py, test_gpu_reset_direct.py): a float64 restatement of include/d2d_hip.h's
d2d_reset_positions (csrc/d2d_reset.hip: reset_kernel, reset_masked_kernel), the host's division estimate in plain integers, and the
case tables, each entry with the path it forces.  Built on oracle.d2d_oracle.reset_uniforms and philox4x32_10 (whose Random123 known
answers test_host_logic.py checks); nothing is imported from the package.

The restatement is vectorised over envs and tries and states the kernel's contract for the one case oracle.sample_positions_from_uniforms
refuses: a receiver whose 64 tries all fall outside the cell takes its transmitter's coordinates exactly (`exhausted`).

The position bar is the project's own (test_gpu_reset.py, tools/fuzz_reset.py): |got - ref| <= BAR * cell_radius per coordinate, BAR =
2e-6.  By the code the kernel's error is about 3e-7 of the radius it scales (one rounding of f * pi/2, two polynomials under 1 ulp, sqrtf,
one product, one sum).  An ACCEPTED receiver lies inside the cell and so does its transmitter, so its offset is at most 2 cell radii long
whatever d2d_radius_m is: 6e-7 from the offset, 3e-7 from the transmitter, 6e-8 from the sum - about 1e-6 of the cell radius at the worst,
3e-7 where d2d_radius_m is small against the cell.

`ambiguous` marks a receiver for which some try, up to and including the accepted one, lies within W = BAR * cell_radius of the cell edge:
float32 may decide such a try the other way.  (A try that float64 rejects at distance rho from the origin has an offset no longer than
rho + cell_radius, so near the edge its float32 error is the 1e-6 above, under W.)  AMBIGUOUS_CAP: at most 0.1 % of a case's receivers."""
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from oracle import d2d_oracle as orc

SEED, EPISODE, FIRST_ENV = 12345, 7, 1000
TRIES = 64                                  # reset_args: max_tries
BAR = 2e-6                                  # of the cell radius, per coordinate; the ambiguity width W is the same figure
AMBIGUOUS_CAP = 1e-3
INSIDE_TOL = 1e-6                           # tools/fuzz_reset.py: |p| <= cell (1 + 1e-6)
PAIR_TOL = (1e-5, 2.4e-7)                   # tools/fuzz_reset.py: |tx - rx| <= d2d (1 + 1e-5) + 2.4e-7 cell

# name: B, CUEs, DUE pairs, cell_radius_m, d2d_radius_m | gids the multiply-high leaves one short | the path it forces
# Unstated: seed SEED, episode EPISODE, first_env FIRST_ENV, no pins.
CASES = {
    'default': dict(b=64, cues=6, pairs=9, cell=500.0, d2d=20.0, corrected=0,
                    why='16 units: the division estimate is never short; the baseline'),
    'units_3': dict(b=5, cues=2, pairs=0, cell=500.0, d2d=20.0, corrected=4, why='3 units, no DUE: 4 of 15 gids take the ++b correction'),
    'one_pair': dict(b=6, cues=0, pairs=1, cell=500.0, d2d=20.0, corrected=0, why='no CUE, one pair: 2 units, an exact reciprocal'),
    'wave_plus_one': dict(b=7, cues=0, pairs=64, cell=500.0, d2d=20.0, corrected=6,
                          why="65 units, 129 devices, 64 links: the masked kernel's second trip has one lane"),
    'wide': dict(b=5, cues=70, pairs=100, cell=500.0, d2d=20.0, corrected=4,
                 why='171 units, 271 devices, 170 links: three trips of every masked loop'),
    'big_d2d': dict(b=33, cues=3, pairs=40, cell=50.0, d2d=60.0, corrected=32,
                    why='d2d radius above the cell radius: about half of the receivers redraw, up to a dozen tries'),
    'late': dict(b=9, cues=0, pairs=130, cell=10.0, d2d=80.0, corrected=8,
                 why='most receivers reach try 16 or later and more than a third exhaust all 64'),
    'exhaust': dict(b=3, cues=1, pairs=66, cell=1.0, d2d=1000.0, corrected=2, why='every receiver exhausts: rx = tx'),
    'first_env_wrap': dict(b=8, cues=6, pairs=9, cell=500.0, d2d=20.0, corrected=0, first_env=2 ** 32 - 3,
                           why='first_env + b wraps in the Philox counter: envs 3..7 take the counters 0..4'),
    'pinned': dict(b=7, cues=0, pairs=64, cell=500.0, d2d=20.0, corrected=6,
                   pins={0: (12.5, -3.25), 11: (495.0, 0.0), 42: (-100.5, 200.25), 81: (300.0, -300.0), 82: (310.5, -295.25)},
                   why='a transmitter alone (on the cell edge: its receiver redraws), a receiver alone, a whole pair, and device 0'),
    'pinned_cues': dict(b=64, cues=6, pairs=9, cell=500.0, d2d=20.0, corrected=0,
                        pins={0: (1.0, 1.0), 3: (-250.0, 125.5), 7: (0.0, -498.0), 10: (64.0, 32.0)},
                        why='a CUE, the first transmitter (its receiver redraws) and a receiver alone, with CUEs in front'),
}
FULL = tuple(CASES)
MASKED_SHAPES = ('wave_plus_one', 'wide', 'big_d2d')
MASKED_B = (1, 5, 7, 9)
PENDING_WORDS = (1, -1, 7)


def spec(name):
    s = dict(first_env=FIRST_ENV, episode=EPISODE, pins=None)
    s.update(CASES[name])
    s['d'] = 1 + s['cues'] + 2 * s['pairs']
    s['units'] = 1 + s['cues'] + s['pairs']
    s['links'] = s['cues'] + s['pairs']
    return s


class Reset(NamedTuple):
    pos: np.ndarray            # float64 [B, D, 2]
    tries: np.ndarray          # int64 [B, D]: 0 base station and pinned devices, 1 CUEs and transmitters, 1..64 receivers
    exhausted: np.ndarray      # bool [B, D]: all 64 tries rejected - the receiver has its transmitter's coordinates exactly
    ambiguous: np.ndarray      # bool [B, D]: a try up to the accepted one within W of the cell edge


def uniforms(seed, episode, b, d, tries=TRIES, first_env=0):
    """[B, D, T, 2] uniforms of the reset at one episode (oracle.reset_uniforms) or at a per-env [B] episode vector (the same map of
    the same Philox words, the episode word per env)."""
    ep = np.asarray(episode)
    if ep.ndim == 0:
        return orc.reset_uniforms(int(seed), int(episode), b, d, tries, first_env=first_env)
    assert ep.shape == (b,)
    env = (np.arange(b, dtype=np.uint64) + np.uint64(first_env))[:, None, None]
    w = orc.philox4x32_10(env, np.arange(d, dtype=np.uint64)[None, :, None], np.arange(tries, dtype=np.uint64)[None, None, :],
                          ep.astype(np.uint64)[:, None, None], int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    scale = 2.0 ** -24
    return np.stack([(w[0] >> np.uint32(8)) * scale, ((w[1] >> np.uint32(8)) + 0.5) * scale], axis=-1)


def restate(seed, episode, b, cues, pairs, cell, d2d, first_env=0, pins=None):
    """d2d_reset_positions in float64: the base station at the origin, CUEs and transmitters at try 0 in the cell disc, every receiver
    at its first try within d2d of its transmitter that is not outside the cell - and on its transmitter when 64 tries are not enough.
    `pins` {device: (x, y)}: a pinned device holds its coordinates, a pinned receiver skips the loop, a pin on device 0 is ignored."""
    d = 1 + cues + 2 * pairs
    u = uniforms(seed, episode, b, d, TRIES, first_env)
    theta = 2 * np.pi * u[..., 0]
    pos = np.zeros((b, d, 2))
    tries = np.zeros((b, d), dtype=np.int64)
    exhausted = np.zeros((b, d), dtype=bool)
    ambiguous = np.zeros((b, d), dtype=bool)
    free = np.array(list(range(1, 1 + cues)) + list(range(1 + cues, d, 2)), dtype=np.int64)
    if free.size:
        r = cell * np.sqrt(u[:, free, 0, 1])
        pos[:, free, 0] = r * np.cos(theta[:, free, 0]); pos[:, free, 1] = r * np.sin(theta[:, free, 0])
        tries[:, free] = 1
    pins = {int(k): v for k, v in (pins or {}).items() if int(k) != 0}
    for k, xy in pins.items():
        pos[:, k] = xy; tries[:, k] = 0
    if pairs:
        kt = np.arange(1 + cues, d, 2); kr = kt + 1
        r = d2d * np.sqrt(u[..., 1][:, kr, :])                                  # [B, P, T]
        x = pos[:, kt, 0][:, :, None] + r * np.cos(theta[:, kr, :])
        y = pos[:, kt, 1][:, :, None] + r * np.sin(theta[:, kr, :])
        inside = ~(x ** 2 + y ** 2 > cell ** 2)
        hit, first = inside.any(axis=2), inside.argmax(axis=2)
        used = np.where(hit, first + 1, TRIES)
        at = lambda a: np.take_along_axis(a, first[..., None], axis=2)[..., 0]
        near = np.abs(np.hypot(x, y) - cell) <= BAR * cell
        seen = np.arange(TRIES)[None, None, :] < used[..., None]
        drawn = np.array([int(k) not in pins for k in kr])
        kd = kr[drawn]
        pos[:, kd, 0] = np.where(hit, at(x), pos[:, kt, 0])[:, drawn]
        pos[:, kd, 1] = np.where(hit, at(y), pos[:, kt, 1])[:, drawn]
        tries[:, kd] = used[:, drawn]
        exhausted[:, kd] = ~hit[:, drawn]
        ambiguous[:, kd] = (near & seen).any(axis=2)[:, drawn]
    return Reset(pos, tries, exhausted, ambiguous)


@lru_cache(maxsize=None)
def reference(name):
    """The restatement of a full-reset case, computed once per process and left unchanged."""
    s = spec(name)
    ref = restate(SEED, s['episode'], s['b'], s['cues'], s['pairs'], s['cell'], s['d2d'], s['first_env'], s['pins'])
    for a in ref:
        a.setflags(write=False)
    return ref


def receivers(cues, d):
    return np.arange(2 + cues, d, 2)


def mask_xy(pins, d):
    """What d2d_reset_positions is given for `pins`: fixed_mask uint8 [D] (the bit of device 0 included) and fixed_xy float32 [D, 2]."""
    mask, xy = np.zeros(d, dtype=np.uint8), np.zeros((d, 2), dtype=np.float32)
    for k, p in pins.items():
        mask[k] = 1; xy[k] = p
    assert all(tuple(float(v) for v in xy[k]) == tuple(float(v) for v in p) for k, p in pins.items())      # float32-exact
    return mask, xy


def division(b, units):
    """The host's division estimate (reset_args) and the kernel's use of it, in plain integers: units_magic, and for every gid of
    the launch the estimate of gid // units, whether it is one short, and (b, u) after the kernel's correction."""
    magic = 0xFFFFFFFF if units == 1 else (1 << 32) // units
    gid = [g for g in range(b * units)]
    est = [(g * magic) >> 32 for g in gid]
    rem = [g - e * units for g, e in zip(gid, est)]
    short = [r >= units for r in rem]
    env = [e + 1 if s else e for e, s in zip(est, short)]
    unit = [r - units if s else r for r, s in zip(rem, short)]
    return magic, est, short, env, unit


# ---- the masked reset's inputs
def pending_and_episodes(b):
    """RESET_PENDING int32 [B]: about a third non-zero, words from PENDING_WORDS, the last env pending.  EPISODE uint32 [B]: distinct,
    2^32 - 1 on the last env (pending), 0 on env 1 (pending), and env 0 - not pending when B > 1 - at an episode of its own."""
    pending = np.zeros(b, dtype=np.int32)
    chosen = sorted({b - 1} | {k for k in range(b) if k % 3 == 1})
    for n, k in enumerate(chosen):
        pending[k] = PENDING_WORDS[n % 3]
    episode = np.array([2 ** 31, 0, 3, 1000003, 1, 2 ** 32 - 2, 77, 5, 9][:b], dtype=np.uint32)
    episode[b - 1] = 2 ** 32 - 1
    assert len(set(episode.tolist())) == b
    return pending, episode


def gather_rows(px, py, link_tx, link_rx):
    """BUF_LINK_POS as NumPy gathers it: float32 [B, N, 4] rows (tx_x, tx_y, rx_x, rx_y)."""
    return np.stack([px[:, link_tx], py[:, link_tx], px[:, link_rx], py[:, link_rx]], axis=-1)

"""What the direct-launch mobility tests share (test_element_direct_cpu.py, test_gpu_mobility_direct.py): the seeded cases of
mobility_move_kernel (csrc/d2d_mobility.hip) at the shapes VecD2DEnv never gives it, each with the path it forces, and their float64
restatement (mobility_util.Restatement), computed once per process and left unchanged.  Nothing is imported from the package.

Also the per-env clock's schedule (clock_schedule), which queue_direct_util shares: include/d2d_queue.h takes its clock from
include/d2d_mobility.h, and both clock cases feed the same sixteen envs.

The position bars, in ulp32(cell_radius) per step, counted as test_gpu_mobility.py counts (one ulp for every rounded operation that
acts on a coordinate of magnitude <= cell_radius):

    free device (CUE, transmitter)     4       the move's multiply-add, and one projection: square root, divide, multiply-add
    tethered receiver, small cell     14       the move's multiply-add; up to THREE projections (tether, wall, tether again) of three
                                               operations each: 10; and the circle's centre is its transmitter, which carries a free
                                               device's 4 - a pulled receiver stands at centre + r * direction, so its radial error
                                               is the centre's and its tangential error a convex mix of the centre's and its own:
                                               the two add, neither is amplified
    both, small cell                + dt * 1e-6 sigma (t + 1) / 2
                                               a velocity may be off by the velocity bar 1e-6 sigma k at step k, and the move
                                               carries dt times that into the position: the sum over k <= t, per step.  At a 500 m
                                               cell this term is 0.04 ulp per step and the existing bar leaves it out; at 40 m, where
                                               ulp32(cell_radius) is 3.8e-6 m and a velocity's own ulp is as wide, it is not small
                                               (a velocity 6e-7 sigma off, as test_gpu_mobility.py measures them, is 2.2 ulp)

The cases at cell_radius 500 m keep the bar of 4 for every device, receivers included, as test_gpu_mobility.py has it.

Beside the drawn cases stands one hand-laid state, CRAFTED['parted'] (parted_positions), for the second tether test after the wall:
no drawn case reaches a pair that only that test keeps together, and the float64 restatement cannot judge it, so it is judged by
pull_inside32, the kernel's projection operation by operation in float32, on the CPU, and by the invariants on the GPU."""
from functools import lru_cache

import numpy as np

import mobility_util as mob

SEED = 21
STEPS = 10
CELL, D2D = 500.0, 20.0
FAST = dict(speed_std_mps=9.0, memory=0.5, dt_s=1.5)
MAX_THREADS = 53287
LEFT_OUT_CAP = 0.01
TOL22 = 1.0 + 2.0 ** -22

# name: B, CUEs, DUE pairs | the path it forces.  Unstated: cell 500 m, d2d 20 m, the model FAST, first_env 4096, episode 3, steps 1 - 10
CASES = {
    'bs_only': dict(b=300, cues=0, pairs=0,
                    why='units = 1: the 0xFFFFFFFF reciprocal, every thread beyond 0 corrected; nothing moves, velocities are 0'),
    'one_pair': dict(b=1025, cues=0, pairs=1, why='units = 2 (exact reciprocal), n_cues == 0, 2050 threads over 9 workgroups'),
    'one_cue': dict(b=1025, cues=1, pairs=0, why='n_due_pairs == 0: no thread takes the pair branch, D = 2'),
    'wg_units': dict(b=9, cues=255, pairs=0, why='units = 256 = the workgroup: an env per workgroup exactly'),
    'odd': dict(b=67, cues=3, pairs=253, why='units 257, 17 219 threads: the last workgroup partly idle, envs straddle workgroups'),
    'small_cell': dict(b=67, cues=3, pairs=253, cell=40.0, small=True,
                       why='tethered receivers hit the wall all the time: the second tether test after the wall'),
    'many_envs': dict(b=4099, cues=5, pairs=7, cell=60.0, model=dict(speed_std_mps=6.0, memory=0.6, dt_s=1.0), small=True,
                      why='209 workgroups, a prime env count'),
    'masks': dict(b=33, cues=6, pairs=12, why='fixed_mask null, all zero, pinning one of each kind, all ones'),
    'counter_edge': dict(b=9, cues=6, pairs=7, first_env=2 ** 32 - 9, episode=2 ** 32 - 1, t0=65526,
                         why='the counter words at their ends: env 2^32 - 1, episode 2^32 - 1, step 65 535'),
    'clock': dict(b=16, cues=6, pairs=7, first_env=2 ** 32 - 16, why='the per-env clock: see clock_schedule'),
}
# masks: device 0, a CUE, a transmitter alone, a receiver alone, a whole pair (6 CUEs: transmitter k is device 7 + 2 k)
PINNED = (0, 3, 11, 18, 23, 24)
MASKS = ('null', 'zeros', 'pinned', 'ones')


# A state laid out by hand instead of drawn, for the one path no drawn case reaches (see parted_positions)
CRAFTED = {
    'parted': dict(b=67, cues=3, pairs=253, model=dict(speed_std_mps=0.0, memory=0.5, dt_s=1.0),
                   why="the wall's rounding parts a pair that stood inside its tether: the second tether test after the wall"),
}


def spec(name):
    s = dict(cell=CELL, d2d=D2D, model=FAST, first_env=4096, episode=3, t0=1, small=False)
    s.update(CASES[name] if name in CASES else CRAFTED[name])
    s['d'] = 1 + s['cues'] + 2 * s['pairs']
    s['units'] = 1 + s['cues'] + s['pairs']
    s['ts'] = list(range(s['t0'], s['t0'] + STEPS))
    return s


def fixed_mask(name, which='null'):
    """bool [D] as the restatement takes it (device 0 set), and what the kernel is given: None or uint8 [D]."""
    d = spec(name)['d']
    m = np.zeros(d, dtype=np.uint8)
    if which == 'pinned':
        m[list(PINNED)] = 1
    elif which == 'ones':
        m[:] = 1
    ref = m.astype(bool)
    ref[0] = True
    return ref, (None if which == 'null' else m)


def _disc(rng, shape, radius):
    r, phi = radius * np.sqrt(rng.random(shape)), 2 * np.pi * rng.random(shape)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=-1)


def layout(rng, b, cues, pairs, cell, d2d, bs_anywhere=False):
    """float32 [B, D, 2]: the base station at the origin, CUEs and transmitters uniform in the disc, every receiver uniform within
    d2d of its transmitter and inside the cell (redrawn until it is).  0.999 of both radii: the float32 rounding stays inside."""
    pos = np.zeros((b, 1 + cues + 2 * pairs, 2))
    if bs_anywhere:
        pos[:, 0] = _disc(rng, (b,), 0.999 * cell)
    pos[:, 1:1 + cues] = _disc(rng, (b, cues), 0.999 * cell)
    tx = _disc(rng, (b, pairs), 0.999 * cell)
    rx = tx + _disc(rng, (b, pairs), 0.999 * d2d)
    for _ in range(1000):
        bad = np.hypot(rx[..., 0], rx[..., 1]) > 0.999 * cell
        if not bad.any():
            break
        rx[bad] = tx[bad] + _disc(rng, (int(bad.sum()),), 0.999 * d2d)
    assert not bad.any()
    pos[:, 1 + cues::2], pos[:, 2 + cues::2] = tx, rx
    return pos.astype(np.float32)


@lru_cache(maxsize=None)
def start_positions(name):
    s = spec(name)
    rng = np.random.default_rng([SEED, sorted(CASES).index(name)])
    pos = layout(rng, s['b'], s['cues'], s['pairs'], s['cell'], s['d2d'], bs_anywhere=name == 'bs_only')
    pos.setflags(write=False)
    return pos


# ---------------------------------------------------------------------------------------------- the path only float32 has
def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def pull_inside32(p, c, limit, target):
    """pull_inside of csrc/d2d_mobility.hip operation by operation in float32 (a product of two float32 is exact in float64, so
    the multiply-adds round once but for a rare double rounding): (where p [..., 2] stands afterwards, which rows were pulled)."""
    limit, target = np.float32(limit), np.float32(target)
    dx, dy = p[..., 0] - c[..., 0], p[..., 1] - c[..., 1]
    d = np.sqrt(_fma32(dx, dx, dy * dy))
    hit = d > limit
    f = target / np.where(hit, d, np.float32(1.0))
    out = np.stack([_fma32(dx, f, c[..., 0]), _fma32(dy, f, c[..., 1])], axis=-1)
    return np.where(hit[..., None], out, p), hit


@lru_cache(maxsize=None)
def parted_positions():
    """float32 [B, D, 2].  Nothing moves (speed_std 0: every velocity is 0), so a step is the two tests alone.  Every receiver
    stands 1 to 3 ulp32(cell_radius) OUTSIDE the wall - inside the |p| <= cell_radius (1 + 2^-22) the kernel itself leaves - and
    at its tether's length to an ulp, no further than d2d_radius (1 + 2^-22) as the kernel leaves a pair (redrawn until the
    float32 coordinates say so); its transmitter stands within 1 m of the wall, so the pair is all but tangential: the projection
    onto the wall hardly shortens it, and the projection's rounding lengthens some beyond the bound.  The CUEs stand anywhere."""
    s = spec('parted')
    rng = np.random.default_rng([SEED, 99])
    b, pairs, cell, d2d, ulp = s['b'], s['pairs'], s['cell'], s['d2d'], mob.ulp32(s['cell'])
    pos = layout(rng, b, s['cues'], pairs, cell, d2d)
    todo = np.ones((b, pairs), dtype=bool)
    tx_at, rx_at = 1 + s['cues'] + 2 * np.arange(pairs), 2 + s['cues'] + 2 * np.arange(pairs)
    for _ in range(100):
        r_t = cell - rng.uniform(0.001, 1.0, (b, pairs))
        r_r = cell + ulp * rng.integers(1, 4, (b, pairs))
        rho = d2d - ulp * rng.uniform(0.0, 1.0, (b, pairs))
        phi = 2 * np.pi * rng.random((b, pairs))
        delta = np.arccos((r_r ** 2 + r_t ** 2 - rho ** 2) / (2 * r_r * r_t)) * rng.choice([-1.0, 1.0], (b, pairs))
        tx = np.stack([r_t * np.cos(phi), r_t * np.sin(phi)], axis=-1).astype(np.float32)
        rx = np.stack([r_r * np.cos(phi + delta), r_r * np.sin(phi + delta)], axis=-1).astype(np.float32)
        pos[:, tx_at] = np.where(todo[..., None], tx, pos[:, tx_at])
        pos[:, rx_at] = np.where(todo[..., None], rx, pos[:, rx_at])
        p = pos.astype(np.float64)
        todo = (np.hypot(*np.moveaxis(p[:, rx_at] - p[:, tx_at], -1, 0)) > d2d * TOL22) | (np.hypot(p[:, rx_at, 0], p[:, rx_at, 1]) > cell * TOL22) \
            | (np.hypot(p[:, rx_at, 0], p[:, rx_at, 1]) <= cell)
        if not todo.any():
            break
    assert not todo.any()
    pos.setflags(write=False)
    return pos


def parted_by_the_wall():
    """One step of the `parted` state's receivers in float32, as the kernel takes it: dict of bool [B, pairs] - wall: the wall
    test fired; parted: the pair then stands further apart than d2d_radius (1 + 2^-22), measured in float64 on the float32
    coordinates; again: the second tether test fired; mended: ... and the pair stands inside the bound afterwards."""
    s = spec('parted')
    pos = parted_positions()
    tx, rx = pos[:, 1 + s['cues']::2], pos[:, 2 + s['cues']::2]
    d2d_r = np.float32(s['d2d'])
    d2d_in = np.float32(d2d_r - np.float32(mob.ulp32(s['cell'])))
    far = lambda p: np.hypot(*np.moveaxis(p.astype(np.float64) - tx.astype(np.float64), -1, 0)) > s['d2d'] * TOL22
    p1, first = pull_inside32(rx, tx, d2d_r, d2d_in)
    p2, wall = pull_inside32(p1, np.zeros_like(p1), s['cell'], s['cell'])
    p3, again = pull_inside32(p2, tx, d2d_r, d2d_in)
    again &= wall
    p3 = np.where(again[..., None], p3, p2)
    return dict(first=first, wall=wall, parted=far(p2), again=again, mended=~far(p3), before=~far(rx))


def tether_target(s, rule):
    return None if rule == 'model_as_stated' else float(np.float32(s['d2d'])) - mob.ulp32(s['cell'])


def bar_ulp(name, t):
    """[D] the position bar of step t (t steps taken) in ulp32(cell_radius) PER STEP: the module docstring's counting."""
    s = spec(name)
    bar = np.full(s['d'], 4.0)
    if s['small']:
        bar[2 + s['cues']::2] = 14.0
        sigma, dt = s['model']['speed_std_mps'], s['model']['dt_s']
        bar += dt * 1e-6 * sigma * (t + 1) / 2 / mob.ulp32(s['cell'])
    return bar


def _left_out(r):
    out = r.near.copy()
    out[:, r.rx] |= out[:, r.tx]                                      # a receiver hangs on its transmitter's position
    return out


@lru_cache(maxsize=None)
def trajectory(name, rule, mask='null'):
    """The restatement of a lockstep case: dict(vel0 [B, D, 2], steps: a list of (pos, vel, left out [B, D]) per step, hits,
    rx_wall_hits: how often a receiver was pulled onto the wall).  Float64, read only."""
    s = spec(name)
    r = mob.Restatement(start_positions(name), s['cues'], s['pairs'], fixed_mask(name, mask)[0], seed=mob.stream_seed(SEED),
                        first_env=s['first_env'], episode=s['episode'], cell_radius=s['cell'], d2d_radius=s['d2d'],
                        tether_target=tether_target(s, rule), **s['model'])
    vel0 = r.vel.copy()
    r.t = s['t0'] - 1                                                 # (a jump in t is a jump in the draws: the state is pos, vel)
    steps, rx_wall = [], 0
    for t in s['ts']:
        pos, vel = r.step()
        assert r.t == t
        # a receiver stands ON the wall only where a wall hit put it (radius = cell_radius to a few 1e-16, below it otherwise)
        rx_wall += int((np.abs(np.hypot(pos[:, r.rx, 0], pos[:, r.rx, 1]) - r.cell_radius) < 1e-9).sum())
        steps.append((pos.copy(), vel.copy(), _left_out(r)))
    for a in (vel0,) + tuple(x for st in steps for x in st):
        a.setflags(write=False)
    return dict(vel0=vel0, steps=steps, hits=dict(r.hits), rx_wall_hits=int(rx_wall), tx=r.tx.copy(), rx=r.rx.copy())


# ---------------------------------------------------------------------------------------------- the per-env clock
CLOCK_B, CLOCK_LAUNCHES = 16, 31
CLOCK_FIRST_ENV = 2 ** 32 - CLOCK_B                                   # first_env + 16 == 2^32
CLOCK_RESETS = {1: tuple(range(CLOCK_B)), 12: (0, 3, 5, 10), 13: (3,)}
CLOCK_EPISODE0 = np.array([2 ** 32 - 2, 0, 2 ** 32 - 1, 2 ** 32 - 3, 7, 1, 8, 9, 10, 11, 2 ** 31, 13, 14, 15, 16, 2 ** 31 - 1], dtype=np.uint32)


@lru_cache(maxsize=None)
def clock_schedule():
    """The 31 launches of the clock cases, as the env's bookkeeping would feed them (include/d2d_mobility.h), with values in the
    words the kernel must not read that the env never produces.  A list of dicts, each:

        reset, elapsed int32 [16], episode uint32 [16]   the three read-only arrays of the launch
        start int32 [16]                                 start_env before the launch
        start_after int32 [16]                           start_env as the launch must leave it: 0 where flagged, else untouched
        own_episode, own_t                               the (episode, t) each env stands at, by the header's two formulas

    Launch 1 flags every env (start_env holds garbage); then start_env is the stagger arange(16) % 5, as the env's
    start.copy_(elapsed) leaves it after a staggered first reset.  Envs 0, 3, 5, 10 are flagged at launch 12 and env 3 again at
    launch 13.  episode_env starts at CLOCK_EPISODE0: env 1 resets at episode 0 and then READS episode_env 1 (steps in episode 0),
    env 2 resets at 2^32 - 1 and steps with episode_env wrapped to 0, envs 0 and 3 reach 2^32 - 1 and the wrap by their later
    resets.  A flag is any non-zero word; elapsed_env of a flagged env is garbage."""
    stagger = (np.arange(CLOCK_B) % 5).astype(np.int32)
    flags = np.array([1, -1, 2, 2 ** 31 - 1, -2 ** 31, 256, 1, 65536] * 2, dtype=np.int32)
    garbage = np.array([-5, 2 ** 31 - 1, 77, -2 ** 31, 12345, 4096, -1, 99] * 2, dtype=np.int32)      # (no zero: a lost write must show)
    episode = CLOCK_EPISODE0.copy()
    start = garbage[::-1].copy()
    elapsed = stagger.copy()
    out = []
    for launch in range(1, CLOCK_LAUNCHES + 1):
        flagged = np.zeros(CLOCK_B, dtype=bool)
        flagged[list(CLOCK_RESETS.get(launch, ()))] = True
        reset = np.where(flagged, flags, 0).astype(np.int32)
        seen = np.where(flagged, garbage, elapsed).astype(np.int32)
        own_episode = np.where(flagged, episode, episode - np.uint32(1)).astype(np.uint32)
        own_t = np.where(flagged, 0, seen.astype(np.int64) - start + 1).astype(np.int64)
        start_after = np.where(flagged, 0, start).astype(np.int32)
        out.append(dict(reset=reset, elapsed=seen, episode=episode.copy(), start=start.copy(), start_after=start_after,
                        own_episode=own_episode, own_t=own_t, flagged=flagged))
        # the env's bookkeeping behind the launch
        episode = np.where(flagged, episode + np.uint32(1), episode).astype(np.uint32)
        elapsed = np.where(flagged, 0, elapsed + 1).astype(np.int32)
        start = start_after.copy()
        if launch == 1:
            start, elapsed = stagger.copy(), stagger.copy()
    for step in out:
        for a in step.values():
            a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def clock_trajectory(rule):
    """The clock case by one single-env restatement per env, at first_env + e and the env's own (episode, t): a list of dicts per
    launch, pos / vel float64 [16, D, 2], out bool [16, D], t [16], fresh float32 [16, D, 2] (the positions the test puts into
    the planes of a flagged env before the launch: the kernel does not sample them)."""
    s = spec('clock')
    envs = [None] * CLOCK_B
    out = []
    for k, launch in enumerate(clock_schedule(), start=1):
        rng = np.random.default_rng([SEED, 1000 + k])
        fresh = layout(rng, CLOCK_B, s['cues'], s['pairs'], s['cell'], s['d2d'])
        for e in range(CLOCK_B):
            if launch['flagged'][e]:
                envs[e] = mob.Restatement(fresh[e:e + 1], s['cues'], s['pairs'], None, seed=mob.stream_seed(SEED),
                                          first_env=CLOCK_FIRST_ENV + e, episode=int(launch['own_episode'][e]),
                                          cell_radius=s['cell'], d2d_radius=s['d2d'], tether_target=tether_target(s, rule),
                                          **s['model'])
            else:
                envs[e].step()
            assert envs[e].t == launch['own_t'][e] and envs[e].episode == launch['own_episode'][e]
        out.append(dict(pos=np.concatenate([r.pos for r in envs]), vel=np.concatenate([r.vel for r in envs]),
                        out=np.concatenate([_left_out(r) for r in envs]), t=np.array(launch['own_t']), fresh=fresh,
                        hits={k2: sum(r.hits[k2] for r in envs) for k2 in ('wall', 'tether')}))
    return out

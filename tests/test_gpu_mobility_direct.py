"""Direct launches of d2d_mobility_move (csrc/d2d_mobility.hip: mobility_move_kernel) at the shapes test_gpu_mobility.py never gives it
through VecD2DEnv - one unit per env, a power-of-two unit count, no CUEs, no pairs, a unit count that is the workgroup, envs that
straddle workgroups, a 40 m cell whose tethered receivers stand on the wall, 4099 envs, the four kinds of fixed_mask, the counter
words at their ends, the per-env clock fed by hand - against the float64 restatement (mobility_util.Restatement) under both of its
rules.  The cases, each with the path it forces, are mobility_direct_util.CASES; test_element_direct_cpu.py asserts on the CPU that
the restatement can judge them and that they cover what they claim.

Every launch reads and writes tensors this file builds.  pos_x, pos_y, vel_x, vel_y (and start_env under the per-env clock) lie inside
larger allocations with 4 KiB of a byte pattern before and after them; the velocities are NaN before the t = 0 launch; after every
launch the device is synchronised, the patterns are intact, the launch counter has moved by one and fixed_mask, elapsed_env,
episode_env and reset_env are bit for bit what they were.

Yardsticks: test_gpu_mobility.py's.  Velocities within 1e-6 sigma t; positions within 4 ulp32(cell_radius) t; a device is left out
from the step on at which the restatement marks it `near`, and its receiver with it; at most 1 % is left out.  For small_cell and
many_envs the position bar is the one counted in mobility_direct_util's docstring: 4 (free devices) or 14 (tethered receivers:
three projections and the transmitter's own error) ulp32(cell_radius) per step, plus what the velocity bar lets the move carry into a
position, dt * 1e-6 sigma (t + 1) / 2 per step - 19.5 ulp per step at step 10 of small_cell, 8.7 of many_envs.

The path "the wall's rounding may have parted the pair again" cannot be judged by a float64 restatement (in exact arithmetic it never
fires).  The invariants judge it, on the GPU's own planes after every step of every case: |p| <= cell_radius (1 + 2^-22), pair
distance <= d2d_radius (1 + 2^-22), fixed devices bit-identical with zero velocity; and small_cell must show more than 1000
receivers standing on the wall and inside their tether (27 041).  No drawn case makes the path matter, though - the kernel without
that line passes all of them: the projection onto the wall shortens a pair by far more than its rounding lengthens it unless the
overshoot is a few ulp.  The hand-laid state `parted` (mobility_direct_util.parted_positions) is the one that fails without it.

Measured on one MI355X (worst position error in ulp32(cell_radius) per step, free devices / receivers, under the kernel's rule;
worst velocity error in sigma per step; share left out):
    bs_only       exact                         one_pair      1.21 / 1.13   4.3e-7   0
    one_cue       1.08 / -      3.7e-7   0      wg_units      1.37 / -      5.0e-7   0
    odd           1.61 / 1.79   6.1e-7   0.032 %
    small_cell    1.81 / 1.72   6.1e-7   0.079 %   (bars 7.5 / 17.5 at step 1, 23.5 / 33.5 at step 10)
    many_envs     1.98 / 1.88   6.3e-7   0.065 %   (bars 5.6 / 15.6 at step 1, 12.7 / 22.7 at step 10)
    masks         0.99 / 0.93   4.2e-7   0      counter_edge  0.53 / 0.74   2.9e-7   0      clock   0.88 / 0.86   3.2e-7   0
Under the model as stated the receivers' figures are 1.3 to 2.8.  Largest |p| / cell_radius - 1: 1.78e-7; largest pair distance /
d2d_radius - 1: 1.19e-8 (allowed 2.38e-7).  The 36 tests of this file took 4.1 s in all, the slowest 0.4 s; CHANGELOG.md has the
rest."""
from functools import lru_cache

import numpy as np
import pytest

import mobility_direct_util as mdu
import mobility_util as mob

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from guard_util import Guarded, bits  # noqa: E402  (after the importorskip: it imports torch)

RULES = ('model_as_stated', 'kernel_rule')
LOCKSTEP = [n for n in mdu.CASES if n not in ('clock', 'masks')]
PLANES = ('pos_x', 'pos_y', 'vel_x', 'vel_y')


class Launcher:
    """The four guarded planes of a case, its mask on the device, and launch(): one d2d_mobility_move with the checks every launch
    gets."""

    def __init__(self, name, mask='null'):
        self.name, self.s = name, mdu.spec(name)
        s = self.s
        self.planes = {k: Guarded((s['b'], s['d']), torch.float32) for k in PLANES}
        for k in ('vel_x', 'vel_y'):
            self.planes[k].array.fill_(float('nan'))                  # garbage: t = 0 has to write all of it
        self.mask_host = mdu.fixed_mask(name, mask)[1]
        self.mask = None if self.mask_host is None else torch.as_tensor(self.mask_host, device='cuda')
        self.a, self.noise, self.sigma, self.dt = mob.constants(**s['model'])
        self.launches = 0

    def put(self, pos, rows=None):
        """Positions float32 [B, D, 2] into the planes: of every env, or of the envs `rows` (indices)."""
        rows = np.arange(self.s['b']) if rows is None else np.asarray(rows)
        where = torch.as_tensor(rows, dtype=torch.int64, device='cuda')
        for axis, k in enumerate(('pos_x', 'pos_y')):
            self.planes[k].array[where] = torch.as_tensor(np.ascontiguousarray(pos[rows, :, axis]), device='cuda')

    def put_vel(self, vel):
        self.planes['vel_x'].array.copy_(torch.as_tensor(np.ascontiguousarray(vel[..., 0]), device='cuda'))
        self.planes['vel_y'].array.copy_(torch.as_tensor(np.ascontiguousarray(vel[..., 1]), device='cuda'))

    def get(self):
        """(pos, vel) float32 [B, D, 2] copies."""
        p = {k: g.array.cpu().numpy() for k, g in self.planes.items()}
        return np.stack([p['pos_x'], p['pos_y']], axis=-1), np.stack([p['vel_x'], p['vel_y']], axis=-1)

    def launch(self, step=0, episode=0, clock=None, start=None):
        from gym_d2d_amd import _native
        s = self.s
        kw, dev = dict(step=step, episode=episode), {}
        if clock is not None:
            dev = {k: torch.as_tensor(np.array(clock[k]).view(np.int32), device='cuda') for k in ('elapsed', 'episode', 'reset')}
            kw = dict(elapsed_ptr=dev['elapsed'].data_ptr(), start_ptr=start.array.data_ptr(), episode_ptr=dev['episode'].data_ptr(),
                      reset_ptr=dev['reset'].data_ptr())
        before = _native.mobility_launches
        torch.cuda.synchronize()
        _native.mobility_move(*(self.planes[k].array.data_ptr() for k in PLANES), 0 if self.mask is None else self.mask.data_ptr(),
                              s['b'], s['cues'], s['pairs'], s['first_env'], mob.stream_seed(mdu.SEED), self.a, self.noise, self.sigma,
                              self.dt, s['cell'], s['d2d'], stream_ptr=torch.cuda.current_stream().cuda_stream, **kw)
        torch.cuda.synchronize()
        self.launches += 1
        what = f'{self.name} launch {self.launches}'
        assert _native.mobility_launches == before + 1, what
        for k, g in self.planes.items():
            assert g.intact(), f'{what}: bytes around {k} were written'
        if start is not None:
            assert start.intact(), f'{what}: bytes around start_env were written'
        if self.mask is not None:
            assert np.array_equal(bits(self.mask), bits(self.mask_host)), f'{what}: fixed_mask was written'
        for k, t in dev.items():
            assert np.array_equal(bits(t), bits(np.array(clock[k]))), f'{what}: {k}_env was written'


@lru_cache(maxsize=None)
def _run(name, mask='null'):
    """A lockstep case on the GPU, launched once and shared by the tests: vel0, and (pos, vel) after every step.  Read only."""
    s = mdu.spec(name)
    pos0 = mdu.start_positions(name)
    gpu = Launcher(name, mask)
    gpu.put(pos0)
    gpu.launch(0, s['episode'])
    pos, vel0 = gpu.get()
    assert np.array_equal(bits(pos), bits(pos0)), f'{name}: the t = 0 launch wrote a position'
    steps = []
    for t in s['ts']:
        gpu.launch(t, s['episode'])
        steps.append(gpu.get())
    for a in (vel0,) + tuple(x for st in steps for x in st):
        a.setflags(write=False)
    return dict(vel0=vel0, steps=steps)


def _judge(label, name, k, t, got, ref, out):
    """One state against the restatement's: k the launch it is printed as, t [B] or a number: the steps taken since t = 0.  Returns
    the worst position error in ulp32(cell_radius) per step of (free devices, receivers) and the worst velocity error in sigma per
    step."""
    s = mdu.spec(name)
    sigma, ulp = s['model']['speed_std_mps'], mob.ulp32(s['cell'])
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (s['b'],))[:, None]
    steps = np.maximum(t, 1.0)
    ep = np.abs(got[0] - ref[0]).max(axis=-1) / (ulp * steps)
    ev = np.abs(got[1] - ref[1]).max(axis=-1) / (sigma * steps)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), f'{label} launch {k}: NaN left in a plane'
    assert out.mean() <= mdu.LEFT_OUT_CAP, (label, k, out.mean())
    bar = np.stack([mdu.bar_ulp(name, int(x)) for x in steps[:, 0]]) if s['small'] else np.full(ep.shape, 4.0)
    bar = np.where(t > 0, bar, 0.0)                                   # t = 0 touches no position
    rx = np.zeros(s['d'], dtype=bool)
    rx[2 + s['cues']::2] = True
    keep = ~out
    worst = (float(ep[:, ~rx][keep[:, ~rx]].max()), float(ep[:, rx][keep[:, rx]].max()) if rx.any() else 0.0, float(ev[keep].max()))
    over_p, over_v = keep & (ep > bar), keep & (ev > 1e-6)
    assert not over_p.any(), (f'{label} launch {k}: {int(over_p.sum())} positions beyond the bar, the worst {ep[over_p].max():.2f} ulp32(cell_radius) '
                              f'per step at (env, device) {np.argwhere(over_p)[0].tolist()}, bar {bar[over_p].max():.2f}')
    assert not over_v.any(), f'{label} launch {k}: {int(over_v.sum())} velocities beyond 1e-6 sigma per step, the worst {ev[over_v].max():.3e}'
    return worst


# ------------------------------------------------------------------------------------------ 1: trajectories
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('name', LOCKSTEP)
def test_trajectory_follows_the_restatement(name, rule):
    s = mdu.spec(name)
    got, ref = _run(name), mdu.trajectory(name, rule)
    label = f'{name} ({rule})'
    pos0 = mdu.start_positions(name)
    none = np.zeros((s['b'], s['d']), dtype=bool)
    w0 = _judge(label, name, 0, 0, (pos0, got['vel0']), (pos0.astype(np.float64), ref['vel0']), none)
    worst = np.zeros(3)
    for k, (g, r) in enumerate(zip(got['steps'], ref['steps']), start=1):
        worst = np.maximum(worst, _judge(label, name, k, k, g, r[:2], r[2]))
    left = max(float(r[2].mean()) for r in ref['steps'])
    print(f'{label} B={s["b"]} D={s["d"]}: start velocities {w0[2]:.2e} sigma; worst position error {worst[0]:.2f} (free) / {worst[1]:.2f} '
          f'(receivers) ulp32(cell_radius) per step, bars {mdu.bar_ulp(name, 10)[1 if s["d"] > 1 else 0]:.1f} / {mdu.bar_ulp(name, 10)[-1]:.1f} '
          f'at step 10; worst velocity error {worst[2]:.2e} sigma per step; left out {left:.3%}; hits {ref["hits"]}')
    if name == 'bs_only':                                             # exact: nothing moves, the velocities are +0.0
        assert not bits(got['vel0']).any()
        assert all(np.array_equal(bits(p), bits(pos0)) and not bits(v).any() for p, v in got['steps'])


# ------------------------------------------------------------------------------------------ 2: invariants
def _invariants(name, got, fixed, pos0):
    """On the GPU's own planes; returns (largest |p| / cell_radius, largest pair distance / d2d_radius, receivers standing on
    the wall and inside their tether, summed over the steps)."""
    s = mdu.spec(name)
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    free = ~(fixed[tx] & fixed[tx + 1])                               # a pair pinned as a whole stands where the layout put it
    worst_r = worst_d = 0.0
    on_wall = 0
    for k, (pos, vel) in enumerate(got['steps'], start=1):
        p = pos.astype(np.float64)
        radius = np.hypot(p[..., 0], p[..., 1])
        assert radius[:, ~fixed].max(initial=0.0) <= s['cell'] * mdu.TOL22, (name, k)
        worst_r = max(worst_r, radius[:, ~fixed].max(initial=0.0) / s['cell'])
        if s['pairs']:
            dist = np.hypot(*np.moveaxis(p[:, tx + 1] - p[:, tx], -1, 0))
            assert dist[:, free].max(initial=0.0) <= s['d2d'] * mdu.TOL22, (name, k)
            worst_d = max(worst_d, dist[:, free].max(initial=0.0) / s['d2d'])
            on_wall += int(((radius[:, tx + 1] >= s['cell'] * (1.0 - 2.0 ** -22)) & (dist <= s['d2d'] * mdu.TOL22) & ~fixed[tx + 1]).sum())
        assert np.array_equal(bits(pos[:, fixed]), bits(pos0[:, fixed])), (name, k)
        assert not bits(vel[:, fixed]).any(), (name, k)
        assert (pos[:, ~fixed] != pos0[:, ~fixed]).any(axis=-1).all(), (name, k)
    return worst_r, worst_d, on_wall


@pytest.mark.parametrize('name', LOCKSTEP)
def test_invariants_hold_on_the_gpu_s_own_planes_after_every_step(name):
    worst_r, worst_d, on_wall = _invariants(name, _run(name), mdu.fixed_mask(name)[0], mdu.start_positions(name))
    print(f'{name}: largest |p| / cell_radius - 1 = {worst_r - 1:.3e}, largest pair distance / d2d_radius - 1 = {worst_d - 1:.3e} '
          f'(allowed {2.0 ** -22:.3e}); receivers on the wall and inside their tether: {on_wall}')
    if name == 'small_cell':
        assert on_wall > 1000


def test_a_pair_the_wall_s_rounding_parts_is_pulled_together_again():
    """The hand-laid state of mobility_direct_util.parted_positions: nothing moves, every receiver stands an ulp or three outside
    the wall at its tether's length.  Operation by operation in float32 the wall's projection leaves 137 of the 16 951 pairs
    further apart than the bound (test_element_direct_cpu.py); only the second tether test brings them back."""
    s, pos0 = mdu.spec('parted'), mdu.parted_positions()
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    rx = np.zeros(s['d'], dtype=bool)
    rx[tx + 1] = True
    gpu = Launcher('parted')
    gpu.put(pos0)
    gpu.launch(0, s['episode'])
    pos, vel = gpu.get()
    assert np.array_equal(bits(pos), bits(pos0)) and (vel == 0).all()                       # speed_std 0: every velocity is 0
    for t in (1, 2, 3):
        gpu.launch(t, s['episode'])
        pos, vel = gpu.get()
        p = pos.astype(np.float64)
        dist = np.hypot(*np.moveaxis(p[:, tx + 1] - p[:, tx], -1, 0))
        radius = np.hypot(p[..., 0], p[..., 1])
        moved = (pos != pos0).any(axis=-1)
        print(f'parted step {t}: largest |p| / cell_radius - 1 = {radius.max() / s["cell"] - 1:.3e}, largest pair distance / d2d_radius - 1 = '
              f'{dist.max() / s["d2d"] - 1:.3e} (allowed {2.0 ** -22:.3e}); receivers the wall moved: {int(moved[:, rx].sum())}')
        assert radius.max() <= s['cell'] * mdu.TOL22, t
        assert dist.max() <= s['d2d'] * mdu.TOL22, f'step {t}: {int((dist > s["d2d"] * mdu.TOL22).sum())} pairs stand apart'
        assert np.array_equal(bits(pos[:, ~rx]), bits(pos0[:, ~rx])) and (vel == 0).all(), t
        assert moved[:, rx].sum() > 16000


# ------------------------------------------------------------------------------------------ 3: fixed_mask
def test_an_all_zero_mask_gives_the_bytes_of_a_null_mask():
    null, zeros = _run('masks', 'null'), _run('masks', 'zeros')
    assert np.array_equal(bits(null['vel0']), bits(zeros['vel0']))
    for (p0, v0), (p1, v1) in zip(null['steps'], zeros['steps']):
        assert np.array_equal(bits(p0), bits(p1)) and np.array_equal(bits(v0), bits(v1))


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('mask', ['null', 'pinned'])
def test_masked_trajectory_follows_the_restatement_and_keeps_the_invariants(mask, rule):
    s = mdu.spec('masks')
    got, ref = _run('masks', mask), mdu.trajectory('masks', rule, mask)
    pos0 = mdu.start_positions('masks')
    label = f'masks/{mask} ({rule})'
    none = np.zeros((s['b'], s['d']), dtype=bool)
    worst = np.array(_judge(label, 'masks', 0, 0, (pos0, got['vel0']), (pos0.astype(np.float64), ref['vel0']), none))
    for k, (g, r) in enumerate(zip(got['steps'], ref['steps']), start=1):
        worst = np.maximum(worst, _judge(label, 'masks', k, k, g, r[:2], r[2]))
    fixed = mdu.fixed_mask('masks', mask)[0]
    assert not bits(got['vel0'][:, fixed]).any()
    worst_r, worst_d, _ = _invariants('masks', got, fixed, pos0)
    print(f'{label}: worst position error {worst[0]:.2f} / {worst[1]:.2f} ulp32(cell_radius) per step, velocity {worst[2]:.2e} sigma per step; '
          f'|p| / cell_radius - 1 = {worst_r - 1:.3e}, pair distance / d2d_radius - 1 = {worst_d - 1:.3e}; hits {ref["hits"]}')


def test_a_mask_of_all_ones_writes_zero_velocities_at_t_0_and_nothing_afterwards():
    got, pos0 = _run('masks', 'ones'), mdu.start_positions('masks')
    assert not bits(got['vel0']).any()                                # written (they were NaN), as +0.0
    for pos, vel in got['steps']:
        assert np.array_equal(bits(pos), bits(pos0)) and not bits(vel).any()


# ------------------------------------------------------------------------------------------ 4: the same launch twice
def test_a_second_launch_from_the_same_state_gives_the_same_bytes():
    name, k = 'small_cell', 6
    s, got = mdu.spec(name), _run(name)
    gpu = Launcher(name)
    for _ in range(2):
        gpu.put(got['steps'][k - 2][0])
        gpu.put_vel(got['steps'][k - 2][1])
        gpu.launch(s['ts'][k - 1], s['episode'])
        pos, vel = gpu.get()
        assert np.array_equal(bits(pos), bits(got['steps'][k - 1][0])) and np.array_equal(bits(vel), bits(got['steps'][k - 1][1]))
    gpu.put(mdu.start_positions(name))
    gpu.launch(0, s['episode'])
    assert np.array_equal(bits(gpu.get()[1]), bits(got['vel0']))


# ------------------------------------------------------------------------------------------ 5: the per-env clock
@lru_cache(maxsize=None)
def _run_clock():
    """The 31 launches of mobility_direct_util.clock_schedule; per launch (pos, vel) and start_env as the launch left it."""
    sched, ref = mdu.clock_schedule(), mdu.clock_trajectory('kernel_rule')
    gpu = Launcher('clock')
    for k in ('pos_x', 'pos_y'):
        gpu.planes[k].array.fill_(float('nan'))                       # every env's positions come from the test, at its reset
    start = Guarded((mdu.CLOCK_B,), torch.int32)
    out = []
    for k, (launch, r) in enumerate(zip(sched, ref), start=1):
        f = launch['flagged']
        if f.any():                                                   # the kernel does not sample positions: the test sets them
            gpu.put(r['fresh'], np.flatnonzero(f))
        if k <= 2:                                                    # garbage, then the stagger; afterwards what the kernel left
            start.array.copy_(torch.as_tensor(np.array(launch['start'])))
        assert np.array_equal(start.array.cpu().numpy(), launch['start']), k
        gpu.launch(clock=launch, start=start)
        pos, vel = gpu.get()
        if f.any():
            assert np.array_equal(bits(pos[f]), bits(r['fresh'][f])), f'launch {k}: a reset wrote a position'
        out.append((pos, vel, start.array.cpu().numpy()))
    return out


def test_per_env_clock_writes_start_env_of_flagged_envs_and_of_no_other():
    sched = mdu.clock_schedule()
    for k, (launch, (_, _, start)) in enumerate(zip(sched, _run_clock()), start=1):
        assert start.dtype == np.int32 and np.array_equal(start, launch['start_after']), k
    assert sched[0]['start'].all() and (sched[11]['start'][[3]] != 0).all() and sched[11]['start'][~sched[11]['flagged']].any()


@pytest.mark.parametrize('rule', RULES)
def test_per_env_clock_equals_one_single_env_restatement_per_env(rule):
    ref = mdu.clock_trajectory(rule)
    worst = np.zeros(3)
    for k, (r, (pos, vel, _)) in enumerate(zip(ref, _run_clock()), start=1):
        worst = np.maximum(worst, _judge(f'clock ({rule})', 'clock', k, r['t'], (pos, vel), (r['pos'], r['vel']), r['out']))
    left = max(float(r['out'].mean()) for r in ref)
    print(f'clock ({rule}): 31 launches, worst position error {worst[0]:.2f} / {worst[1]:.2f} ulp32(cell_radius) per step, worst velocity error '
          f'{worst[2]:.2e} sigma per step, left out {left:.3%}, hits {ref[-1]["hits"]}')


def test_per_env_clock_keeps_the_invariants():
    s = mdu.spec('clock')
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    for k, (pos, vel, _) in enumerate(_run_clock(), start=1):
        p = pos.astype(np.float64)
        assert np.hypot(p[..., 0], p[..., 1]).max() <= s['cell'] * mdu.TOL22, k
        assert np.hypot(*np.moveaxis(p[:, tx + 1] - p[:, tx], -1, 0)).max() <= s['d2d'] * mdu.TOL22, k
        assert not bits(pos[:, 0]).any() and not bits(vel[:, 0]).any(), k

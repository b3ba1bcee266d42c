"""The placement kernels (csrc/d2d_reset.hip: reset_kernel, reset_masked_kernel) and the two small kernels at the end of
csrc/d2d_step.hip (link_positions_kernel, flags_or_kernel) through the C ABI at the shapes no other test gives them, against the float64
restatement reset_util.restate and plain NumPy.  The cases, each with the path it forces, are reset_util.CASES; test_reset_cpu.py asserts
on the CPU that the restatement can judge them (the ambiguity cap) and that they cover what they claim.

The handles are driven as tools/fuzz_reset.py and test_gpu_autoreset.py drive theirs.  POS_X and POS_Y (ENV_FLAGS in the flag test) are
bound to allocations with 4 KiB of a byte pattern before and after the array (guard_util.Guarded), NaN-filled before the first launch;
after every launch the handle is synchronised and the patterns are intact.  BUF_LINK_POS cannot be bound (the library owns it).

Yardsticks.  A device that is neither ambiguous nor exhausted: |got - ref| <= 2e-6 cell_radius per coordinate (test_gpu_reset.py's and
tools/fuzz_reset.py's bar; by the code the kernel is about 3e-7 off, reset_util's docstring).  Every device: inside the cell within 1e-6 of
the radius; every receiver within d2d_radius (1 + 1e-5) + 2.4e-7 cell_radius of its transmitter (fuzz_reset.py's two bounds - they hold
for the ambiguous receivers in particular).  An exhausted receiver: its transmitter's bits.  Everything else is bit for bit: a second
launch, BUF_LINK_POS against the NumPy gather of POS_X / POS_Y, shards against one handle, a masked reset against a full reset at the
env's episode, the envs a masked reset leaves alone.

Measured on one MI355X (worst deviation of a judged device, in units of the cell radius, at the 2e-6 bar; no receiver of any case is
ambiguous at its own episode):
    default 1.34e-7   units_3 7.3e-8   one_pair 8.7e-8   wave_plus_one 1.34e-7   wide 1.28e-7   big_d2d 2.39e-7   late 2.81e-7
    exhaust 8.7e-8   first_env_wrap 1.12e-7   pinned 1.34e-7   pinned_cues 1.34e-7   masked resets at most 1.97e-7 (big_d2d)
The 66 tests of this file took 3.2 s in all, the slowest (which loads the library) 0.6 s; CHANGELOG.md has the rest, with the five
value-only mutations of the kernels and the tests each one fails."""
import numpy as np
import pytest

import reset_util as ru

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from guard_util import Guarded, bits  # noqa: E402  (after the importorskip: it imports torch)

LINK_LISTS = ('default', 'reversed', 'downlink', 'single', 'mixed', 'repeated')


def n_links(kind, cues, pairs):
    n = cues + pairs
    return {'default': n, 'reversed': n, 'downlink': n, 'single': 1, 'mixed': n + cues + 1, 'repeated': 2 * n}[kind]


def link_keys(sim, kind):
    """Link lists d2d_set_links accepts.  'default' is the standard list (the sampler writes its rows); every other one is gathered:
    'mixed' is the reversed default, then every downlink, then the first default link once more."""
    from gym_d2d_amd.simulator import BASE_STATION_ID
    default = sim.default_link_keys()
    down = [(BASE_STATION_ID, c) for c in sim.devices.cues.keys()]
    return {'default': default, 'reversed': default[::-1], 'downlink': down + list(sim.devices.dues.keys()), 'single': default[-1:],
            'mixed': default[::-1] + down + default[:1], 'repeated': default + default}[kind]


class Rig:
    """One handle of a case's shape with its link list set, its env offset set and POS_X / POS_Y bound to guarded arrays."""

    def __init__(self, native, s, b=None, first_env=None, links='default', guard=True, guard_flags=False):
        from gym_d2d_amd.simulator import Simulator
        self.n, self.s = native, s
        self.b = s['b'] if b is None else b
        self.sim = Simulator(dict(num_cues=s['cues'], num_due_pairs=s['pairs'], num_envs=self.b, cell_radius_m=s['cell'],
                                  d2d_radius_m=s['d2d']), max_links=max(2 * s['cues'] + s['pairs'], n_links(links, s['cues'], s['pairs'])))
        self.h = self.sim.handle
        self.sim.set_links(link_keys(self.sim, links))
        assert self.h.num_links == n_links(links, s['cues'], s['pairs'])
        self.h.set_env_offset(s['first_env'] if first_env is None else first_env)
        self.guards = {}
        if guard:
            for which in (native.BUF_POS_X, native.BUF_POS_Y):
                g = Guarded((self.b, s['d']), torch.float32)
                g.array.fill_(float('nan'))                               # garbage: a reset has to write all of it
                self.guards[which] = g
        if guard_flags:
            self.guards[native.BUF_ENV_FLAGS] = Guarded((self.b,), torch.int32)
            self.guards[native.BUF_ENV_FLAGS].array.fill_(-1)
        torch.cuda.synchronize()                                          # the handle launches on a stream of its own
        for which, g in self.guards.items():
            self.h.bind_buffer(which, g.array.data_ptr(), g.nbytes)

    def intact(self):
        self.h.synchronize()
        assert all(g.intact() for g in self.guards.values()), 'a store outside POS_X / POS_Y'

    def reset(self, episode, pins=None):
        mask, xy = (None, None) if pins is None else ru.mask_xy(pins, self.s['d'])
        self.h.reset_positions(ru.SEED, episode, mask, xy)
        self.intact()

    def mark(self, pending, episode):
        self.h.upload(self.n.BUF_RESET_PENDING, pending)
        self.h.upload(self.n.BUF_EPISODE, episode)

    def marks(self):
        return self.h.download(self.n.BUF_RESET_PENDING), self.h.download(self.n.BUF_EPISODE)

    def state(self):
        """(POS_X [B, D], POS_Y [B, D], LINK_POS [B, N, 4]) float32 copies; the download brings the link rows up to date."""
        out = [self.h.download(w) for w in (self.n.BUF_POS_X, self.n.BUF_POS_Y, self.n.BUF_LINK_POS)]
        self.intact()
        return out

    def rows(self, px, py):
        return ru.gather_rows(px, py, self.sim.link_tx, self.sim.link_rx)

    def close(self):
        self.h.close()


def same_bits(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def judge(tag, s, ref, px, py, envs=None, pins=None):
    """The yardsticks of this file's docstring on the envs `envs` (every env if None).  Returns the worst deviation of a judged device
    in units of the cell radius, printed before anything is asserted."""
    envs = np.arange(px.shape[0]) if envs is None else np.asarray(envs)
    cell, d2d = s['cell'], s['d2d']
    px, py = px[envs], py[envs]
    got = np.stack([px, py], axis=-1).astype(np.float64)
    want, amb, exh = ref.pos[envs], ref.ambiguous[envs], ref.exhausted[envs]
    dev = np.abs(got - want).max(axis=2)
    judged = ~amb & ~exh
    worst = float(dev[judged].max() / cell)
    rx = ru.receivers(s['cues'], s['d'])
    print(f'{tag}: worst deviation {worst:.2e} of the cell radius over {int(judged.sum())} devices; ambiguous {int(amb.sum())} of '
          f'{amb[:, rx].size} receivers; exhausted {int(exh.sum())}')
    assert np.isfinite(got).all(), tag
    assert (dev[judged] <= ru.BAR * cell).all(), (tag, worst, np.argwhere(judged & (dev > ru.BAR * cell))[:5].tolist())
    assert (np.hypot(got[..., 0], got[..., 1]) <= cell * (1 + ru.INSIDE_TOL)).all(), tag
    rx = np.array([k for k in rx if k not in (pins or {})], dtype=np.int64)      # a pinned receiver is not drawn around its transmitter
    if rx.size:
        gap = np.hypot(got[:, rx, 0] - got[:, rx - 1, 0], got[:, rx, 1] - got[:, rx - 1, 1])
        assert (gap <= d2d * (1 + ru.PAIR_TOL[0]) + ru.PAIR_TOL[1] * cell).all(), tag
        on_tx = exh[:, rx] & ~amb[:, rx]                                  # an exhausted receiver: its transmitter's bits
        same_bits(px[:, rx][on_tx], px[:, rx - 1][on_tx], f'{tag}: exhausted x')
        same_bits(py[:, rx][on_tx], py[:, rx - 1][on_tx], f'{tag}: exhausted y')
        live = ~exh[:, rx] & ~amb[:, rx]
        assert (gap[live] > 0.0).all(), tag                               # the open radius interval
    assert not bits(px[:, 0]).any() and not bits(py[:, 0]).any(), f'{tag}: the base station is (+0, +0)'
    for k, xy in (pins or {}).items():
        if k:
            same_bits(px[:, k], np.full(len(envs), xy[0], dtype=np.float32), f'{tag}: pin {k} x')
            same_bits(py[:, k], np.full(len(envs), xy[1], dtype=np.float32), f'{tag}: pin {k} y')
    return worst


# ---------------------------------------------------------------------------------------------------------------- the full reset
@pytest.mark.parametrize('name', ru.FULL)
def test_full_reset_against_the_restatement(native, name):
    """Three launches: the next episode (the link records are not current yet: the rows are gathered by link_positions_kernel at the
    download), then the case's episode twice (the sampler writes the rows itself, over the other episode's).  Pinned devices, the
    receiver drawn around a pinned transmitter and the wrap of first_env + b are judged by the same restatement."""
    s, ref = ru.spec(name), ru.reference(name)
    rig = Rig(native, s)
    try:
        rig.reset(s['episode'] + 1, s['pins'])
        px, py, lp = rig.state()
        same_bits(lp, rig.rows(px, py), f'{name}: gathered rows')
        other = ru.restate(ru.SEED, s['episode'] + 1, s['b'], s['cues'], s['pairs'], s['cell'], s['d2d'], s['first_env'], s['pins'])
        judge(f'{name} (episode + 1)', s, other, px, py, pins=s['pins'])
        rig.reset(s['episode'], s['pins'])
        first = rig.state()
        rig.reset(s['episode'], s['pins'])
        second = rig.state()
        for a, b_, what in zip(first, second, ('POS_X', 'POS_Y', 'LINK_POS')):
            same_bits(b_, a, f'{name}: second launch, {what}')
        assert not np.array_equal(px, second[0]), f'{name}: another episode, other positions'
        px, py, lp = second
        judge(name, s, ref, px, py, pins=s['pins'])
        same_bits(lp, rig.rows(px, py), f'{name}: rows of the sampler')
        assert lp.shape == (s['b'], s['links'], 4)
        assert not bits(lp[:, :s['cues'], 2:]).any(), f'{name}: a CUE row ends in (0, 0)'
    finally:
        rig.close()


def test_first_env_wraps_in_the_counter(native):
    """first_env = 2^32 - 3: envs 3..7 are, bit for bit, envs 0..4 of a handle at first_env 0 (the restatement judges the handle
    itself in test_full_reset_against_the_restatement)."""
    s = ru.spec('first_env_wrap')
    high, zero = Rig(native, s), Rig(native, s, b=5, first_env=0)
    try:
        high.reset(s['episode']); zero.reset(s['episode'])
        for a, b_, what in zip(high.state(), zero.state(), ('POS_X', 'POS_Y', 'LINK_POS')):
            same_bits(a[3:], b_, what)
            assert not np.array_equal(a[:3], b_[:3]), what
    finally:
        high.close(); zero.close()


def test_two_shards_equal_one_handle(native):
    """`wide` at first_env 1000: handles of 3 and 2 envs at first_env 1000 and 1003 against the handle of 5, bit for bit."""
    s = ru.spec('wide')
    whole, head, tail = Rig(native, s), Rig(native, s, b=3, first_env=s['first_env']), Rig(native, s, b=2, first_env=s['first_env'] + 3)
    try:
        for r in (whole, head, tail):
            r.reset(s['episode']); r.state(); r.reset(s['episode'])          # the second launch: rows by the sampler
        for a, h_, t_, what in zip(whole.state(), head.state(), tail.state(), ('POS_X', 'POS_Y', 'LINK_POS')):
            same_bits(a, np.concatenate([h_, t_]), what)
    finally:
        whole.close(); head.close(); tail.close()


@pytest.mark.parametrize('name,raised', [('exhaust', True), ('late', True), ('default', False)])
def test_an_exhausted_receiver_shows_as_zero_distance_at_the_next_step(native, name, raised):
    """include/d2d_hip.h: a receiver whose 64 tries are all rejected stands on its transmitter; the step reports it."""
    s = ru.spec(name)
    rig = Rig(native, s, guard_flags=True)                                # ENV_FLAGS bound too, -1 in every env before the step
    try:
        with pytest.raises(native.NativeError) as err:                    # the library owns LINK_POS: no guard bands around it
            rig.h.bind_buffer(native.BUF_LINK_POS, rig.guards[native.BUF_POS_X].array.data_ptr(), 16)
        assert err.value.code == native.ERR_INVALID
        rig.reset(s['episode'])
        rig.state()
        rig.sim.step_arrays(np.zeros((s['b'], s['links']), dtype=np.int32))
        rig.intact()
        assert bool(rig.h.status_flags() & native.FLAG_ZERO_DISTANCE) == raised
        flags = rig.h.download(native.BUF_ENV_FLAGS)
        want = ru.reference(name).exhausted.any(axis=1)
        np.testing.assert_array_equal((flags & native.FLAG_ZERO_DISTANCE) != 0, want)
    finally:
        rig.close()


# -------------------------------------------------------------------------------------------------------------- the masked reset
def _masked(native, s, b, links, route, pins=None, tag=''):
    pending, episode = ru.pending_and_episodes(b)
    ref = ru.restate(ru.SEED, episode, b, s['cues'], s['pairs'], s['cell'], s['d2d'], s['first_env'], pins)
    rig, twin = Rig(native, s, b=b, links=links), Rig(native, s, b=b, links=links, guard=False)
    try:
        rig.reset(s['episode'], pins)
        before = rig.state()                                              # the rows are current from here on
        rig.mark(pending, episode)
        if route == 'not_current':
            rig.h.positions_changed()                                     # the reset writes no row; the next download rebuilds them
        rig.reset(native.EPISODE_PER_ENV)
        after = rig.state()
        same_bits(after[2], rig.rows(after[0], after[1]), f'{tag}: rows against the gather')
        todo = np.flatnonzero(pending)
        for e in range(b):
            if pending[e]:
                twin.reset(int(episode[e]), pins)
                want = twin.state()
            else:
                want = before
            for k, what in enumerate(('POS_X', 'POS_Y', 'LINK_POS')):
                same_bits(after[k][e], want[k][e], f'{tag}: env {e} ({"reset" if pending[e] else "left alone"}), {what}')
        worst = judge(tag, s, ref, after[0], after[1], envs=todo, pins=pins)
        got_pending, got_episode = rig.marks()
        np.testing.assert_array_equal(got_pending, pending)
        np.testing.assert_array_equal(got_episode, episode)
        return worst
    finally:
        rig.close(); twin.close()


@pytest.mark.parametrize('route', ['units', 'gathered', 'not_current'])
@pytest.mark.parametrize('b', ru.MASKED_B)
@pytest.mark.parametrize('shape', ru.MASKED_SHAPES)
def test_masked_reset_against_the_restatement_and_a_full_reset(native, shape, b, route):
    """Each pending env (words 1, -1, 7; the last env among them, its workgroup partly filled) at its own episode (0 and 2^32 - 1
    among them) against the restatement and, bit for bit, a full reset at that episode on a second handle; every other env as before.
    Routes of reset_pending: rows written by the units (standard list), rows gathered per reset env ('mixed' list, N past 64 for
    wave_plus_one and wide), rows not current (positions_changed first: rebuilt by the next download)."""
    links = 'mixed' if route == 'gathered' else 'default'
    _masked(native, ru.spec(shape), b, links, route, tag=f'masked {shape} B={b} {route}')


def test_masked_reset_keeps_the_pins_of_the_last_full_reset(native):
    s = ru.spec('pinned')
    for route in ('units', 'not_current'):
        _masked(native, s, s['b'], 'default', route, pins=s['pins'], tag=f'masked pinned {route}')


@pytest.mark.parametrize('links', ['default', 'reversed'])
def test_masked_reset_zeroes_the_low_parts_past_one_wave(native, links):
    """test_masked_reset_zeroes_the_low_parts_of_reset_envs_only at 271 devices and 170 links (three trips of the loops over lo_x and
    rows_lo): after float64 positions, the step equals that of a handle given the expected float64 coordinates."""
    s, b = ru.spec('wide'), 5
    pending, episode = ru.pending_and_episodes(b)
    rig, twin = Rig(native, s, b=b, links=links, guard=False), Rig(native, s, b=b, links=links, guard=False)
    planes = (native.BUF_SINR_DB, native.BUF_SNR_DB, native.BUF_CAPACITY, native.BUF_REWARD)
    try:
        rig.reset(s['episode'])
        px, py, _ = rig.state()
        pos = np.stack([px, py], axis=-1).astype(np.float64)
        pos += np.random.default_rng(4).uniform(-1e-4, 1e-4, pos.shape)                # low parts float32 cannot hold
        pos[:, 0] = 0.0
        rig.sim.set_positions(pos)
        raw = np.random.default_rng(5).integers(0, 25 * 4, (b, s['links'])).astype(np.int32)
        rig.sim.step_arrays(raw)                                          # the rows and their low parts are current
        rig.mark(pending, episode)
        rig.reset(native.EPISODE_PER_ENV)
        rig.sim.step_arrays(raw)
        got = [rig.h.download(w) for w in planes]
        expect = pos.copy()
        for e in np.flatnonzero(pending):
            twin.reset(int(episode[e]))
            fx, fy, _ = twin.state()
            expect[e, :, 0], expect[e, :, 1] = fx[e], fy[e]
        twin.sim.set_positions(expect)
        twin.sim.step_arrays(raw)
        want = [twin.h.download(w) for w in planes]
        for g, w, what in zip(got, want, ('sinr_db', 'snr_db', 'capacity', 'reward')):
            assert np.isfinite(w).all(), what
            same_bits(g, w, what)
        # and the low parts did matter: the float32 roundings of the same coordinates give other bits somewhere
        twin.sim.set_positions(expect.astype(np.float32))
        twin.sim.step_arrays(raw)
        assert any(not np.array_equal(twin.h.download(w), g) for w, g in zip(planes, got))
    finally:
        rig.close(); twin.close()


# ------------------------------------------------------------------------------------------------------- link_positions_kernel
@pytest.mark.parametrize('shape,links,b', [('wide', 'reversed', 5), ('wide', 'downlink', 5), ('wide', 'default', 5), ('wide', 'repeated', 5),
                                           ('wide', 'repeated', 1), ('wide', 'single', 1), ('default', 'single', 33),
                                           ('default', 'reversed', 1), ('default', 'mixed', 67)])
def test_link_rows_equal_the_numpy_gather(native, shape, links, b):
    """BUF_LINK_POS after positions_changed(): link_positions_kernel over B * N threads - 850, 1700 (a list of 340 links), 340, 1, 33,
    15 and 1474, none a multiple of 256 - on positions that differ in every word."""
    s = ru.spec(shape)
    rig = Rig(native, s, b=b, links=links)
    try:
        n = rig.h.num_links
        assert (b * n) % 256 != 0
        rig.reset(s['episode'])
        rig.state()
        xy = np.random.default_rng(b * 1000 + n).uniform(-400.0, 400.0, (2, b, s['d'])).astype(np.float32)
        rig.h.set_positions(xy[0], xy[1])
        rig.h.positions_changed()
        px, py, lp = rig.state()
        same_bits(px, xy[0], 'POS_X'); same_bits(py, xy[1], 'POS_Y')
        assert lp.shape == (b, n, 4)
        same_bits(lp, rig.rows(xy[0], xy[1]), f'{shape} {links} B={b}')
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------------- flags_or_kernel
FLAG_B = 16384 + 257
FLAG_ENVS = (0, 63, 64, 255, 256, 16383, 16384, FLAG_B - 1)
FLAG_WORDS = (1, 2, 4, 8, 0x80000000)


@pytest.mark.parametrize('how', ['bound', 'uploaded'])
def test_status_flags_is_the_or_of_every_env(native, how):
    """16 641 envs: flags_or_kernel's 64 workgroups take a second trip for the envs from 16 384 on.  One non-zero env at a time."""
    from gym_d2d_amd.simulator import Simulator
    sim = Simulator(dict(num_cues=1, num_due_pairs=0, num_envs=FLAG_B))
    h = sim.handle
    guard = None
    try:
        if how == 'bound':
            guard = Guarded((FLAG_B,), torch.int32)
            guard.array.zero_()
            torch.cuda.synchronize()
            h.bind_buffer(native.BUF_ENV_FLAGS, guard.array.data_ptr(), guard.nbytes)

        def put(words):
            if guard is not None:
                guard.array.zero_()
                for e, v in words.items():
                    guard.array[e] = v - (1 << 32) if v >= 1 << 31 else v
                torch.cuda.synchronize()
            else:
                a = np.zeros(FLAG_B, dtype=np.uint32)
                for e, v in words.items():
                    a[e] = v
                h.upload(native.BUF_ENV_FLAGS, a.view(np.int32))

        put({})
        assert h.status_flags() == 0
        for e in FLAG_ENVS:
            for v in FLAG_WORDS:
                put({e: v})
                assert h.status_flags() == v, (e, hex(v))
        put({63: 1, 16384: 4, FLAG_B - 1: 0x80000000})
        assert h.status_flags() == 0x80000005
        put({0: 2, 256: 8, 16383: 2})
        assert h.status_flags() == 10
        put({})
        assert h.status_flags() == 0
        if guard is not None:
            assert guard.intact()
    finally:
        h.close()

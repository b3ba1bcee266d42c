"""The cases of test_gpu_mobility_direct.py and test_gpu_queue_direct.py (mobility_direct_util.CASES, queue_direct_util.CASES) on
their references alone, without a GPU: every case exercises what its `why` claims, stays inside the caps (53 287 threads for the move
kernel, 17 219 for the queue kernel, at most 1 % of the devices left out, every plane value below 2^31), and the per-env clock's
schedule feeds the words the header's formulas name.

Counted here on the restatements (ten steps, either tether rule): small_cell leaves out 0.079 % of its devices at most, with 75 892
wall hits (27 041 of them receivers') and 107 348 tether hits; many_envs leaves out 0.065 %, odd 0.032 %, every other case nothing;
`limits` draws k = 64 five times in 80 steps, serves bits of age 31, holds 2 147 483 584 in a plane and reaches a served x delay
product of 2.07e10; of the 16 951 hand-laid pairs of `parted` the wall's rounding parts 137 and the second tether test fires for 323."""
import numpy as np
import pytest

import mobility_direct_util as mdu
import mobility_util as mob
import queue_direct_util as qdu
import queue_util as qu

RULES = ('model_as_stated', 'kernel_rule')


def _reciprocal(units, total):
    """The kernel's index split over every thread: (estimate exact, corrected) counts, and that the corrected pair is right."""
    magic = 0xFFFFFFFF if units == 1 else (1 << 32) // units
    gid = np.arange(total, dtype=np.uint64)
    b = (gid * np.uint64(magic)) >> np.uint64(32)
    u = gid - b * np.uint64(units)
    short = u >= units
    b, u = b + short, u - short * np.uint64(units)
    assert np.array_equal(b, gid // np.uint64(units)) and np.array_equal(u, gid % np.uint64(units))
    return int((~short).sum()), int(short.sum())


# ---------------------------------------------------------------------------------------------- mobility
@pytest.mark.parametrize('name', list(mdu.CASES))
def test_mobility_case_has_the_shape_it_claims_and_stays_inside_the_caps(name):
    s = mdu.spec(name)
    threads = s['b'] * s['units']
    assert threads <= mdu.MAX_THREADS and s['first_env'] + s['b'] <= 2 ** 32 and max(s['ts']) < 65536 and len(s['why']) > 20
    exact, short = _reciprocal(s['units'], threads)
    power_of_two = s['units'] & (s['units'] - 1) == 0
    if s['units'] == 1:
        assert (exact, short) == (1, threads - 1)                     # every thread beyond 0 takes the correction
    else:
        assert (short == 0) == power_of_two                           # an exact reciprocal never takes it; the others do somewhere
    want = {'bs_only': (300, 1, 1), 'one_pair': (2050, 2, 3), 'one_cue': (2050, 2, 2), 'wg_units': (2304, 256, 256),
            'odd': (17219, 257, 510), 'small_cell': (17219, 257, 510), 'many_envs': (53287, 13, 20), 'masks': (627, 19, 31),
            'counter_edge': (126, 14, 21), 'clock': (224, 14, 21)}[name]
    assert (threads, s['units'], s['d']) == want
    if name == 'one_pair':
        assert s['cues'] == 0
    if name == 'one_cue':
        assert s['pairs'] == 0
    if name in ('odd', 'small_cell'):
        assert threads % 256 != 0 and s['units'] % 256 != 0
    if name == 'many_envs':
        assert -(-threads // 256) == 209 and all(s['b'] % p for p in range(2, 65))
    if name == 'counter_edge':
        assert s['first_env'] + s['b'] == 2 ** 32 and s['episode'] == 2 ** 32 - 1 and s['ts'][-1] == 65535
    if name == 'clock':
        assert s['first_env'] + s['b'] == 2 ** 32 and s['b'] == mdu.CLOCK_B
    assert s['small'] == (name in ('small_cell', 'many_envs'))


@pytest.mark.parametrize('name', list(mdu.CASES))
def test_mobility_layout_is_float32_inside_the_cell_and_every_pair_inside_its_tether(name):
    s = mdu.spec(name)
    pos = mdu.start_positions(name)
    assert pos.dtype == np.float32 and pos.shape == (s['b'], s['d'], 2)
    p = pos.astype(np.float64)
    assert np.hypot(p[..., 0], p[..., 1]).max() <= s['cell']
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    if s['pairs']:
        assert np.hypot(*np.moveaxis(p[:, tx + 1] - p[:, tx], -1, 0)).max() <= s['d2d']
    assert (name == 'bs_only') == bool(p[:, 0].any())                 # the base station: at the origin, but where it is the only device


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('name', [n for n in mdu.CASES if n != 'clock'])
def test_mobility_reference_can_judge_the_case(name, rule):
    s = mdu.spec(name)
    tr = mdu.trajectory(name, rule)
    worst = max(float(out.mean()) for _, _, out in tr['steps'])
    print(f'{name} ({rule}): left out {worst:.4%} at most, hits {tr["hits"]}, receivers pulled onto the wall {tr["rx_wall_hits"]}')
    assert len(tr['steps']) == mdu.STEPS and worst <= mdu.LEFT_OUT_CAP
    pos0 = mdu.start_positions(name).astype(np.float64)
    if name == 'bs_only':
        assert not tr['vel0'].any() and all(np.array_equal(p, pos0) and not v.any() for p, v, _ in tr['steps'])
        return
    moved = ~mdu.fixed_mask(name)[0]
    assert all((p[:, moved] != pos0[:, moved]).any(axis=-1).all() for p, _, _ in tr['steps'])
    assert tr['hits']['wall'] > 0
    assert (tr['hits']['tether'] > 0) == (s['pairs'] > 0)
    if name == 'small_cell':
        assert tr['rx_wall_hits'] >= 10000
        assert s['cell'] == 40.0 and s['d2d'] == 20.0 and s['model'] == dict(speed_std_mps=9.0, memory=0.5, dt_s=1.5)


def test_mobility_masks_pin_one_of_each_kind_and_the_restatement_honours_them():
    s = mdu.spec('masks')
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    pinned = set(mdu.PINNED)
    assert 0 in pinned and any(1 <= d <= s['cues'] for d in pinned)
    assert any(d in pinned and d + 1 not in pinned for d in tx) and any(d + 1 in pinned and d not in pinned for d in tx)
    assert any(d in pinned and d + 1 in pinned for d in tx)
    assert mdu.fixed_mask('masks', 'null')[1] is None and not mdu.fixed_mask('masks', 'zeros')[1].any()
    assert mdu.fixed_mask('masks', 'ones')[1].all() and sorted(np.flatnonzero(mdu.fixed_mask('masks', 'pinned')[1])) == sorted(pinned)
    pos0 = mdu.start_positions('masks').astype(np.float64)
    null, zeros = mdu.trajectory('masks', 'kernel_rule', 'null'), mdu.trajectory('masks', 'kernel_rule', 'zeros')
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(null['steps'], zeros['steps']))
    for rule in RULES:
        ones = mdu.trajectory('masks', rule, 'ones')
        assert not ones['vel0'].any() and all(np.array_equal(p, pos0) and not v.any() for p, v, _ in ones['steps'])
        pin = mdu.trajectory('masks', rule, 'pinned')
        fixed = mdu.fixed_mask('masks', 'pinned')[0]
        assert max(float(out.mean()) for _, _, out in pin['steps']) <= mdu.LEFT_OUT_CAP
        for p, v, _ in pin['steps']:
            assert np.array_equal(p[:, fixed], pos0[:, fixed]) and not v[:, fixed].any()
            assert (p[:, ~fixed] != pos0[:, ~fixed]).any(axis=-1).all()
        # the transmitter of the pinned receiver is the tethered one: it stays within d2d of where the receiver stands
        d = np.hypot(*np.moveaxis(pin['steps'][-1][0][:, 17] - pos0[:, 18], -1, 0))
        assert d.max() <= s['d2d'] * (1 + 1e-12)


def test_mobility_bars_are_the_counted_ones():
    for name in mdu.CASES:
        s = mdu.spec(name)
        for t in (1, 10):
            bar = mdu.bar_ulp(name, t)
            if not s['small']:
                assert (bar == 4.0).all()
                continue
            extra = s['model']['dt_s'] * 1e-6 * s['model']['speed_std_mps'] * (t + 1) / 2 / mob.ulp32(s['cell'])
            rx = np.zeros(s['d'], dtype=bool)
            rx[2 + s['cues']::2] = True
            assert np.allclose(bar[rx], 14.0 + extra) and np.allclose(bar[~rx], 4.0 + extra)
    assert mob.ulp32(40.0) == mob.ulp32(60.0) == 2.0 ** -18
    assert abs(mdu.bar_ulp('small_cell', 10)[-1] - (14.0 + 19.46)) < 0.01 and abs(mdu.bar_ulp('many_envs', 10)[1] - (4.0 + 8.65)) < 0.01


def test_parted_state_is_one_the_kernel_could_have_left_and_the_wall_parts_enough_of_its_pairs():
    """The path no drawn case reaches (a wall overshoot of a few ulp is a 1e-5 event per wall hit, and a larger one shortens the
    pair by more than any rounding lengthens it): laid out by hand, judged by the kernel's own operations in float32."""
    s, pos = mdu.spec('parted'), mdu.parted_positions().astype(np.float64)
    tx = 1 + s['cues'] + 2 * np.arange(s['pairs'])
    radius = np.hypot(pos[..., 0], pos[..., 1])
    assert pos.shape == (s['b'], s['d'], 2) and s['b'] * s['units'] <= mdu.MAX_THREADS
    assert (radius[:, tx + 1] > s['cell']).all() and radius.max() <= s['cell'] * mdu.TOL22 and (radius[:, tx] < s['cell']).all()
    assert np.hypot(*np.moveaxis(pos[:, tx + 1] - pos[:, tx], -1, 0)).max() <= s['d2d'] * mdu.TOL22
    assert mob.constants(**s['model'])[1:3] == (0.0, 0.0)                                    # no noise, no speed: nothing moves
    r = mdu.parted_by_the_wall()
    count = {k: int(v.sum()) for k, v in r.items()}
    print(f'parted: of {r["wall"].size} pairs {count}')
    assert r['before'].all() and count['wall'] > 16000
    assert count['parted'] >= 100 and (r['again'] | ~r['parted']).all() and r['mended'].all()
    assert count['first'] < r['wall'].size // 10                      # most pairs reach the wall untouched by the first tether test


# ---------------------------------------------------------------------------------------------- the per-env clock
def test_clock_schedule_feeds_what_the_header_names():
    sched = mdu.clock_schedule()
    assert len(sched) == mdu.CLOCK_LAUNCHES == 31 and mdu.CLOCK_FIRST_ENV + mdu.CLOCK_B == 2 ** 32
    first = sched[0]
    assert first['flagged'].all() and (first['reset'] != 0).all() and len(set(first['reset'].tolist())) > 4
    assert first['start'].all() and not first['start_after'].any() and not first['own_t'].any()
    assert np.array_equal(sched[1]['start'], np.arange(16) % 5) and np.array_equal(sched[1]['elapsed'], np.arange(16) % 5)
    flagged = {k + 1: tuple(np.flatnonzero(s['flagged'])) for k, s in enumerate(sched) if s['flagged'].any()}
    assert flagged == {1: tuple(range(16)), 12: (0, 3, 5, 10), 13: (3,)}
    stepping_episodes, reset_episodes = set(), set()
    t = np.zeros(16, dtype=np.int64)
    for k, s in enumerate(sched, start=1):
        f = s['flagged']
        # the header's two formulas, in the kernel's own unsigned arithmetic
        want_t = np.where(f, 0, (s['elapsed'].astype(np.int64) - s['start'] + 1) % 2 ** 32)
        want_e = np.where(f, s['episode'].astype(np.int64), (s['episode'].astype(np.int64) - 1) % 2 ** 32)
        assert np.array_equal(s['own_t'], want_t) and np.array_equal(s['own_episode'].astype(np.int64), want_e)
        t = np.where(f, 0, t + 1)
        assert np.array_equal(s['own_t'], t), k                        # every env advances by one step per launch, or restarts
        assert np.array_equal(s['reset'] != 0, f) and np.array_equal(s['start_after'], np.where(f, 0, s['start']))
        if k == 12:
            assert (s['start'][f] != 0).any() and (s['start'][~f] != 0).any()      # a stagger to lose, and staggers to keep
        stepping_episodes |= set(s['own_episode'][~f].tolist()); reset_episodes |= set(s['own_episode'][f].tolist())
        assert (s['episode'][~f] == (s['own_episode'][~f].astype(np.int64) + 1) % 2 ** 32).all()
    assert {0, 2 ** 32 - 1} <= stepping_episodes and {0, 2 ** 32 - 1} <= reset_episodes
    assert any(1 in s['episode'][~s['flagged']].tolist() for s in sched)          # a stepping env READS 1 and stands in episode 0
    assert any(0 in s['episode'][~s['flagged']].tolist() for s in sched)          # ... reads 0 and stands in 2^32 - 1
    garbage = [int(s['elapsed'][e]) for s in sched for e in np.flatnonzero(s['flagged'])]
    assert min(garbage) == -2 ** 31 and max(garbage) == 2 ** 31 - 1


@pytest.mark.parametrize('rule', RULES)
def test_clock_mobility_reference_can_judge_the_case(rule):
    tr = mdu.clock_trajectory(rule)
    sched = mdu.clock_schedule()
    assert len(tr) == 31
    worst = max(float(k['out'].mean()) for k in tr)
    print(f'clock ({rule}): left out {worst:.4%} at most, hits {tr[-1]["hits"]}')
    assert worst <= mdu.LEFT_OUT_CAP and tr[-1]['hits']['tether'] > 0
    for k, s in zip(tr, sched):
        f = s['flagged']
        assert np.array_equal(k['pos'][f], k['fresh'][f].astype(np.float64)) and np.array_equal(k['t'], s['own_t'])
    assert not np.array_equal(tr[11]['fresh'][3], tr[12]['fresh'][3])            # two resets in a row, two layouts


# ---------------------------------------------------------------------------------------------- queue
@pytest.mark.parametrize('name', list(qdu.CASES))
def test_queue_case_exercises_what_it_claims_and_stays_inside_the_caps(name):
    s = qdu.spec(name)
    launches, stats = qdu.program(name)
    threads = s['b'] * s['n']
    print(f'{name}: B={s["b"]} N={s["n"]} D={s["d"]} launches={len(launches)}: {stats}')
    assert threads <= qdu.MAX_THREADS and s['first_env'] + s['b'] <= 2 ** 32 and len(s['why']) > 20
    exact, short = _reciprocal(s['n'], threads)
    if s['n'] == 1:
        assert (exact, short) == (1, threads - 1)
    else:
        assert (short == 0) == (s['n'] & (s['n'] - 1) == 0)
    want = {'one_link': (300, 1), 'due_only': (2112, 64), 'wg_links': (2304, 256), 'odd': (17219, 257), 'clock': (2096, 131)}
    assert (threads, s['n']) == want.get(name, (655, 131))
    for k in qdu.EVENTS:
        assert (stats['events'][k] == 0) if k in qdu.NEVER.get(name, ()) else (stats['events'][k] > 0), (k, stats['events'])
    assert stats['max_plane'] < 2 ** 31 and stats['max_served_age'] <= s['d'] - 1
    for launch in launches:
        for k, v in launch['want'].items():
            assert v.dtype == (np.float32 if k == 'mean_delay_steps' else np.uint8 if k == 'on' else np.int32), k
            assert v.shape == ((s['d'], s['b'], s['n']) if k == 'ring' else (s['b'], s['n']))
    r = qdu.restatement(name, 1)
    if name == 'one_link':
        cap = launches[1]['capacity']
        assert cap.shape == (300, 1) and np.isnan(cap).any() and np.isinf(cap).any() and (cap == 0).any() and (cap > 0).sum() > 100
        assert s['cues'] == 1 and s['pairs'] == 0
    if name == 'due_only':
        assert s['cues'] == 0
    if name == 'always_on':
        assert r.thr_off == 0 and all(launch['want']['on'].all() for launch in launches)
    if name == 'p_one':
        assert r.thr_off == r.thr_on == qu.U32 and 0 < r.thr_start < qu.U32
    if name.startswith('no_buffer'):
        assert r.buffer_bits < r.packet_bits and (r.buffer_bits == 0) == (name == 'no_buffer_0')
        for launch in launches:
            w = launch['want']
            assert not w['ring'].any() and not w['backlog_bits'].any() and not w['served_bits'].any()
            assert np.array_equal(w['overflow_bits'], w['arrived_bits'])
        assert sum(int(launch['want']['arrived_bits'].astype(np.int64).sum()) for launch in launches) > 0
    if name == 'limits':
        assert r.packet_bits == 2 ** 25 - 1 and r.buffer_bits == 2 ** 31 - 1 and r.rates == (40.0, 12.0) and s['d'] == 32 and len(s['ts']) == 80
        assert stats['k64'] >= 1 and stats['max_product'] > 2 ** 32 and stats['max_backlog'] > 2 ** 31 - 2 ** 26
        assert stats['max_served_age'] == 31
        budgets = qu.budget_bits(np.array(qdu.LIMIT_MBPS, dtype=np.float32), r.bits_per_mbps_step)
        assert budgets.tolist() == list(qdu.LIMIT_BUDGETS[:4])
        assert float(np.float32(qdu.LIMIT_MBPS[1])) * r.bits_per_mbps_step == 2147483750.0       # clipped only after float32's rounding
        assert float(np.float32(qdu.LIMIT_MBPS[3])) * r.bits_per_mbps_step == 3e9                # finite, and it saturates
        cap = launches[5]['capacity']
        assert np.isinf(cap[:, 4::7]).any() and 0 < cap[:, 5::7].max() <= 6.0 * r.packet_bits / r.bits_per_mbps_step
    if name in ('wrap31', 'wrap32'):
        ts = [launch['step'] for launch in launches]
        assert ts[0] == 0 and s['episode'] == 2 ** 32 - 1 and s['first_env'] + s['b'] == 2 ** 32 and len(ts) == 13
        assert ts[1:] == (list(range(2 ** 31 - 5, 2 ** 31 + 7)) if name == 'wrap31' else list(range(2 ** 32 - 12, 2 ** 32)))
        # a signed step counter picks another slot, also where the negative remainder is put back into range
        assert any((t - 2 ** 32) % s['d'] != t % s['d'] for t in ts if t >= 2 ** 31)
    if name == 'clock':
        assert len(launches) == 31 and all(launch['clock'] is k for launch, k in zip(launches, mdu.clock_schedule()))
        assert not any(v.any() for k, v in launches[0]['want'].items() if k != 'on') and launches[0]['want']['on'].any()
        after = launches[11]['want']
        assert not after['ring'][:, [0, 3, 5, 10]].any() and after['ring'][:, [1, 2, 4]].any()


def test_queue_cases_are_the_issue_s_table():
    assert list(qdu.CASES) == ['one_link', 'due_only', 'wg_links', 'odd', 'limits', 'wrap31', 'wrap32', 'always_on', 'p_one', 'no_buffer',
                               'no_buffer_0', 'clock']
    assert list(mdu.CASES) == ['bs_only', 'one_pair', 'one_cue', 'wg_units', 'odd', 'small_cell', 'many_envs', 'masks', 'counter_edge',
                               'clock']
    assert qdu.BASE == dict(packets_per_step=(2.0, 0.7), packet_bits=1000, buffer_bits=5007, dt_s=1e-3, p_on_to_off=0.2, p_off_to_on=0.3)

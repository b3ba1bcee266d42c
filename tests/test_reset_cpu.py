"""The reset tests' restatement and case tables (reset_util) without a GPU: the restatement equals oracle.sample_positions_from_uniforms
operation for operation wherever that sampler answers, states the exhausted receiver itself, and can judge every case
test_gpu_reset_direct.py gives the kernels - the ambiguity cap and the coverage each case claims hold on the restatement alone, and
the host's multiply-high division estimate is short exactly where the table says."""
import numpy as np
import pytest

import reset_util as ru
from oracle import d2d_oracle as orc


def _receivers(name):
    s = ru.spec(name)
    return ru.receivers(s['cues'], s['d'])


@pytest.mark.parametrize('name', ru.FULL)
def test_the_case_is_what_its_row_says(name):
    s, ref = ru.spec(name), ru.reference(name)
    assert ref.pos.shape == (s['b'], s['d'], 2) and ref.tries.shape == ref.exhausted.shape == ref.ambiguous.shape == (s['b'], s['d'])
    assert (ref.pos[:, 0] == 0.0).all() and (ref.tries[:, 0] == 0).all()
    rx = _receivers(name)
    others = np.setdiff1d(np.arange(s['d']), rx)
    assert not ref.exhausted[:, others].any() and not ref.ambiguous[:, others].any()
    assert (np.hypot(ref.pos[..., 0], ref.pos[..., 1]) <= s['cell']).all()
    pins = {k: v for k, v in (s['pins'] or {}).items() if k}
    for k, xy in pins.items():
        assert (ref.pos[:, k] == np.asarray(xy)).all() and (ref.tries[:, k] == 0).all()
        assert np.hypot(*xy) < s['cell']
    drawn = np.array([k for k in rx if k not in pins], dtype=np.int64)
    if drawn.size:
        tx = ref.pos[:, drawn - 1]
        dist = np.hypot(*np.moveaxis(ref.pos[:, drawn] - tx, -1, 0))
        assert (dist <= s['d2d']).all()
        assert ((dist == 0.0) == ref.exhausted[:, drawn]).all()             # the open radius interval: never 0 unless exhausted
        assert (ref.tries[:, drawn][ref.exhausted[:, drawn]] == ru.TRIES).all()


@pytest.mark.parametrize('name', ru.FULL)
def test_at_most_one_receiver_in_a_thousand_is_ambiguous(name):
    s, ref = ru.spec(name), ru.reference(name)
    n_rx = s['b'] * s['pairs']
    assert int(ref.ambiguous.sum()) <= ru.AMBIGUOUS_CAP * n_rx, (name, int(ref.ambiguous.sum()), n_rx)


@pytest.mark.parametrize('shape', ru.MASKED_SHAPES)
@pytest.mark.parametrize('b', ru.MASKED_B)
def test_the_masked_cases_stay_under_the_ambiguity_cap_and_never_exhaust(shape, b):
    s = ru.spec(shape)
    pending, episode = ru.pending_and_episodes(b)
    ref = ru.restate(ru.SEED, episode, b, s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV)
    assert int(ref.ambiguous.sum()) <= ru.AMBIGUOUS_CAP * b * s['pairs'] and not ref.exhausted.any()
    assert pending[b - 1] != 0 and set(pending.tolist()) <= {0, 1, -1, 7}
    share = (pending != 0).mean()
    assert b == 1 or 0.25 <= share <= 0.45, share
    assert len(set(episode.tolist())) == b and episode[b - 1] == 2 ** 32 - 1
    if b > 1:
        assert pending[0] == 0 and pending[1] != 0 and episode[1] == 0 and episode[0] not in episode[pending != 0]


@pytest.mark.parametrize('name', [n for n in ru.FULL if n not in ('late', 'exhaust')])
def test_the_restatement_equals_the_oracle_sampler_where_nothing_exhausts(name):
    s, ref = ru.spec(name), ru.reference(name)
    assert not ref.exhausted.any()
    u = ru.uniforms(ru.SEED, s['episode'], s['b'], s['d'], ru.TRIES, s['first_env'])
    pins = {k: v for k, v in (s['pins'] or {}).items() if k}                # the oracle would pin device 0 too: the kernel ignores it
    pos, used = orc.sample_positions_from_uniforms(u, s['cues'], s['pairs'], s['cell'], s['d2d'], fixed=pins or None)
    np.testing.assert_array_equal(ref.pos, pos)
    np.testing.assert_array_equal(ref.tries, used)


@pytest.mark.parametrize('name', ['late', 'exhaust'])
def test_the_oracle_sampler_refuses_what_the_restatement_states(name):
    s, ref = ru.spec(name), ru.reference(name)
    u = ru.uniforms(ru.SEED, s['episode'], s['b'], s['d'], ru.TRIES, s['first_env'])
    with pytest.raises(RuntimeError, match='ran out of tries'):
        orc.sample_positions_from_uniforms(u, s['cues'], s['pairs'], s['cell'], s['d2d'])
    rx = _receivers(name)
    ex = ref.exhausted[:, rx]
    np.testing.assert_array_equal(ref.pos[:, rx][ex], ref.pos[:, rx - 1][ex])
    # a receiver that does not exhaust is the oracle's with the tries it needed, env by env where the whole env does not exhaust
    whole = ~ex.any(axis=1)
    for b in np.flatnonzero(whole):
        pos, used = orc.sample_positions_from_uniforms(u[b:b + 1], s['cues'], s['pairs'], s['cell'], s['d2d'])
        np.testing.assert_array_equal(ref.pos[b], pos[0])


def test_coverage_the_rows_name():
    tries = lambda name: ru.reference(name).tries[:, _receivers(name)]
    late, ex = ru.reference('late'), ru.reference('exhaust')
    assert int((tries('late') >= 16).sum()) >= 100 and int(late.exhausted.sum()) >= 100
    assert int((tries('late') >= 16).sum()) == 922 and int(late.exhausted.sum()) == 447 and tries('late').size == 1170
    assert ex.exhausted[:, _receivers('exhaust')].all() and int(ex.exhausted.sum()) == 198
    big = tries('big_d2d')
    assert (big > 1).mean() >= 0.25
    assert int((big > 1).sum()) == 653 and big.size == 1320 and int(big.max()) == 12
    # pinned: the receiver of the transmitter pinned on the cell edge redraws in some env; the pinned receiver never draws
    assert (ru.reference('pinned').tries[:, 12] > 1).any() and (ru.reference('pinned').tries[:, 42] == 0).all()
    assert (ru.reference('pinned_cues').tries[:, 8] > 1).any()
    # first_env_wrap: envs 3..7 are envs 0..4 of first_env 0
    s = ru.spec('first_env_wrap')
    zero = ru.restate(ru.SEED, s['episode'], 5, s['cues'], s['pairs'], s['cell'], s['d2d'], 0)
    np.testing.assert_array_equal(ru.reference('first_env_wrap').pos[3:], zero.pos)
    last = ru.restate(ru.SEED, s['episode'], 3, s['cues'], s['pairs'], s['cell'], s['d2d'], 2 ** 32 - 3)
    np.testing.assert_array_equal(ru.reference('first_env_wrap').pos[:3], last.pos)
    assert not np.array_equal(zero.pos[:3], last.pos)


@pytest.mark.parametrize('name', ru.FULL)
def test_the_division_estimate_is_short_exactly_where_the_table_says(name):
    s = ru.spec(name)
    magic, est, short, env, unit = ru.division(s['b'], s['units'])
    assert magic == (0xFFFFFFFF if s['units'] == 1 else 2 ** 32 // s['units']) and 0 < magic < 2 ** 32
    assert len(est) == s['b'] * s['units'] < 0xFFFFFF00
    for g in range(len(est)):
        assert est[g] in (g // s['units'], g // s['units'] - 1) and short[g] == (est[g] != g // s['units'])
        assert (env[g], unit[g]) == divmod(g, s['units'])
    assert sum(short) == s['corrected'], (name, sum(short))


def test_the_division_estimate_of_one_unit_per_env():
    magic, est, short, env, unit = ru.division(300, 1)                      # units == 1: the 0xFFFFFFFF reciprocal
    assert magic == 0xFFFFFFFF and sum(short) == 299 and env == list(range(300)) and set(unit) == {0}


@pytest.mark.parametrize('shape', ru.MASKED_SHAPES)
def test_an_episode_vector_gives_env_by_env_what_the_scalar_episode_gives(shape):
    s = ru.spec(shape)
    b = 9
    _, episode = ru.pending_and_episodes(b)
    vec = ru.restate(ru.SEED, episode, b, s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV)
    for e in range(b):
        one = ru.restate(ru.SEED, int(episode[e]), b, s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV)
        for got, want in zip(vec, one):
            np.testing.assert_array_equal(got[e], want[e])
    same = ru.restate(ru.SEED, np.full(b, ru.EPISODE, dtype=np.uint32), b, s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV)
    for got, want in zip(same, ru.restate(ru.SEED, ru.EPISODE, b, s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV)):
        np.testing.assert_array_equal(got, want)


def test_pins_as_the_kernel_is_given_them():
    s = ru.spec('pinned')
    mask, xy = ru.mask_xy(s['pins'], s['d'])
    assert mask.dtype == np.uint8 and xy.dtype == np.float32 and mask[0] == 1 and int(mask.sum()) == 5
    # a pin on device 0 changes nothing
    without = ru.restate(ru.SEED, ru.EPISODE, s['b'], s['cues'], s['pairs'], s['cell'], s['d2d'], ru.FIRST_ENV,
                         {k: v for k, v in s['pins'].items() if k})
    np.testing.assert_array_equal(without.pos, ru.reference('pinned').pos)
    # and only the pinned devices and the receiver of the pinned transmitter differ from the unpinned case of the same shape
    diff = (ru.reference('pinned').pos != ru.reference('wave_plus_one').pos).any(axis=(0, 2))
    assert set(np.flatnonzero(diff).tolist()) == {11, 12, 42, 81, 82}

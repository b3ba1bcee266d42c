"""episode_util.py on its own, no GPU: merge_ref against envs/_rng.py's per-env stream and against plain Python integers, advance_ref
against a per-env Python loop over consecutive steps, and the shape lists against the kernel paths they exist for
(csrc/d2d_episode.hip: 16-byte vectors of four, the tail lane, the capped grid, waves of 64 in workgroups of 256)."""
import numpy as np
import pytest

import episode_util as eu

MASK = 2 ** 64 - 1


def _py_mix(x):
    x = ((x ^ (x >> 30)) * eu.M1) & MASK
    x = ((x ^ (x >> 27)) * eu.M2) & MASK
    return x ^ (x >> 31)


def _py_draw(seed, episode, first_env, b, c, n_cols, high):
    key = _py_mix(_py_mix(seed & MASK) ^ (((episode + 1) * eu.GOLDEN) & MASK))
    x = (key + ((((first_env + b) & MASK) * n_cols + c + 1) & MASK) * eu.GOLDEN) & MASK
    return (_py_mix(x) >> 11) % high


@pytest.mark.parametrize('seed', eu.SEEDS)
@pytest.mark.parametrize('first_env', eu.FIRST_ENVS)
@pytest.mark.parametrize('n_envs,n_cols', eu.MERGE_SHAPES)
def test_merge_ref_equals_the_per_env_stream_and_python_integers(n_envs, n_cols, first_env, seed):
    from gym_d2d_amd.envs import _rng
    rng = np.random.default_rng(1)
    for pattern in eu.PENDING_PATTERNS:
        c = eu.build_merge_case(n_envs, n_cols, pattern, first_env, seed)
        got = eu.merged(n_envs, n_cols, pattern, first_env, seed)
        assert got.shape == (n_envs, n_cols) and got.dtype == np.int32
        draws = _rng.uniform_ints_numpy_per_env(seed, c['episode'], first_env, n_cols, c['high'])
        mask = c['pending'] != 0
        np.testing.assert_array_equal(got[mask], draws[mask])
        np.testing.assert_array_equal(got[~mask], c['actions_in'][~mask])
        assert (got[mask] >= 0).all() and (got[mask] < c['high'][None, :].astype(np.int64)).all()
        for k in rng.integers(0, n_envs * n_cols, 200):
            b, col = divmod(int(k), n_cols)
            want = _py_draw(seed, int(c['episode'][b]), first_env, b, col, n_cols, int(c['high'][col])) if mask[b] \
                else int(c['actions_in'][b, col])
            assert int(got[b, col]) == want, (pattern, b, col)


def test_the_seeded_inputs_are_what_the_cases_claim():
    c = eu.build_merge_case(33, 13, 'random')
    assert c['actions_in'].min() < -2 ** 30 and c['actions_in'].max() > 2 ** 30
    assert (c['high'] >= 1).all() and 1 in c['high'] and c['high'][-1] == eu.INT32_MAX
    assert sorted(c['high'])[-2] < 5000
    assert {0, 1, 0xFFFFFFFF} <= set(c['episode'].tolist())
    share = float((c['pending'] != 0).mean())
    assert 0.1 < share < 0.5
    assert set(np.unique(c['pending'])) - {0, 1}                     # some non-zero value that is not 1
    want = {'none': [0, 0, 0, 0, 0], 'all': [1, 1, 1, 1, 1], 'first': [1, 0, 0, 0, 0], 'last': [0, 0, 0, 0, 1],
            'alternating': [0, 1, 0, 1, 0]}
    for pattern, p in want.items():
        assert eu.pending_pattern(pattern, None, 5).tolist() == p
    cycled = {(eu.build_merge_case(b, a, p)['first_env'], eu.build_merge_case(b, a, p)['seed'])
              for b, a in eu.MERGE_SHAPES for p in eu.PENDING_PATTERNS}
    assert {f for f, _ in cycled} == set(eu.FIRST_ENVS) and {s for _, s in cycled} == set(eu.SEEDS)
    state = eu.random_advance_state(257, 65)
    assert state['elapsed'].min() == 0 and state['elapsed'].max() == 12
    mid = 257 // 2
    assert state['episode'][mid] == 0xFFFFFFFF and state['pending'][mid] != 0
    assert eu.advance_ref(state, 10)['episode'][mid] == 0
    bits = state['reward'].view(np.uint32)
    assert np.isnan(state['reward']).any() and (bits == 0x80000000).any()
    lone = [int(eu.random_advance_state(1, r, salt=k)['pending'][0] != 0) for k, r in enumerate(eu.REWARD_COLS)]
    assert 0 in lone and 1 in lone                                   # the single env takes either branch over the reward widths


def _py_advance(state, length):
    """The header's two branches, one env at a time, in place."""
    for b in range(len(state['pending'])):
        if state['pending'][b] != 0:
            state['elapsed'][b] = 0
            state['episode'][b] = (int(state['episode'][b]) + 1) % 2 ** 32
            state['pending'][b] = 0
            state['reset_out'][b] = 1
            state['done'][b] = 0
            if state['reward'] is not None:
                for i in range(state['reward'].shape[1]):
                    state['reward'][b, i] = 0.0
        else:
            state['elapsed'][b] += 1
            state['done'][b] = 1 if state['elapsed'][b] >= length else 0
            state['pending'][b] = state['done'][b]
            state['reset_out'][b] = 0


@pytest.mark.parametrize('n_envs,reward_cols,length', [(65, None, 10), (257, 65, 10), (63, 1, 1), (1, 50, 3)])
def test_advance_ref_equals_a_per_env_loop_over_25_steps(n_envs, reward_cols, length):
    rng = np.random.default_rng(2)
    state = eu.staggered_advance_state(n_envs, reward_cols, rng)
    assert state['elapsed'].tolist() == [b % 10 for b in range(n_envs)]
    loop = {k: None if v is None else v.copy() for k, v in state.items()}
    resets = 0
    for t in range(25):
        fresh = eu.random_reward(rng, n_envs, reward_cols)
        state['reward'] = fresh
        loop['reward'] = None if fresh is None else fresh.copy()
        arg, before = state, {k: None if v is None else v.copy() for k, v in state.items()}
        state = eu.advance_ref(arg, length)
        _py_advance(loop, length)
        for k, v in before.items():                                  # the argument is left as it was
            assert v is None or np.array_equal(v.view(np.uint8), arg[k].view(np.uint8)), k
        for k, v in state.items():
            if v is None:
                assert loop[k] is None
            else:
                assert v.dtype == loop[k].dtype and np.array_equal(v.view(np.uint8), loop[k].view(np.uint8)), (t, k)
        resets += int(state['reset_out'].sum())
    assert resets >= 2 * n_envs                                      # every env was reset at least twice


def test_advance_ref_wraps_the_episode_and_writes_plus_zero():
    state = dict(pending=np.array([1, 0, -5], dtype=np.int32), episode=np.array([0xFFFFFFFF, 0xFFFFFFFF, 6], dtype=np.uint32),
                 elapsed=np.array([4, 8, 12], dtype=np.int32), done=np.array([7, 7, 7], dtype=np.uint8),
                 reset_out=np.array([9, 9, 9], dtype=np.uint8),
                 reward=np.array([[np.nan, -0.0], [-0.0, np.nan], [1.5, -2.5]], dtype=np.float32))
    out = eu.advance_ref(state, 9)
    assert out['pending'].tolist() == [0, 1, 0] and out['episode'].tolist() == [0, 0xFFFFFFFF, 7]
    assert out['elapsed'].tolist() == [0, 9, 0] and out['done'].tolist() == [0, 1, 0] and out['reset_out'].tolist() == [1, 0, 1]
    assert out['reward'].view(np.uint32).tolist() == [[0, 0], state['reward'].view(np.uint32)[1].tolist(), [0, 0]]
    assert state['pending'].tolist() == [1, 0, -5]


def test_the_shape_lists_keep_their_reasons():
    totals = [b * a for b, a in eu.MERGE_SHAPES]
    assert {t % eu.VEC for t in totals} == {0, 1, 2, 3}
    assert any(t < eu.VEC for t in totals)
    assert {1, 2, 3} <= {a for _, a in eu.MERGE_SHAPES}
    assert any(t // eu.VEC > eu.WORKGROUP for t in totals)
    assert set(eu.SCALAR_SHAPES) <= set(eu.MERGE_SHAPES)
    for cus in (64, 256, 304):
        b, a = eu.grid_stride_shape(cus)
        assert b % 2 == 1 and (b * a) % eu.VEC != 0
        assert b * a // eu.VEC >= eu.grid_cap_vectors(cus) + 4096
        assert eu.grid_cap_vectors(cus) == 32 * cus * 256
        assert (b - 2) * a // eu.VEC < eu.grid_cap_vectors(cus) + 4096            # the smallest odd one
        assert b * a < 2 ** 31
    assert any(b < 64 for b in eu.ADVANCE_ENVS)
    assert any(b > 64 and b % 64 for b in eu.ADVANCE_ENVS)
    assert any(b > 256 for b in eu.ADVANCE_ENVS)
    assert 64 in eu.ADVANCE_ENVS and None in eu.REWARD_COLS and any(r and r > 64 for r in eu.REWARD_COLS)

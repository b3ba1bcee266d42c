"""What the episode tests share (test_episode_cpu.py, test_gpu_episode.py): the restatement of include/d2d_episode.h's two entry
points in NumPy, written from the header and not as calls into envs/_rng.py, the shapes at which csrc/d2d_episode.hip takes its
other paths (merge_kernel: 16-byte vectors, a tail of total % 4 elements by one lane, the scalar route, a grid capped at 32
workgroups per CU; advance_kernel: one lane per env, a wave's ballot for the reward rows), and the seeded inputs.

A merge case is a dict: actions_in int32 [B, A], pending int32 [B], episode uint32 [B], high int32 [A], first_env, seed.  An advance
state is a dict of pending int32, episode uint32, elapsed int32, done uint8, reset_out uint8 (all [B]) and reward (float32
[B, reward_cols] or None).  What build_* and merged() return is cached and read-only."""
from functools import lru_cache

import numpy as np

GOLDEN, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
VEC = 4                             # int32 elements per 16-byte vector
WORKGROUP, WORKGROUPS_PER_CU = 256, 32

# (n_envs, n_cols): total 1 and 3 (fewer than one vector: the tail lane alone), 7 (one vector, tail 3), 10 (tail 2), 27 (tail 3),
# 30 (tail 2), 429 (tail 1), 3200 (no tail, 800 vectors: four workgroups), 7000 (no tail, 1750 vectors); n_cols 1, 2 and 3 put
# three or four envs into one vector, 5, 7 and 13 move the env boundary through every position of a vector
MERGE_SHAPES = [(1, 1), (3, 1), (7, 1), (5, 2), (9, 3), (6, 5), (33, 13), (64, 50), (1000, 7)]
SCALAR_SHAPES = [(7, 1), (33, 13), (1000, 7)]
# one lane; a partly filled only wave; one full wave; a second wave with one live lane; a last wave with lanes past n_envs in a full
# workgroup; a second workgroup with one live lane; four workgroups
ADVANCE_ENVS = (1, 63, 64, 65, 255, 257, 1000)
REWARD_COLS = (None, 1, 50, 64, 65, 200)           # no plane; one word; under a wave; a wave; a wave and one; four passes of the row loop
PENDING_PATTERNS = ('none', 'all', 'first', 'last', 'alternating', 'random')
FIRST_ENVS = (0, 77, 2 ** 32 - 5, 2 ** 40 + 3)
SEEDS = (0, 2 ** 63 + 5)
INT32_MAX = 2 ** 31 - 1


def grid_cap_vectors(cus):
    """The vectors one pass of the capped grid covers: past it the kernels stride."""
    return WORKGROUPS_PER_CU * cus * WORKGROUP


def grid_stride_shape(cus, n_cols=129):
    """The smallest odd n_envs whose vector count exceeds the capped grid by at least 4096 vectors, with a tail."""
    n_envs = ((grid_cap_vectors(cus) + 4096) * VEC + n_cols - 1) // n_cols
    while n_envs % 2 == 0 or n_envs * n_cols // VEC < grid_cap_vectors(cus) + 4096 or n_envs * n_cols % VEC == 0:
        n_envs += 1
    return n_envs, n_cols


# ------------------------------------------------------------------------------------------ the restatements
def _mix(x):
    """splitmix64's finaliser on uint64 arrays, wrapping."""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(M1)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(M2)
    return x ^ (x >> np.uint64(31))


def merge_ref(actions_in, pending, episode, high, first_env, seed):
    """d2d_episode_merge_actions: int32 [B, A]; the rows of pending envs are the reset's draws, every other row the input row."""
    actions_in = np.asarray(actions_in, dtype=np.int32)
    n_envs, n_cols = actions_in.shape
    with np.errstate(over='ignore'):
        seed_mix = _mix(np.array([seed & (2 ** 64 - 1)], dtype=np.uint64))
        key = _mix(seed_mix ^ ((np.asarray(episode).astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)))[:, None]
        env = (np.array([first_env & (2 ** 64 - 1)], dtype=np.uint64) + np.arange(n_envs, dtype=np.uint64))[:, None]
        c = np.arange(n_cols, dtype=np.uint64)[None, :]
        x = key + (env * np.uint64(n_cols) + c + np.uint64(1)) * np.uint64(GOLDEN)
        draw = ((_mix(x) >> np.uint64(11)) % np.asarray(high).astype(np.uint64)[None, :]).astype(np.int32)
    return np.where((np.asarray(pending) != 0)[:, None], draw, actions_in)


def advance_ref(state, episode_length):
    """d2d_episode_advance: the state after one launch, as a new dict (the argument is left as it is)."""
    was_pending = np.asarray(state['pending']) != 0
    elapsed = np.where(was_pending, 0, state['elapsed'].astype(np.int64) + 1).astype(np.int32)
    done = ~was_pending & (elapsed >= episode_length)
    out = dict(pending=done.astype(np.int32),
               episode=((state['episode'].astype(np.uint64) + was_pending.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32),
               elapsed=elapsed, done=done.astype(np.uint8), reset_out=was_pending.astype(np.uint8), reward=None)
    if state['reward'] is not None:
        out['reward'] = np.array(state['reward'], dtype=np.float32)
        out['reward'][was_pending] = 0.0                             # +0.0: all bits clear
    return out


# ------------------------------------------------------------------------------------------ the inputs
def pending_pattern(pattern, rng, n_envs):
    """int32 [n_envs]; the random pattern marks 30 % with non-zero values other than 1 among them (the header tests != 0)."""
    p = np.zeros(n_envs, dtype=np.int32)
    if pattern == 'all':
        p[:] = 1
    elif pattern == 'first':
        p[0] = 1
    elif pattern == 'last':
        p[-1] = 1
    elif pattern == 'alternating':
        p[1::2] = 1
    elif pattern == 'random':
        p[:] = np.where(rng.random(n_envs) < 0.3, rng.choice(np.array([1, 1, 2, -1, -2 ** 31], dtype=np.int64), n_envs), 0)
    else:
        assert pattern == 'none', pattern
    return p


def random_actions(rng, n_envs, n_cols):
    """Uniform over all of int32, negatives included: a row that is clamped or drawn again shows."""
    return rng.integers(-2 ** 31, 2 ** 31, (n_envs, n_cols), dtype=np.int64).astype(np.int32)


def random_highs(rng, n_cols):
    """[1, 5000), the middle column 1 (every draw 0) and the last 2^31 - 1; with one column the last rule holds."""
    high = rng.integers(1, 5000, n_cols).astype(np.int32)
    high[n_cols // 2] = 1
    high[-1] = INT32_MAX
    return high


def random_episodes(rng, n_envs):
    """Uniform over uint32 with 0xFFFFFFFF, 0 and 1 forced on the first envs (as many as there are)."""
    episode = rng.integers(0, 2 ** 32, n_envs, dtype=np.uint64).astype(np.uint32)
    for k, v in enumerate((0xFFFFFFFF, 0, 1)):
        if k < n_envs:
            episode[k] = v
    return episode


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def build_merge_case(n_envs, n_cols, pattern, first_env=None, seed=None):
    """The seeded inputs of one merge; first_env and seed cycle over FIRST_ENVS and SEEDS with the case unless given."""
    k = (n_envs * 31 + n_cols) * len(PENDING_PATTERNS) + PENDING_PATTERNS.index(pattern)
    rng = np.random.default_rng([n_envs, n_cols, PENDING_PATTERNS.index(pattern)])
    return _freeze(dict(n_envs=n_envs, n_cols=n_cols, pattern=pattern, actions_in=random_actions(rng, n_envs, n_cols),
                        pending=pending_pattern(pattern, rng, n_envs), episode=random_episodes(rng, n_envs),
                        high=random_highs(rng, n_cols), first_env=FIRST_ENVS[k % len(FIRST_ENVS)] if first_env is None else first_env,
                        seed=SEEDS[(k // len(FIRST_ENVS)) % len(SEEDS)] if seed is None else seed))


@lru_cache(maxsize=None)
def merged(n_envs, n_cols, pattern, first_env=None, seed=None):
    """merge_ref of build_merge_case's inputs: computed once, read-only."""
    c = build_merge_case(n_envs, n_cols, pattern, first_env, seed)
    out = merge_ref(c['actions_in'], c['pending'], c['episode'], c['high'], c['first_env'], c['seed'])
    out.setflags(write=False)
    return out


def random_reward(rng, n_envs, reward_cols):
    """float32 [n_envs, reward_cols] with NaN and -0.0 sprinkled in (a tenth each), or None."""
    if reward_cols is None:
        return None
    r = rng.standard_normal((n_envs, reward_cols)).astype(np.float32)
    u = rng.random((n_envs, reward_cols))
    r[u < 0.1] = np.nan
    r[u > 0.9] = -0.0
    return r


def random_advance_state(n_envs, reward_cols, salt=0):
    """pending at 30 %, elapsed in [0, 12] (at episode_length 10 some envs are at or past the length), episode uniform over uint32
    with 0xFFFFFFFF on the middle env, which is pending so that it wraps (with one env: on even salts only); done and reset_out
    start as bytes the launch has to overwrite."""
    rng = np.random.default_rng([n_envs, reward_cols or 0, salt])
    state = dict(pending=pending_pattern('random', rng, n_envs), episode=rng.integers(0, 2 ** 32, n_envs, dtype=np.uint64).astype(np.uint32),
                 elapsed=rng.integers(0, 13, n_envs).astype(np.int32), done=np.full(n_envs, 7, dtype=np.uint8),
                 reset_out=np.full(n_envs, 9, dtype=np.uint8), reward=random_reward(rng, n_envs, reward_cols))
    state['episode'][n_envs // 2] = 0xFFFFFFFF
    if n_envs > 1 or salt % 2 == 0:
        state['pending'][n_envs // 2] = 1
    return state


def staggered_advance_state(n_envs, reward_cols, rng):
    """elapsed = arange(B) % 10, nothing pending: what VecD2DEnv.reset(elapsed=...) leaves."""
    return dict(pending=np.zeros(n_envs, dtype=np.int32), episode=random_episodes(rng, n_envs),
                elapsed=(np.arange(n_envs) % 10).astype(np.int32), done=np.zeros(n_envs, dtype=np.uint8),
                reset_out=np.zeros(n_envs, dtype=np.uint8), reward=random_reward(rng, n_envs, reward_cols))

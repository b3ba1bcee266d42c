"""Direct launches of libd2d_episode.so (csrc/d2d_episode.hip: merge_kernel, advance_kernel) at the shapes VecD2DEnv(autoreset=True)
never gives them - a tail of 1 to 3 elements, fewer elements than one vector, vectors that span three or four envs, the scalar
route of pointers off 16-byte alignment, more vectors than the capped grid holds, more than one wave and workgroup, a partly
filled last wave, reward rows wider than a wave - against the NumPy restatement of include/d2d_episode.h (episode_util.merge_ref,
advance_ref).  The shape lists, each with the path it forces, are in episode_util.py; test_episode_cpu.py checks them and the
restatement on the CPU.  Every comparison is exact.

Every array a launch writes lies inside one arena of a sentinel byte with 64 guard words before and after it; after the launch every
byte outside the live ranges is still the sentinel, and what a merge only reads is bit for bit what it was.  done and reset_out
also stand at odd byte offsets.  actions_in and actions_out are distinct, as the header requires.

Not covered: the 64-bit index arithmetic of totals of 2^32 and more (narrow == 0), which needs planes of 16 GiB.

Measured on an MI355X (256 CUs): 112 tests, 127 merge launches (54 on the vector route, 72 on the scalar route, one of 65155 x 129:
2 101 248 vectors against a grid of 2 097 152, tail 3) and 117 advance launches (42 single, 3 x 25 consecutive), every one equal
to the restatement in every word and every guard byte intact.  The slowest test took 0.48 s (the first, which loads the library),
the one past the capped grid 0.27 s with its reference, every other under 0.03 s.  With the `p = pending[b]` refresh at the env
boundary taken out of merge_kernel (a scratch build), 23 vector-route cases, the capped-grid case and test_gpu_autoreset.py's
row-slice test fail; CHANGELOG.md has the list."""
import numpy as np
import pytest

import episode_util as eu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GUARD_WORDS = 64
SENTINEL = 0xA5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class Arena:
    """One device allocation of SENTINEL bytes holding the named arrays of `specs` ((name, NumPy array or (shape, dtype), byte
    offset past a 16-byte boundary)), each with GUARD_WORDS words of sentinel on either side."""

    def __init__(self, specs):
        self.live, cursor = {}, 0
        for name, what, offset in specs:
            shape, dtype = (what.shape, what.dtype) if isinstance(what, np.ndarray) else what
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            start = (cursor + 4 * GUARD_WORDS + 15) // 16 * 16 + offset
            self.live[name] = (start, nbytes, shape, np.dtype(dtype))
            cursor = start + nbytes + 4 * GUARD_WORDS
        self.buf = torch.full((cursor + 16,), SENTINEL, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 16 == 0
        for name, what, _ in specs:
            if isinstance(what, np.ndarray):
                self.upload(name, what)

    def _bytes(self, name):
        start, nbytes, _, _ = self.live[name]
        return self.buf[start:start + nbytes]

    def ptr(self, name):
        return self.buf.data_ptr() + self.live[name][0]

    def upload(self, name, array):
        _, nbytes, shape, dtype = self.live[name]
        assert array.shape == tuple(shape) and array.dtype == dtype
        self._bytes(name).copy_(torch.as_tensor(_bits(array).reshape(-1).copy()))

    def download(self, name):
        _, _, shape, dtype = self.live[name]
        return self._bytes(name).cpu().numpy().view(dtype).reshape(shape)

    def assert_guards(self, what):
        """Byte by byte: everything outside the live ranges is the sentinel."""
        outside = torch.ones(self.buf.numel(), dtype=torch.bool, device='cuda')
        for name, (start, nbytes, _, _) in self.live.items():
            assert bool(outside[start - 4 * GUARD_WORDS:start + nbytes + 4 * GUARD_WORDS].all()), f'{name}: guards overlap'
            outside[start:start + nbytes] = False
        bad = torch.nonzero(outside & (self.buf != SENTINEL)).view(-1)
        assert bad.numel() == 0, f'{what}: {bad.numel()} bytes outside the outputs were written, the first at arena offset ' \
                                 f'{int(bad[0])} (live ranges {[(n, v[0], v[0] + v[1]) for n, v in self.live.items()]})'


def _merge(c, want, in_words=0, out_words=0):
    """One d2d_episode_merge_actions of a case with actions_in / actions_out moved in_words / out_words int32 words past a 16-byte
    boundary; the guard and input checks every launch gets; asserts out == want."""
    from gym_d2d_amd import _native
    n_envs, n_cols = c['n_envs'], c['n_cols']
    arena = Arena([('out', ((n_envs, n_cols), np.int32), 4 * out_words)])
    room = torch.zeros(n_envs * n_cols + 4, dtype=torch.int32, device='cuda')
    assert room.data_ptr() % 16 == 0
    src = room[in_words:in_words + n_envs * n_cols]
    src.copy_(torch.as_tensor(np.array(c['actions_in']).reshape(-1)))
    dev = {k: torch.as_tensor(np.array(c[k]).view(np.int32), device='cuda') for k in ('pending', 'episode', 'high')}
    assert (src.data_ptr() % 16 != 0) == (in_words % 4 != 0) and (arena.ptr('out') % 16 != 0) == (out_words % 4 != 0)
    torch.cuda.synchronize()
    _native.episode_merge_actions(src.data_ptr(), arena.ptr('out'), dev['pending'].data_ptr(), dev['episode'].data_ptr(),
                                  dev['high'].data_ptr(), n_envs, n_cols, c['first_env'], c['seed'], _stream())
    torch.cuda.synchronize()
    what = f"merge {n_envs} x {n_cols} {c['pattern']} in+{in_words} out+{out_words} first_env {c['first_env']} seed {c['seed']}"
    arena.assert_guards(what)
    for k in dev:
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(c[k])), f'{what}: {k} was written'
    assert np.array_equal(src.cpu().numpy(), c['actions_in'].reshape(-1)), f'{what}: actions_in was written'
    assert int(room[:in_words].abs().sum()) == 0 and int(room[in_words + n_envs * n_cols:].abs().sum()) == 0, what
    got = arena.download('out')
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, f'{what}: {len(wrong)} of {got.size} entries differ, the first at (env, column) {wrong[0].tolist()}: ' \
                            f'{got[tuple(wrong[0])]} for {want[tuple(wrong[0])]}'
    return what


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize('pattern', eu.PENDING_PATTERNS)
@pytest.mark.parametrize('n_envs,n_cols', eu.MERGE_SHAPES)
def test_merge_vector_route_equals_the_restatement(n_envs, n_cols, pattern):
    c = eu.build_merge_case(n_envs, n_cols, pattern)
    what = _merge(c, eu.merged(n_envs, n_cols, pattern))
    print(f"{what}: {n_envs * n_cols // 4} vectors, tail {n_envs * n_cols % 4}, {int((c['pending'] != 0).sum())} pending, exact")


@pytest.mark.parametrize('in_words,out_words', [(1, 0), (0, 1), (1, 1), (3, 3)])
@pytest.mark.parametrize('n_envs,n_cols', eu.SCALAR_SHAPES)
def test_merge_scalar_route_equals_the_restatement(n_envs, n_cols, in_words, out_words):
    """A pointer one or three words off 16-byte alignment, either one alone or both: merge_kernel<1>, the route a row slice of
    a user's action tensor takes."""
    for pattern in eu.PENDING_PATTERNS:
        what = _merge(eu.build_merge_case(n_envs, n_cols, pattern), eu.merged(n_envs, n_cols, pattern), in_words, out_words)
        print(f'{what}: exact')


def test_merge_past_the_capped_grid_equals_the_restatement():
    """More vectors than 32 workgroups per CU of 256 lanes hold: every lane of the grid takes a second trip of its loop, some a
    third; a tail too."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_envs, n_cols = eu.grid_stride_shape(cus)
    nvec, cap = n_envs * n_cols // 4, 32 * cus * 256
    print(f'{cus} CUs: {n_envs} x {n_cols}, nvec {nvec}, cap {cap} vectors, tail {n_envs * n_cols % 4}')
    assert nvec > cap and n_envs * n_cols % 4 != 0
    _merge(eu.build_merge_case(n_envs, n_cols, 'random'), eu.merged(n_envs, n_cols, 'random'))


# ------------------------------------------------------------------------------------------ advance
NAMES = ('pending', 'episode', 'elapsed', 'done', 'reset_out')


def _advance_arena(state, byte_offset):
    """pending, episode, elapsed, then done and reset_out `byte_offset` and `byte_offset + 2` bytes past a 16-byte boundary, then
    the reward plane."""
    specs = [(k, state[k], 0) for k in NAMES[:3]] + [('done', state['done'], byte_offset)]
    specs.append(('reset_out', state['reset_out'], byte_offset + 2 if byte_offset else 0))
    if state['reward'] is not None:
        specs.append(('reward', state['reward'], 0))
    return Arena(specs)


def _advance(arena, state, length, what):
    """One d2d_episode_advance on the arena's arrays; asserts them equal to advance_ref(state) bit for bit; returns that state."""
    from gym_d2d_amd import _native
    n_envs = len(state['pending'])
    reward = state['reward']
    torch.cuda.synchronize()
    _native.episode_advance(*(arena.ptr(k) for k in NAMES), 0 if reward is None else arena.ptr('reward'),
                            1 if reward is None else reward.shape[1], n_envs, length, _stream())
    torch.cuda.synchronize()
    arena.assert_guards(what)
    want = eu.advance_ref(state, length)
    for k in NAMES:
        got = arena.download(k)
        wrong = np.argwhere(got != want[k]).reshape(-1)
        assert len(wrong) == 0, f'{what}: {k} differs at {len(wrong)} envs, the first {wrong[0]}: {got[wrong[0]]} for {want[k][wrong[0]]}'
    if reward is not None:
        got, ref = arena.download('reward').view(np.uint32), want['reward'].view(np.uint32)
        wrong = np.argwhere(got != ref)
        assert len(wrong) == 0, f'{what}: reward differs at {len(wrong)} words, the first at (env, column) {wrong[0].tolist()}: ' \
                                f'{got[tuple(wrong[0])]:#x} for {ref[tuple(wrong[0])]:#x}'
        assert not ref[want['reset_out'] != 0].any()
    return want


@pytest.mark.parametrize('reward_cols', eu.REWARD_COLS)
@pytest.mark.parametrize('n_envs', eu.ADVANCE_ENVS)
def test_advance_one_launch_equals_the_restatement(n_envs, reward_cols):
    state = eu.random_advance_state(n_envs, reward_cols, salt=eu.REWARD_COLS.index(reward_cols))
    odd = 1 if n_envs in (65, 1000) else 0
    arena = _advance_arena(state, odd)
    assert arena.ptr('done') % 2 == odd and arena.ptr('reset_out') % 2 == odd
    want = _advance(arena, state, 10, f'advance {n_envs} envs, reward_cols {reward_cols}')
    print(f"advance {n_envs} envs, reward_cols {reward_cols}: {int(want['reset_out'].sum())} reset, {int(want['done'].sum())} done, "
          f"done / reset_out {'odd' if odd else 'even'} addresses, exact")
    if n_envs > 1:
        assert want['reset_out'].any() and want['done'].any() and not want['done'].all()


@pytest.mark.parametrize('n_envs,reward_cols,length', [(257, 65, 10), (65, None, 10), (257, 65, 1)])
def test_advance_25_consecutive_launches_equal_the_restatement(n_envs, reward_cols, length):
    """From elapsed = arange(B) % 10 with nothing pending; the reward plane is new before every launch; compared after every one.
    With episode_length 1 every env alternates between done and reset."""
    rng = np.random.default_rng(3)
    state = eu.staggered_advance_state(n_envs, reward_cols, rng)
    arena = _advance_arena(state, 1)
    assert arena.ptr('done') % 16 == 1 and arena.ptr('reset_out') % 16 == 3
    resets = dones = 0
    for t in range(25):
        if reward_cols is not None:
            state['reward'] = eu.random_reward(rng, n_envs, reward_cols)
            arena.upload('reward', state['reward'])
        state = _advance(arena, state, length, f'advance {n_envs} envs, reward_cols {reward_cols}, length {length}, launch {t + 1}')
        if length == 1:
            assert state['done'].all() if t % 2 == 0 else state['reset_out'].all()
        resets, dones = resets + int(state['reset_out'].sum()), dones + int(state['done'].sum())
    print(f'advance {n_envs} envs, reward_cols {reward_cols}, length {length}: 25 launches, {dones} dones, {resets} resets, exact')
    assert resets >= 2 * n_envs

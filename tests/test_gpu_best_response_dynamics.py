"""Sequential best-response RB dynamics on the GPU (VecD2DEnv.best_response_dynamics, best_response_dynamics_actions,
csrc/d2d_brdyn.hip).

Two yardsticks.  Exact, no tolerance: the existing kernels - a torch loop does the same thing link by link through the public API
(best_rb(), move link i if its gain is large enough, step(), next link) and every output must be equal, sinr_db bit for bit with
the last step's plane.  Within the project's bar: the float64 restatement on the oracle's path loss
(best_response_dynamics_util.dynamics), compared on the envs it does not call ambiguous (test_best_response_dynamics_cpu.py holds
their share under 25 % on the oracle alone)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import best_response_dynamics_util as bu
import power_control_util as pcu
from golden_util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

B, BAR = bu.B, bu.BAR
NAMES = ('rb', 'sinr_db', 'rounds', 'moves', 'converged')

# the exact cases - name: (cues, due pairs, R, law, cell radius m, links put on no RB, max_rounds), then optionally a dict: b (envs;
# large shapes take 4 to 8, not 64), movable (the links that take turns; None: all), rb_below (the seeded RBs folded into [0, rb_below))
EXACT = {
    'n37_r5': (12, 25, 5, 'ld2', 40.0, 1, 6),                           # not a multiple of the wave, fewer RBs than lanes
    'n20_r64': (6, 14, 64, 'ld2', 40.0, 1, 6),                          # more RBs than links: empty RBs, exact ties to the lowest r
    'n50_r6_ld2': (20, 30, 6, 'ld2', 40.0, 1, 6),
    'n50_r6_ld35': (20, 30, 6, 'ld35', 40.0, 1, 6),
    'n50_r6_hata': (20, 30, 6, 'urban', 40.0, 1, 6),
    'n50_r6_mixed': (20, 30, 6, 'mixed', 40.0, 1, 6),
    'n300_r7': (100, 200, 7, 'ld2', 40.0, 1, 2),                        # more links than threads, ten words per RB
    'n1_r3': (1, 0, 3, 'ld2', 40.0, 0, 6),
    'n96_r1': (32, 64, 1, 'ld2', 40.0, 1, 6),                           # nothing can move
    # ---- the paths of brdyn_kernel that need more than 64 RBs or more than 64 KiB (threads = min(256, R rounded up to 64))
    # TWO WAVES (128 threads): the cross-wave half of the argmax, s.key[parity * 4 + wave] and the parity double buffer.  With
    # with_allowed=True also the MULTI-WORD allowed mask: three words per link, a ragged tail of ONE valid bit in the last word
    'n150_r65': (50, 100, 65, 'ld2', 40.0, 1, 3, dict(b=8)),
    'n300_r160_ld35': (100, 200, 160, 'ld35', 40.0, 1, 3, dict(b=8)),   # THREE WAVES: the 192-thread launch; pow-k law
    'n300_r200': (100, 200, 200, 'ld2', 40.0, 1, 3, dict(b=8)),         # FOUR WAVES, the last one partly filled (lanes 200..255 idle)
    'n400_r256_mixed': (100, 300, 256, 'mixed', 40.0, 1, 3, dict(b=8)),  # R = 256 exactly: every lane owns one RB; general power law
    'n400_r300': (100, 300, 300, 'ld2', 40.0, 1, 3, dict(b=8)),         # R > 256: lanes 0..43 own TWO RBs (r and r + 256); ten mask words
    # LARGE LDS through the links: 152 KiB, the MaxDynamicSharedMemorySize branch; j up to 2047, 64 bitset words per RB
    'n2048_r256': (512, 1536, 256, 'ld2', 40.0, 1, 3, dict(b=4, movable=bu.BIG_MOVABLE)),
    # LARGE LDS through the bitset: 10 x 2500 words are 98 KiB of 112 KiB; the movers run out of empty RBs below 256 (see bu.CASES)
    'n320_r2500': (100, 220, 2500, 'ld2', 40.0, 1, 2, dict(b=4, rb_below=280)),
}
MULTI_ROUND = ('n37_r5', 'n20_r64', 'n50_r6_ld2', 'n50_r6_ld35', 'n50_r6_hata', 'n50_r6_mixed', 'n300_r7')
# the shapes above 64 RBs or 64 KiB: (name, the hystereses the public-API loop is run at)
WIDE = [('n150_r65', (0.0, 3.0)), ('n300_r160_ld35', (0.0, 3.0)), ('n300_r200', (0.0, 3.0)), ('n400_r256_mixed', (0.0, 3.0)),
        ('n400_r300', (0.0, 3.0)), ('n2048_r256', (0.0, 3.0)), ('n320_r2500', (3.0,))]
_cache = {}


def _case(name):
    if name.startswith('oracle/'):
        return bu.make_case(name[len('oracle/'):])
    cues, dues, r, law, cell, no_rb, max_rounds = EXACT[name][:7]
    o = dict(dict(b=B, movable=None, rb_below=None), **(EXACT[name][7] if len(EXACT[name]) > 7 else {}))
    pos, raw, rb, pwr = pcu.state(cues, dues, r, 100 + sum(map(ord, name)), cell, no_rb, o['b'])
    levels = pcu.bounds(cues, dues)[2]
    if o['rb_below']:
        rb = np.where(rb < r, rb % o['rb_below'], rb).astype(np.int32)  # the links on no RB stay there
        raw = (rb * levels[None, :] + pwr).astype(np.int32)
    movable = None
    if o['movable'] is not None:
        movable = np.zeros(cues + dues, dtype=bool)
        movable[list(o['movable'])] = True
    return SimpleNamespace(name=name, cues=cues, dues=dues, n=cues + dues, r=r, law=law, pos=pos, raw=raw, rb=rb, pwr=pwr,
                           levels=levels, max_rounds=max_rounds, b=o['b'], movable=movable)


def _build(name, cue_actions='agent'):
    """The env of a case, stepped once on the case's layout with the case's actions; built once."""
    key = (name, cue_actions)
    if key not in _cache:
        from gym_d2d_amd.envs import VecD2DEnv
        c = _case(name)
        cfg = {'num_rbs': c.r, 'num_cues': c.cues, 'num_due_pairs': c.dues, 'path_loss_model': pcu.models()[c.law][0]}
        if c.n > 300:                                                   # no [B, N, 6 N] observation block at these sizes
            from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
            cfg['obs_fn'] = SignalPlanesObsFunction
        env = VecD2DEnv(cfg, num_envs=c.b, cue_actions=cue_actions)
        env.reset(seed=3)
        env.simulator.set_positions(c.pos)
        first = c.n - env.num_agents
        raw = torch.as_tensor(np.ascontiguousarray(c.raw[:, first:]), device=env.device)
        env.step(raw)
        _cache[key] = (env, c, raw)
    return _cache[key]


@pytest.fixture(scope='module', autouse=True)
def _close_envs():
    yield
    for env, _, _ in _cache.values():
        env.close()
    _cache.clear()


def _host(res):
    torch.cuda.synchronize()                                            # raises if the device faulted
    return tuple(t.cpu().numpy().copy() for t in res)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, what=''):
    for x, y, name in zip(a, b, NAMES):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f'{what}: {name}'


def _api_loop(env, c, allowed, movable, min_gain_db, max_rounds):
    """The dynamics through the public API, one link at a time: best_rb(), move link i, step().  Returns (rb, sinr_db, rounds, moves,
    converged) on the host, sinr_db being the last step's plane, and (dest int [R], the moves that ended on each RB; moved int [N],
    the moves each link made)."""
    first = c.n - env.num_agents
    levels = torch.as_tensor(np.asarray(c.levels), device=env.device)
    rounds = torch.zeros(c.b, dtype=torch.int32, device=env.device)
    moves = torch.zeros(c.b, dtype=torch.int32, device=env.device)
    dest = torch.zeros(c.r, dtype=torch.int64, device=env.device)
    by_link = torch.zeros(c.n, dtype=torch.int64, device=env.device)
    turns = [i for i in range(first, c.n) if movable is None or movable[i]]
    for _ in range(max_rounds):
        moved = torch.zeros(c.b, dtype=torch.bool, device=env.device)
        for i in turns:
            best, _, gain = env.best_rb(allowed)
            move = gain[:, i] > min_gain_db                              # NaN: stays
            rb = env._t['rb'].clone()
            rb[:, i] = torch.where(move, best[:, i], rb[:, i])
            dest += torch.bincount(best[:, i][move].to(torch.int64), minlength=c.r)
            by_link[i] += move.sum()
            env.step((rb * levels + env._t['pwr'])[:, first:].to(torch.int32).contiguous())
            moved |= move
            moves += move.to(torch.int32)
        rounds += moved.to(torch.int32)
        if not bool(moved.any()):
            break
    conv = (rounds < max_rounds).to(torch.uint8)                         # a round moved nobody, and then no later one does
    return _host((env._t['rb'], env._t['sinr_db'], rounds, moves, conv)), dest.cpu().numpy(), by_link.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1: the whole trajectory, exactly
def _trajectory(name, min_gain_db, with_allowed=False, coverage=None):
    """One launch against the public-API loop.  The mask of with_allowed is built for any R: a link with no allowed RB and, past
    one word, a link whose only allowed RB is the last one (it lies in the last word, next to the ragged tail).  coverage: a dict
    that receives the reference loop's dest and moved (see _api_loop)."""
    from gym_d2d_amd import _native
    env, c, raw = _build(name)
    allowed = None
    if with_allowed:
        rng = np.random.default_rng(31)
        allowed = rng.random((c.n, c.r)) < 0.7
        allowed[5] = False                                               # a link with no allowed RB never moves
        allowed[np.arange(c.n), rng.integers(0, c.r, c.n)] |= np.arange(c.n) != 5
        if c.r > 32:
            allowed[7] = False
            allowed[7, c.r - 1] = True                                   # its only allowed RB lies in the last word
        allowed = torch.as_tensor(allowed, device=env.device)
    before = _native.brdyn_launches
    got = _host(env.best_response_dynamics(allowed, c.movable, min_gain_db=min_gain_db, max_rounds=c.max_rounds))
    assert _native.brdyn_launches == before + 1
    rb, sinr, rounds, moves, conv = got
    assert rb.dtype == np.int32 and sinr.dtype == np.float32 and rounds.dtype == moves.dtype == np.int32 and conv.dtype == np.uint8
    assert rb.shape == sinr.shape == (c.b, c.n) and rounds.shape == moves.shape == conv.shape == (c.b,)
    if with_allowed and c.r & 31:
        # garbage in every bit at and above R of the last word (the public packing leaves them 0) must change nothing
        k = env._best_response_dynamics_kernel()
        pack = k.words

        def dirty(mask):
            words = pack(mask)
            words[:, -1] |= -(1 << (c.r & 31))
            return words
        k.words = dirty
        try:
            again = _host(env.best_response_dynamics(allowed, c.movable, min_gain_db=min_gain_db, max_rounds=c.max_rounds))
        finally:
            del k.words
        _same(again, got, 'bits at and above R in the last allowed word')
    want, dest, by_link = _api_loop(env, c, allowed, c.movable, min_gain_db, c.max_rounds)
    if coverage is not None:
        coverage.update(dest=dest, moved=by_link)
    env.step(raw)                                                       # the case's own state back
    print(f'{name} at {min_gain_db:g} dB: rounds {rounds.min()}..{rounds.max()}, moves {moves.min()}..{moves.max()}, converged '
          f'{conv.mean():.0%}')
    on = (c.rb >= 0) & (c.rb < c.r)
    assert np.array_equal(rb, want[0]) and np.array_equal(rounds, want[2]) and np.array_equal(moves, want[3])
    assert np.array_equal(conv, want[4])
    assert np.array_equal(_bits(sinr[on]), _bits(want[1][on])) and np.isnan(sinr[~on]).all()
    assert np.array_equal(rb[~on], c.rb[~on])                           # on no RB: kept
    if with_allowed:
        assert np.array_equal(rb[:, 5], c.rb[:, 5])
        if c.r > 32:
            assert ((rb[:, 7] == c.rb[:, 7]) | (rb[:, 7] == c.r - 1)).all() and (want[0][:, 7] == c.r - 1).any()
    return got


@pytest.mark.parametrize('min_gain_db', [0.0, 3.0])
@pytest.mark.parametrize('name', MULTI_ROUND)
def test_whole_trajectory_equals_the_public_api_loop(name, min_gain_db):
    rb, sinr, rounds, moves, conv = _trajectory(name, min_gain_db)
    c = _case(name)
    assert (moves > 0).any() and rounds.max() >= 1
    if min_gain_db == 0.0 and name not in ('n20_r64',):
        assert (conv == 0).any() and (rounds[conv == 0] == c.max_rounds).all()      # cycling exercises the cap


def test_whole_trajectory_with_an_allowed_mask():
    _trajectory('n37_r5', 3.0, with_allowed=True)


@pytest.mark.parametrize('name,min_gain_db', [(name, g) for name, gains in WIDE for g in gains])
def test_whole_trajectory_at_multi_wave_and_large_lds_shapes(name, min_gain_db):
    """The shapes of WIDE against the public-API loop, with what each is there for asserted on that loop's own moves: they end in
    every block of RBs (bu.rb_blocks: every wave of the launch holds a winner at some turn), past 256 RBs on both sides of 256
    (both RBs of a lane), and at 2048 links a link j >= 1024 moves."""
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response_dynamics import lds_bytes
    seen = {}
    rb, sinr, rounds, moves, conv = _trajectory(name, min_gain_db, coverage=seen)
    c = _case(name)
    lds = lds_bytes(c.n, c.r, c.law != 'ld2', False)
    print(f'{name}: {lds} bytes of LDS; moves into each RB block {np.bincount(bu.rb_blocks(c.r), weights=seen["dest"]).astype(int).tolist()}, '
          f'{int(seen["dest"][256:].sum())} at r >= 256, {int(seen["moved"][1024:].sum())} by links j >= 1024')
    assert (moves > 0).any() and rounds.max() >= 1 and seen['dest'].sum() == moves.sum()
    assert c.r > 64 and bu.covers(seen['dest'], c.r)
    assert lds <= _native.BRDYN_MAX_LDS_BYTES and (lds > 64 * 1024) == (name in ('n2048_r256', 'n320_r2500'))
    if c.n > 1024:
        assert seen['moved'][1024:].sum() > 0 and not seen['moved'][~c.movable].any()
        assert (rb[:, ~c.movable] == c.rb[:, ~c.movable]).all()


@pytest.mark.parametrize('name', ['n150_r65', 'n400_r300'])
def test_whole_trajectory_with_a_multi_word_allowed_mask(name):
    """Three words with one valid bit in the last (R = 65), ten words with a tail of 12 (R = 300): s.al[i * words + (r >> 5)] past
    word 0, the tail mask on a last word that is not the first, garbage above R, a link allowed on the last RB only."""
    seen = {}
    rb, sinr, rounds, moves, conv = _trajectory(name, 3.0, with_allowed=True, coverage=seen)
    c = _case(name)
    assert (moves > 0).any() and bu.covers(seen['dest'], c.r)           # the allowed winners come from every word's RBs


def test_one_link_has_nobody_to_avoid():
    rb, sinr, rounds, moves, conv = _trajectory('n1_r3', 0.0)
    assert (rounds == 0).all() and (moves == 0).all() and (conv == 1).all()


def test_one_rb_nothing_can_move():
    rb, sinr, rounds, moves, conv = _trajectory('n96_r1', 0.0)
    assert (rounds == 0).all() and (moves == 0).all() and (conv == 1).all()


# ------------------------------------------------------------------------------------------ 2: through step()
@pytest.mark.parametrize('name,with_allowed', [('n37_r5', False), ('n37_r5', True), ('n50_r6_mixed', False), ('n20_r64', False),
                                               ('n300_r200', False), ('n400_r300', True)])
def test_step_of_the_actions_lands_on_the_solved_rbs_and_converged_envs_are_quiet(name, with_allowed):
    env, c, raw = _build(name)
    allowed = None
    if with_allowed:
        allowed = torch.as_tensor(np.random.default_rng(8).random((c.n, c.r)) < 0.6, device=env.device)
    min_gain_db = 3.0
    res = _host(env.best_response_dynamics(allowed, min_gain_db=min_gain_db))
    rb, sinr, rounds, moves, conv = res
    actions = env.best_response_dynamics_actions(allowed, min_gain_db=min_gain_db)
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (c.b, env.num_agents)
    _, _, _, info = env.step(actions)
    on = (c.rb >= 0) & (c.rb < c.r)
    assert np.array_equal(info['rb'].cpu().numpy(), rb) and np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), c.pwr)
    s = info['sinr_db'].cpu().numpy()
    assert np.array_equal(_bits(s[on]), _bits(sinr[on])) and np.isnan(sinr[~on]).all()
    gain = env.best_rb(allowed)[2].cpu().numpy()
    done = conv == 1
    assert done.any()
    with np.errstate(invalid='ignore'):
        assert (np.isnan(gain[done]) | (gain[done] <= min_gain_db)).all()          # nobody wants to move any more
    env.step(raw)


# ------------------------------------------------------------------------------------------ 3: one movable link, one round
def test_a_single_movable_link_equals_best_response_actions_for_that_link():
    env, c, raw = _build('n37_r5')
    for k in (0, 17, c.n - 2):
        only = np.arange(c.n) == k
        allowed = torch.as_tensor(np.broadcast_to(only[:, None], (c.n, c.r)).copy(), device=env.device)
        for min_gain_db in (0.0, 3.0):
            want = env.best_response_actions(allowed=allowed, min_gain_db=min_gain_db).clone()
            got = env.best_response_dynamics_actions(movable=only, min_gain_db=min_gain_db, max_rounds=1)
            assert torch.equal(got, want), (k, min_gain_db)
            res = _host(env.best_response_dynamics(movable=only, min_gain_db=min_gain_db, max_rounds=1))
            assert np.array_equal(res[3], (res[0][:, k] != c.rb[:, k]).astype(np.int32))
            assert np.array_equal(res[2], res[3]) and np.array_equal(res[4], 1 - res[3])
        assert (res[0][:, ~only] == c.rb[:, ~only]).all()


# ------------------------------------------------------------------------------------------ 4: the remaining properties
def test_env_mask_out_planes_determinism_and_zero_rounds():
    from gym_d2d_amd import _native
    env, c, _ = _build('n37_r5')
    want = _host(env.best_response_dynamics())
    own = env.best_response_dynamics()
    assert all(a is b for a, b in zip(own, env.best_response_dynamics()))           # the env's one quintuple, reused
    assert own.rb is own[0] and own.sinr_db is own[1] and own.rounds is own[2] and own.moves is own[3] and own.converged is own[4]
    _same(_host(own), want, 'two calls')

    def fresh():
        return (torch.full((B, c.n), -77, dtype=torch.int32, device=env.device), torch.full((B, c.n), 123.25, device=env.device),
                torch.full((B,), -5, dtype=torch.int32, device=env.device), torch.full((B,), -6, dtype=torch.int32, device=env.device),
                torch.full((B,), 9, dtype=torch.uint8, device=env.device))
    out = fresh()
    got = env.best_response_dynamics(out=out)
    assert all(a is b for a, b in zip(got, out))
    _same(_host(got), want, 'out=')
    mask = np.arange(B) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        got = _host(env.best_response_dynamics(out=fresh(), env_mask=m))
        _same([a[mask] for a in got], [a[mask] for a in want], 'env_mask')
        assert (got[0][~mask] == -77).all() and (got[1][~mask] == 123.25).all() and (got[2][~mask] == -5).all()
        assert (got[3][~mask] == -6).all() and (got[4][~mask] == 9).all()
    zero = _host(env.best_response_dynamics(max_rounds=0))
    on = (c.rb >= 0) & (c.rb < c.r)
    assert np.array_equal(zero[0], c.rb) and (zero[2] == 0).all() and (zero[3] == 0).all() and (zero[4] == 0).all()
    assert np.array_equal(_bits(zero[1][on]), _bits(env._t['sinr_db'].cpu().numpy()[on])) and np.isnan(zero[1][~on]).all()
    none = _host(env.best_response_dynamics(movable=np.zeros(c.n, bool)))
    assert np.array_equal(none[0], c.rb) and (none[2] == 0).all() and (none[4] == 1).all()
    before = _native.brdyn_launches
    o = fresh()
    for bad in (o[:4], (o[0], o[1], o[2], o[2], o[4]), (o[0], o[0].view(torch.float32), o[2], o[3], o[4]), o[0],
                (o[0], o[1], o[2], o[3], torch.empty(B, dtype=torch.int32, device=env.device)),
                (o[0], torch.empty((B, c.n + 1), device=env.device), o[2], o[3], o[4]), (o[0].cpu(), o[1], o[2], o[3], o[4])):
        with pytest.raises(ValueError, match='out must be'):
            env.best_response_dynamics(out=bad)
    with pytest.raises(ValueError, match='env_mask must be'):
        env.best_response_dynamics(env_mask=np.ones(B + 1, bool))
    for bad in (np.ones(c.n + 1, bool), np.ones(c.n, np.int32)):
        with pytest.raises(ValueError, match='movable must be'):
            env.best_response_dynamics(movable=bad)
    with pytest.raises(ValueError, match='allowed must be'):
        env.best_response_dynamics(allowed=np.ones((c.n, c.r + 1), bool))
    for bad in (-1, 2.5, True, _native.BRDYN_MAX_ROUNDS + 1):
        with pytest.raises(ValueError, match='max_rounds'):
            env.best_response_dynamics(max_rounds=bad)
    for bad in (-0.5, float('nan'), 'x'):
        with pytest.raises(ValueError, match='min_gain_db'):
            env.best_response_dynamics(min_gain_db=bad)
    assert _native.brdyn_launches == before                             # refused before any launch


def test_cue_links_on_traffic_actions_never_move():
    env, c, raw = _build('n37_r5', cue_actions='traffic')
    rb0 = env._t['rb'].cpu().numpy().copy()
    for movable in (None, np.ones(c.n, bool)):
        res = _host(env.best_response_dynamics(movable=movable, min_gain_db=0.0))
        assert np.array_equal(res[0][:, :c.cues], rb0[:, :c.cues]) and (res[0][:, c.cues:] != rb0[:, c.cues:]).any()
    a = env.best_response_dynamics_actions(min_gain_db=0.0)
    assert a.dtype == torch.int32 and tuple(a.shape) == (B, c.dues) == (B, env.num_agents)
    _, _, _, info = env.step(a)
    on = (rb0 >= 0) & (rb0 < c.r)
    assert np.array_equal(info['rb'].cpu().numpy(), res[0])
    assert np.array_equal(_bits(info['sinr_db'].cpu().numpy()[on]), _bits(res[1][on]))
    env.step(raw)


SMALL = {'num_rbs': 5, 'num_cues': 6, 'num_due_pairs': 20}


def _small_env(b=8, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    return VecD2DEnv(dict(SMALL), num_envs=b, **kw)


def _small_actions(env, rng):
    highs = env._initial_action_highs()
    return torch.as_tensor(np.stack([rng.integers(0, h, env.num_envs) for h in highs], axis=1).astype(np.int32), device=env.device)


def test_two_shards_equal_the_whole_batch():
    rng = np.random.default_rng(4)
    whole = _small_env()
    acts = [_small_actions(whole, rng) for _ in range(2)]

    def run(env, rows):
        out = []
        env.reset(seed=11)
        out.append(_host(env.best_response_dynamics()))
        for a in acts:
            env.step(a[rows].contiguous())
            out.append(_host(env.best_response_dynamics()))
        env.close()
        return out
    ref = run(whole, slice(0, 8))
    for k in range(2):
        rows = slice(k * 4, (k + 1) * 4)
        got = run(_small_env(b=4, first_env=k * 4), rows)
        for t, (a, b) in enumerate(zip(ref, got)):
            _same([x[rows] for x in a], b, f'shard {k}, step {t}')


@pytest.mark.parametrize('moving', [False, True])
def test_staggered_autoreset_equals_one_lockstep_env_each(moving):
    from gym_d2d_amd.mobility import GaussMarkovMobility
    mob = (lambda: {'mobility': GaussMarkovMobility(speed_std_mps=8.0, memory=0.7)}) if moving else (lambda: {})
    steps, first, b = 12, 40, 8
    env = _small_env(b=b, autoreset=True, first_env=first, **mob())
    env.reset(seed=21, elapsed=np.arange(b) % 10)
    rng = np.random.default_rng(4)
    acts, outs, resets = [], [_host(env.best_response_dynamics())], []
    for t in range(steps):
        a = _small_actions(env, rng)
        _, _, _, info = env.step(a)
        outs.append(_host(env.best_response_dynamics())); resets.append(info['reset'].cpu().numpy().copy()); acts.append(a)
    env.close()
    assert np.array(resets).sum() >= b
    for e in range(b):
        one = _small_env(b=1, first_env=first + e, **mob())
        one.reset(seed=21)
        _same([x[e:e + 1] for x in outs[0]], _host(one.best_response_dynamics()), f'env {e} reset')
        for t in range(steps):
            if resets[t][e]:
                one.reset()
            else:
                one.step(acts[t][e:e + 1].contiguous())
            _same([x[e:e + 1] for x in outs[t + 1]], _host(one.best_response_dynamics()), f'env {e} step {t + 1}')
        one.close()


def test_composes_with_power_control_actions():
    env = _small_env()
    try:
        env.reset(seed=2)
        target = {'cue': -4.0, 'due': 9.0}
        for _ in range(2):
            res = tuple(t.clone() for t in env.best_response_dynamics())
            _, _, _, info = env.step(env.best_response_dynamics_actions())
            assert torch.equal(info['rb'], res[0]) and torch.equal(info['sinr_db'].view(torch.int32), res[1].view(torch.int32))
            power = env.power_control(target)[0].clone()
            _, _, _, info = env.step(env.power_control_actions(target))
            assert torch.equal(info['rb'], res[0]) and torch.equal(info['tx_pwr_dbm'], power)      # RBs stay, powers are the solve's
        assert env.status_flags() == 0
    finally:
        env.close()


def test_envs_that_do_not_ask_launch_nothing():
    from gym_d2d_amd import _native
    before = _native.brdyn_launches
    env = _small_env()
    try:
        env.reset(seed=1)
        for _ in range(3):
            env.step(env.action_buffer().clone())
        assert env._brdyn is None and _native.brdyn_launches == before
        env.best_response_dynamics()
        assert env._brdyn is not None and _native.brdyn_launches == before + 1
    finally:
        env.close()


def test_unsupported_envs_are_refused_by_name(tmp_path):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.path_loss import ArrayPathLoss, PathLoss, ShadowingPathLoss, SpatialChannelPathLoss
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Foo(PathLoss):
        def __call__(self, tx, rx):
            return 20 * np.log10(tx.position.distance(rx.position)) + 40.0

    class Arr(ArrayPathLoss):
        def compute(self, view):
            return 20 * view.xp.log10(view.distance()) + 40.0

    class PerStep(Arr):
        per_step = True
    before = _native.brdyn_launches

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            with pytest.raises(ValueError, match=text):
                env.best_response_dynamics()
            with pytest.raises(ValueError, match=text):
                env.best_response_dynamics_actions()
            assert env._brdyn is None
        finally:
            env.close()
    refused(r'best_response_dynamics\(\).*export_actions', export_actions=False)
    refused(r'best_response_dynamics\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"best_response_dynamics\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"best_response_dynamics\(\).*'array'", {'path_loss_model': Arr})
    refused(r"best_response_dynamics\(\).*'per_step'", {'path_loss_model': PerStep})
    refused(r"best_response_dynamics\(\).*'channel'", {'path_loss_model': SpatialChannelPathLoss})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'best_response_dynamics\(\).*float32 cannot hold', {'device_config_file': pinned})
    env = VecD2DEnv(dict(small), num_envs=2, use_torch=False)
    try:
        with pytest.raises(ValueError, match=r'best_response_dynamics\(\) needs the torch path'):
            env.best_response_dynamics()
    finally:
        env.close()
    assert _native.brdyn_launches == before                             # at the call, not inside a launch


# ------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize('name', list(bu.CASES))
def test_against_the_oracle_restatement(name):
    env, c, _ = _build('oracle/' + name)
    o = bu.oracle_side(name)
    rb, sinr, rounds, moves, conv = _host(env.best_response_dynamics(movable=c.movable, min_gain_db=bu.MIN_GAIN_DB, max_rounds=c.max_rounds))
    ok = ~o.ambiguous
    share = float(o.ambiguous.mean())
    same = (rb == o.rb).all(axis=1)
    print(f'{name}: {share:.2%} of {c.b} envs ambiguous; rb equal in {same.mean():.2%} of all envs; sinr_db rel_err on the others '
          f'{rel_err(sinr[ok], o.sinr_db[ok]):.3e}; rounds {rounds.min()}..{rounds.max()}, moves {moves.min()}..{moves.max()}, '
          f'converged {conv.mean():.0%}')
    assert share <= bu.CAP and ok.sum() >= 3
    if c.r > 64:                                                        # the reference's moves end in every block of RBs
        assert bu.covers(o.dest, c.r) and (c.n <= 1024 or o.moved[1024:].sum() > 0)
    assert np.array_equal(rb[ok], o.rb[ok])
    assert np.array_equal(rounds[ok], o.rounds[ok]) and np.array_equal(moves[ok], o.moves[ok])
    assert np.array_equal(conv[ok], o.converged[ok].astype(np.uint8))
    assert rel_err(sinr[ok], o.sinr_db[ok]) <= BAR


# ------------------------------------------------------------------------------------------ the example
def test_example_runs_and_the_dynamics_meet_more_targets_with_less_power():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'best_response_dynamics.py'), run_name='__main__')
    assert res['final_met'] > res['random_met'] and res['final_mw'] < res['random_mw']

"""Conflict-graph RB colouring on the GPU (csrc/d2d_color.hip; VecD2DEnv.color_graph, color_rbs, color_rbs_actions).

One yardstick, no tolerance: the NumPy restatement (color_util) fed the same tensors, downloaded - the conflict graph is float32
comparisons, the turns are integers, so all four outputs are compared for equality.  Every launch writes into guarded allocations
whose guard words are checked."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import color_util as cu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

NAMES = ('rb', 'conflicts', 'rbs_used', 'proper')
GUARD = 64                                          # guard elements on either side of an output
SENTINEL = {torch.int32: -1234567, torch.uint8: 0xA5}


def _guarded(shape, dtype):
    """(the whole allocation, the output inside it): GUARD sentinel elements before and behind."""
    total = int(np.prod(shape))
    whole = torch.full((total + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device='cuda')
    return whole, whole[GUARD:GUARD + total].view(shape)


def _intact(whole, dtype):
    return bool((whole[:GUARD] == SENTINEL[dtype]).all()) and bool((whole[-GUARD:] == SENTINEL[dtype]).all())


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _launch(c, pack):
    """d2d_color_graph on the case's tensors, uploaded; the four outputs on the host, the guards checked."""
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response import pack_allowed
    score, bias, thr, rb = _dev(c.score), _dev(c.tx_bias), _dev(c.rx_thr), _dev(c.rb)
    movable = None if c.movable is None else _dev(c.movable.astype(np.uint8))
    allowed = None if c.allowed is None else _dev(pack_allowed(c.allowed))
    shapes = ((c.b, c.n), (c.b,), (c.b,), (c.b,))
    dtypes = (torch.int32, torch.int32, torch.int32, torch.uint8)
    bufs = [_guarded(s, dt) for s, dt in zip(shapes, dtypes)]
    ptr = lambda t: 0 if t is None else t.data_ptr()
    _native.color_graph(ptr(score), ptr(bias), ptr(thr), ptr(rb), c.b, c.n, c.r, ptr(allowed), ptr(movable), pack,
                        *(o.data_ptr() for _, o in bufs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    for (whole, _), dt, name in zip(bufs, dtypes, NAMES):
        assert _intact(whole, dt), f'guard words of {name}'
    return tuple(o.cpu().numpy().copy() for _, o in bufs)


def _ref(c, pack):
    return cu.color_graph(c.score, c.tx_bias, c.rx_thr, c.rb, c.r, c.movable, c.allowed, pack)


def _same(got, want, what):
    for x, y, name in zip(got, want, NAMES):
        assert x.dtype == y.dtype and np.array_equal(x, y), f'{what}: {name}'


def _check(c, pack, what):
    got, want = _launch(c, pack), _ref(c, pack)
    turn = cu.turn_takers(c.n, c.r, c.movable, c.allowed)
    print(f'{what}, pack={pack}: {int(turn.sum())} of {c.n} links take a turn on {c.r} RBs; conflicts {want[1].tolist()}, rbs_used '
          f'{want[2].tolist()}, proper {want[3].tolist()}; LDS {cu.lds_bytes(c.n, c.r, c.allowed is not None)} bytes')
    _same(got, want, what)
    return got


def _case(score, thr, rb, r, bias=None, movable=None, allowed=None):
    score, thr, rb = np.asarray(score, dtype=np.float32), np.asarray(thr, dtype=np.float32), np.asarray(rb, dtype=np.int32)
    return SimpleNamespace(b=rb.shape[0], n=rb.shape[1], r=r, score=score, tx_bias=bias, rx_thr=thr, rb=rb, movable=movable, allowed=allowed)


# ------------------------------------------------------------------------------------------ color_graph on synthetic scores
@pytest.mark.parametrize('pack', [False, True])
@pytest.mark.parametrize('shape', list(cu.SHAPES), ids=lambda s: 'x'.join(map(str, s)))
def test_synthetic_scores_equal_the_restatement(shape, pack):
    c = cu.synthetic(*shape)
    got = _check(c, pack, 'x'.join(map(str, shape)))
    turn = cu.turn_takers(c.n, c.r, c.movable, c.allowed)
    assert np.array_equal(got[0][:, ~turn], c.rb[:, ~turn])            # background rows are copied through, -1, R and R + 5 too
    assert ((got[0][:, turn] >= 0) & (got[0][:, turn] < c.r)).all()
    if c.allowed is not None:
        for e in range(c.b):
            assert c.allowed[np.nonzero(turn)[0], got[0][e, turn]].all()
    if shape == (1, 800, 24):
        assert cu.lds_bytes(800, 24, False) > 64 * 1024                 # the dynamic-LDS attribute was needed


# ------------------------------------------------------------------------------------------ special graphs
@pytest.mark.parametrize('pack', [False, True])
def test_the_empty_and_the_complete_graph_are_decided_by_the_tie_rules(pack):
    n, r = 70, 4
    rb = np.full((1, n), -1)
    none = _check(_case(np.zeros((1, n, n)), np.ones((1, n)), rb, r), pack, 'the empty graph')
    assert none[0][0].tolist() == ([0] * n if pack else [i % r for i in range(n)])
    assert [int(x[0]) for x in none[1:]] == [0, 1 if pack else r, 1]
    for m, r, loads, conflicts in ((7, 3, [3, 2, 2], 5), (10, 4, [3, 3, 2, 2], 8), (5, 1, [5], 10), (70, 33, None, None)):
        full = _check(_case(np.ones((1, m, m)), np.zeros((1, m)), np.zeros((1, m)), r), pack, f'K{m} on {r} RBs')
        got = np.bincount(full[0][0], minlength=r)
        assert loads is None or (got.tolist() == loads and int(full[1][0]) == conflicts)
        assert got.max() - got.min() <= 1 and int(full[1][0]) == sum(int(k) * (int(k) - 1) // 2 for k in got) and int(full[3][0]) == 0


def test_a_one_directional_score_is_symmetrised():
    """Only d(i<-j) with i > j holds: the lower triangle.  Without the transpose link 0 would see no neighbour at all."""
    n, r = 67, 70
    score = np.tril(np.ones((n, n), dtype=np.float32), -1)[None]
    for pack in (False, True):
        got = _check(_case(score, np.full((1, n), 0.5), np.zeros((1, n)), r), pack, 'lower-triangular score')
        assert sorted(got[0][0].tolist()) == list(range(n)) and (int(got[1][0]), int(got[2][0]), int(got[3][0])) == (0, n, 1)
    upper = np.triu(np.ones((n, n), dtype=np.float32), 1)[None]
    got = _check(_case(upper, np.full((1, n), 0.5), np.zeros((1, n)), r), True, 'upper-triangular score')
    assert int(got[2][0]) == n


def test_nan_and_infinities_in_score_and_rx_thr():
    rng = np.random.default_rng(9)
    b, n, r = 3, 45, 6
    score = rng.normal(size=(b, n, n)).astype(np.float32)
    score[rng.random((b, n, n)) < 0.1] = np.nan
    score[rng.random((b, n, n)) < 0.05] = np.inf
    score[rng.random((b, n, n)) < 0.05] = -np.inf
    thr = (1.0 + 0.2 * rng.normal(size=(b, n))).astype(np.float32)
    thr[:, 1::6] = np.inf                                               # never a victim
    thr[:, 2::6] = -np.inf                                              # every entry that is not NaN conflicts
    thr[:, 3::6] = np.nan
    bias = rng.normal(size=(b, n)).astype(np.float32)
    bias[:, 5::11] = np.nan
    bias[:, 7::11] = -np.inf                                            # inf + -inf is NaN: false
    rb = rng.integers(0, r, size=(b, n))
    for pack in (False, True):
        _check(_case(score, thr, rb, r, bias=bias), pack, 'NaN and infinities')
        _check(_case(score, thr, rb, r), pack, 'NaN and infinities, no bias')


def test_nobody_takes_a_turn():
    c = cu.synthetic(2, 40, 5, half=True, masked=False, bias=True, density=0.2)
    c.movable = np.zeros(40, dtype=bool)
    got = _check(c, False, 'M = 0')
    assert np.array_equal(got[0], c.rb) and got[1].tolist() == [0, 0] and got[2].tolist() == [0, 0] and got[3].tolist() == [1, 1]
    c.movable = np.ones(40, dtype=bool)
    c.allowed = np.zeros((40, 5), dtype=bool)                           # movable, but nothing is allowed
    got = _check(c, True, 'M = 0 by the mask')
    assert np.array_equal(got[0], c.rb) and got[2].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------ batching
def test_an_env_of_a_batch_equals_a_launch_of_its_own_and_two_calls_agree():
    c = cu.synthetic(5, 90, 7, half=True, masked=True, bias=True, density=0.12)
    whole = _check(c, False, 'B = 5')
    again = _launch(c, False)
    for x, y in zip(whole, again):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for k in range(5):
        one = SimpleNamespace(**{**vars(c), 'b': 1, 'score': c.score[k:k + 1], 'tx_bias': c.tx_bias[k:k + 1], 'rx_thr': c.rx_thr[k:k + 1],
                                 'rb': c.rb[k:k + 1]})
        alone = _launch(one, False)
        for x, y, name in zip(alone, whole, NAMES):
            assert np.array_equal(x[0], y[k]), (k, name)


# ------------------------------------------------------------------------------------------ through the env
def _env(r, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': r, 'num_cues': 12, 'num_due_pairs': 25}, num_envs=8, **kw)
    env.reset(seed=4)
    return env


def _random_actions(env, rng):
    highs = env._initial_action_highs()
    return torch.as_tensor(np.stack([rng.integers(0, h, env.num_envs) for h in highs], axis=1).astype(np.int32), device=env.device)


def _env_ref(env, margin, movable, allowed, pack, power=None):
    """color_rbs() by the restatement on the downloaded coupling() and planes."""
    from gym_d2d_amd import coloring
    c = env.coupling().cpu().numpy()
    p = (env._t['pwr'] if power is None else power).cpu().numpy().astype(np.float32)
    thr = coloring.sir_threshold(c, p, margin)
    agent = env._agent_links()
    mov = agent if movable is None else agent & movable
    rb = env._t['rb'].cpu().numpy()
    return cu.color_graph(c, p, thr, rb, env.simulator.config.num_rbs, mov, allowed, pack), (c, p, thr, mov)


def _host(res):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().copy() for t in res)


def _margins_hold(env, res, margin, turn, power=None):
    """In every proper env, recomputed in torch: no same-RB pair with an end that took a turn breaks either margin."""
    c = env.coupling()
    p = (env._t['pwr'] if power is None else power).to(torch.float32)
    m = torch.as_tensor(margin, device=env.device)
    thr = (c.diagonal(0, 1, 2) + p) - m[None, :]
    hurts = (c + p[:, None, :]) >= thr[:, :, None]                      # [b, i, j]: j alone holds i under its margin
    n = env.num_links
    t = torch.as_tensor(turn, device=env.device)
    pair = (res.rb[:, :, None] == res.rb[:, None, :]) & ~torch.eye(n, dtype=torch.bool, device=env.device) & (t[:, None] | t[None, :])
    broken = (hurts & pair).flatten(1).any(dim=1)
    proper = res.proper != 0
    assert not bool((broken & proper).any())
    assert bool((broken == ~proper).all())                              # and an improper env does break one
    return int(proper.sum())


@pytest.mark.parametrize('r', [6, 40, 300])                     # 300: ten `allowed` words with a 12-bit tail, a second trip of the r loops
def test_color_rbs_equals_the_restatement_and_keeps_the_margins_where_proper(r):
    env = _env(r)
    try:
        rng = np.random.default_rng(r)
        env.step(_random_actions(env, rng))
        n = env.num_links
        movable = np.zeros(n, dtype=bool)
        movable[1::2] = True
        allowed = rng.random((n, r)) < 0.7
        allowed[5] = False
        per_link = np.where(np.arange(n) < 12, 3.0, 10.0).astype(np.float32)
        per_link[20] = -np.inf
        for margin_arg, margin, mov, al, pack in ((3.0, np.full(n, 3.0, np.float32), None, None, False),
                                                  (20.0, np.full(n, 20.0, np.float32), None, None, True),
                                                  ({'cue': 3.0, 'due': 10.0}, np.where(np.arange(n) < 12, 3.0, 10.0).astype(np.float32), movable, None, False),
                                                  (per_link, per_link, movable, allowed, True)):
            res = env.color_rbs(margin_arg, movable=mov, allowed=al, pack=pack)
            assert type(res).__name__ == 'ColoringResult' and res._fields == NAMES
            got = _host(res)
            want, (_, _, _, turn_mov) = _env_ref(env, margin, mov, al, pack)
            _same(got, want, f'color_rbs({margin_arg!r})')
            turn = cu.turn_takers(n, r, turn_mov, al)
            held = _margins_hold(env, res, margin, turn)
            print(f'{n} links on {r} RBs, margin {margin_arg!r}, pack={pack}: {int(turn.sum())} turns; proper envs {held} of 8; conflicts '
                  f'{got[1].tolist()}; rbs_used {got[2].tolist()}')
            if r == 40 and al is None:
                assert held == 8                                        # at most 36 neighbours on 40 RBs: always proper
        # another power plane: power_control()'s
        power = env.power_control(5.0).power_dbm.clone()
        res = env.color_rbs(8.0, power_dbm=power)
        want, _ = _env_ref(env, np.full(n, 8.0, np.float32), None, None, False, power)
        _same(_host(res), want, 'color_rbs(power_dbm=)')
        _margins_hold(env, res, np.full(n, 8.0, np.float32), cu.turn_takers(n, r, env._agent_links(), None), power)
    finally:
        env.close()


def test_color_graph_takes_any_tensors_honours_out_and_refuses_by_name():
    env = _env(6)
    try:
        b, n, r = 8, env.num_links, 6
        c = cu.synthetic(b, n, r, half=True, masked=True, bias=True, density=0.2)
        rb = env._t['rb'].cpu().numpy()
        want = cu.color_graph(c.score, c.tx_bias, c.rx_thr, rb, r, c.movable, c.allowed, True)
        score, thr, bias = _dev(c.score), _dev(c.rx_thr), _dev(c.tx_bias)
        res = env.color_graph(score, thr, bias, movable=c.movable, allowed=c.allowed, pack=True)
        _same(_host(res), want, 'color_graph()')
        assert env.color_graph(score, thr, bias, movable=c.movable, allowed=torch.as_tensor(c.allowed, device=env.device), pack=True).rb is res.rb
        shapes, dtypes = ((b, n), (b,), (b,), (b,)), (torch.int32, torch.int32, torch.int32, torch.uint8)
        bufs = [_guarded(s, dt) for s, dt in zip(shapes, dtypes)]
        out = tuple(o for _, o in bufs)
        got = env.color_graph(score, thr, bias, movable=c.movable, allowed=c.allowed, pack=True, out=out)
        assert all(x is y for x, y in zip(got, out))
        _same(_host(got), want, 'color_graph(out=)')
        assert all(_intact(whole, dt) for (whole, _), dt in zip(bufs, dtypes))
        _same(_host(env.color_graph(score, thr)), cu.color_graph(c.score, None, c.rx_thr, rb, r, None, None, False), 'the defaults')
        for kw, text in ((dict(out=(out[0], out[1], out[1], out[3])), 'out must be .* do not share memory'),
                         (dict(out=(out[0].long(), out[1], out[2], out[3])), r'out must be \(rb, conflicts, rbs_used, proper\)'),
                         (dict(out=out[:3]), 'out must be'), (dict(score=score.double()), 'score must be a contiguous float32'),
                         (dict(score=score.cpu()), 'score must be'), (dict(score=score[:, :, :n - 1]), 'score must be'),
                         (dict(rx_thr=thr[:4]), 'rx_thr must be'), (dict(tx_bias=bias.half()), 'tx_bias must be'),
                         (dict(movable=np.ones(n - 1, bool)), 'movable must be'), (dict(allowed=np.ones((n, r + 1), bool)), 'allowed must be'),
                         (dict(pack=None), 'pack must be')):
            a = dict(dict(score=score, rx_thr=thr, tx_bias=bias), **kw)
            with pytest.raises(ValueError, match=text):
                env.color_graph(**a)
        for bad in (float('nan'), {'cue': 1.0}, np.zeros(n - 1)):
            with pytest.raises(ValueError, match='margin_db'):
                env.color_rbs(bad)
        with pytest.raises(ValueError, match='power_dbm must be'):
            env.color_rbs(3.0, power_dbm=env._t['pwr'].float())
    finally:
        env.close()


@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_step_of_the_actions_exports_exactly_that_rb(cue_actions):
    env = _env(6, cue_actions=cue_actions)
    try:
        rng = np.random.default_rng(3)
        env.step(_random_actions(env, rng))
        first = env.num_links - env.num_agents
        assert first == (12 if cue_actions == 'traffic' else 0)
        for pack in (False, True):
            rb_before = env._t['rb'].clone()
            rb = env.color_rbs(6.0, pack=pack).rb.clone()
            pwr = env._t['pwr'].clone()
            assert torch.equal(rb[:, :first], rb_before[:, :first])    # links on fixed actions never move
            act = env.color_rbs_actions(6.0, pack=pack)
            assert tuple(act.shape) == (8, env.num_agents) and act.dtype == torch.int32
            _, _, _, info = env.step(act)
            assert torch.equal(info['rb'][:, first:], rb[:, first:]) and torch.equal(env._t['pwr'][:, first:], pwr[:, first:])
        if cue_actions == 'agent':                                      # one call picks RBs, the other picks powers
            levels = env._action_levels
            rb = env.color_rbs(6.0).rb.clone()
            mixed = (env.color_rbs_actions(6.0) // levels) * levels + env.power_control_actions({'cue': -4.0, 'due': 9.0}) % levels
            _, _, _, info = env.step(mixed.to(torch.int32))
            assert torch.equal(info['rb'], rb)
    finally:
        env.close()


def test_with_mobility_the_graph_is_the_one_of_the_moved_positions():
    from gym_d2d_amd.mobility import GaussMarkovMobility
    env = _env(6, mobility=GaussMarkovMobility(speed_std_mps=8.0, memory=0.7))
    try:
        rng = np.random.default_rng(5)
        before = env.coupling().clone()
        for _ in range(3):
            env.step(_random_actions(env, rng))
        assert not torch.equal(before, env.coupling())
        margin = np.full(env.num_links, 6.0, np.float32)
        res = env.color_rbs(6.0)
        want, _ = _env_ref(env, margin, None, None, False)
        _same(_host(res), want, 'after three moves')
        _margins_hold(env, res, margin, cu.turn_takers(env.num_links, 6, env._agent_links(), None))
    finally:
        env.close()


def test_what_cannot_be_served_is_refused_by_name():
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.path_loss import PathLoss, ShadowingPathLoss
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Foo(PathLoss):
        def __call__(self, tx, rx):
            return 20 * np.log10(tx.position.distance(rx.position)) + 40.0

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            for call in (lambda: env.color_rbs(3.0), lambda: env.color_rbs_actions(3.0), lambda: env.color_graph(None, None)):
                with pytest.raises(ValueError, match=text):
                    call()
            assert env._color is None
        finally:
            env.close()
    refused(r"color_rbs\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r'color_rbs\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r'color_rbs\(\).*export_actions', export_actions=False)
    refused(r'color_rbs\(\).*torch path', use_torch=False)


def test_the_example_runs_and_colouring_serves_more_pairs_than_rbs():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'graph_coloring.py'), run_name='__main__')['results']
    print(json.dumps(res, indent=1))
    many = res['many-to-one: 6 + 24 links on 8 RBs']
    assert many['assign_rbs()'] == 'ValueError' and all(np.isfinite(v).all() for k, v in many.items() if k != 'assign_rbs()')

"""Sum-capacity RB ascent on a path-loss table on the GPU (VecD2DEnv.rb_ascent_table, rb_ascent_table_actions,
csrc/d2d_tabascent.hip).

Two yardsticks.  EXACT, no tolerance: all seven outputs of ONE rb_ascent_table() call equal
table_rb_ascent_util.table_rb_ascent_by_evaluate, the statement as a host loop with one evaluate_table() launch per link turn, on
drawn tables (every entry on its own, not symmetric: a transposed or mis-pitched gain block shows), both entry widths, N and N + 1
rows.  REFERENCE: at the returned RBs of every converged env the float64 reference (the oracle's step formulas on the table) finds
no admissible RB that gains more than min_gain_mbps plus what the project's bar allows on the four group sums
(table_rb_ascent_util.reference_check; test_table_rb_ascent_cpu.py holds the share of checks left out under 25 % on the
restatement's own fixed point).  Then the domain word, the env routes ('channel', 'per_step', a native env with table=), the
untouched env and the refusals.

The figures of the build this was written on are in the docstring of the float64 test."""
import runpy
from pathlib import Path

import numpy as np
import pytest

import table_rb_ascent_util as tu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parent.parent

_cache = {}


def _env(cues, dues, r, b, model=None, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    cfg = {'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'seed': 4321}
    if model is not None:
        cfg['path_loss_model'] = model
    if cues + dues > 300:                                               # no [B, N, 6 N] observation block at these sizes
        from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
        cfg['obs_fn'] = SignalPlanesObsFunction
    return VecD2DEnv(cfg, num_envs=b, **kw)


def _build(name):
    """(env, case, table, rb, pwr) of a case: a NATIVE env of the case's shape - the table and the start state come with the call -
    and the case's arrays on the device; built once."""
    if name not in _cache:
        c = tu.make_case(name)
        env = _env(c.cues, c.dues, c.r, c.b)
        env.reset(seed=3)
        assert env.simulator.path_loss_table.route == 'native' and env.num_links == c.n
        _cache[name] = (env, c, *(torch.as_tensor(np.array(a), device=env.device) for a in (c.table, c.rb, c.pwr)))
    return _cache[name]


@pytest.fixture(scope='module', autouse=True)
def _close_envs():
    yield
    for env, *_ in _cache.values():
        env.close()
    _cache.clear()


def _host(res):
    torch.cuda.synchronize()                                            # raises if the device faulted
    return tuple(t.cpu().numpy().copy() for t in res)


def _same(got, want):
    for name, x, y in zip(tu.NAMES, got, want):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name


def _check_exact(name, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """One call against the host loop, word for word, and a second call against the first; returns the call's host arrays."""
    from gym_d2d_amd import _native
    env, c, table, rb, pwr = _build(name)
    want, calls = tu.table_rb_ascent_by_evaluate(env, table, rb, pwr, allowed, movable, floor, min_gain, max_rounds)
    before = _native.tabascent_launches
    got = _host(env.rb_ascent_table(table, rb, pwr, allowed, movable, floor, min_gain, max_rounds))
    assert _native.tabascent_launches == before + 1
    print(f'{name}: rounds {got[3].tolist()}, moves {got[4].tolist()}, converged {got[5].tolist()}, domain {got[6].tolist()}; '
          f'the host loop made {calls} evaluate_table() calls')
    _same(got, want)
    _same(_host(env.rb_ascent_table(table, rb, pwr, allowed, movable, floor, min_gain, max_rounds)), got)    # the same words again
    return got


# ------------------------------------------------------------------------------------------ 1: exact, against the host loop
@pytest.mark.parametrize('name', list(tu.CASES))
def test_the_cases_equal_the_host_loop_over_evaluate_table(name):
    from gym_d2d_amd import table_rb_ascent
    env, c, table, _, _ = _build(name)
    mov = tu.movable_mask(c)
    rb, sinr, cap, rounds, moves, conv, domain = _check_exact(name, movable=mov)
    assert str(table.dtype) == 'torch.' + c.dtype and tuple(table.shape) == (c.b, c.n + c.extra, c.n)
    assert (domain == 0).all()                                          # the NaN row of the live layout is never read
    on = (c.rb >= 0) & (c.rb < c.r)
    still = ~on | ~(np.ones(c.n, bool) if mov is None else mov)[None, :]
    assert np.array_equal(rb[still], c.rb[still]) and np.isfinite(sinr).all() and (cap > 0).any()
    if name == 'n3_r1':
        assert (moves == 0).all() and (conv == 1).all() and (rounds == 0).all() and np.array_equal(rb, c.rb)
    else:
        assert (moves > 0).any()
    if name == 'n20_r300':
        assert c.r > 256 and c.r % 32 != 0
    if name == 'n96_r2':
        assert max(np.bincount(rb[e], minlength=2).max() for e in range(c.b)) >= 40
    if name == 'n50_r6_no_rb':
        assert (~on).sum() == 2 * c.b and np.isfinite(sinr[~on]).all()               # evaluate_table()'s SNR for a link on no RB
    if name == 'n300_r7':
        assert c.n > 256 and (c.n + 31) // 32 == 10
    if name == 'n1000_r320':
        assert table_rb_ascent.lds_bytes(c.n, c.r) > 64 * 1024


@pytest.mark.parametrize('max_rounds', [16, 1, 2])
@pytest.mark.parametrize('floors', [False, True])
def test_n37_r5_equals_the_host_loop_with_floors_and_at_the_round_cap(floors, max_rounds):
    got = _check_exact('n37_r5', floor=tu.FLOORS if floors else None, max_rounds=max_rounds)
    assert (got[4] > 0).all()
    if max_rounds == 16:
        assert (got[5] == 1).all() and len(np.unique(got[3])) >= 2
    else:
        assert (got[5] == 0).any() and (got[3] <= max_rounds).all()


def test_n37_r5_min_gain_equals_the_host_loop():
    free = _check_exact('n37_r5_f32')
    gated = _check_exact('n37_r5_f32', min_gain=0.5)
    fl = _check_exact('n37_r5_f32', floor=tu.FLOORS, min_gain=0.5)
    # half a Mbps is a real bar: it stops moves
    assert (gated[4] <= free[4]).all() and (gated[4] < free[4]).any() and (gated[4] > 0).any() and (fl[4] > 0).any()


@pytest.mark.parametrize('name', ['n37_r5', 'n20_r300'])
def test_an_allowed_mask_and_a_movable_subset_equal_the_host_loop(name):
    import rb_ascent_util as ru
    env, c, _, _, _ = _build(name)
    allowed = ru.allowed_mask(c.n, c.r, 5, c.rb[0])
    movable = np.arange(c.n) % 4 != 2
    assert (~allowed.any(axis=1)).any() and allowed.any(axis=1).any()
    assert any(not allowed[i, c.rb[0, i]] and allowed[i].any() for i in range(c.n))          # a link that may only leave
    got = _check_exact(name, allowed, movable, tu.FLOORS)
    never = ~allowed.any(axis=1) | ~movable
    assert np.array_equal(got[0][:, never], c.rb[:, never]) and (got[4] > 0).any()
    moved = got[0] != c.rb
    assert allowed[np.nonzero(moved)[1], got[0][moved]].all()            # a link that moved sits on an allowed RB
    _check_exact(name, torch.as_tensor(allowed, device=env.device), torch.as_tensor(movable, device=env.device))


def test_the_table_layouts_and_entry_widths_give_the_words_their_entries_give():
    """The same entries as [B, N, N] and in the live layout [B, N + 1, N] (a -inf last row: it would raise the word if read) give the
    same words; float32 entries widened to float64 give the float32 table's words."""
    env, c, table, rb, pwr = _build('n37_r5_f32')
    first = _host(env.rb_ascent_table(table, rb, pwr, floor_sinr_db=tu.FLOORS))
    wide = torch.full((c.b, c.n + 1, c.n), float('-inf'), dtype=torch.float64, device=env.device)
    wide[:, :c.n] = table
    _same(_host(env.rb_ascent_table(wide, rb, pwr, floor_sinr_db=tu.FLOORS)), first)
    assert (first[6] == 0).all() and (first[4] > 0).any()


# ------------------------------------------------------------------------------------------ 2: the interface
def test_env_mask_out_and_two_calls():
    from guard_util import Guarded, bits
    from gym_d2d_amd import _native
    env, c, table, rb, pwr = _build('n37_r5')
    b, n = c.b, c.n
    call = lambda **kw: env.rb_ascent_table(table, rb, pwr, floor_sinr_db=tu.FLOORS, **kw)
    want = _host(call())
    own = call()
    assert all(x is y for x, y in zip(own, call()))                     # the env's one tuple, reused
    assert own.rb is own[0] and own.capacity_mbps is own[2] and own.converged is own[5] and own.domain is own[6]
    _same(_host(own), want)                                             # two calls, the same words
    shapes = ((b, n),) * 3 + ((b,),) * 4
    dtypes = (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8, torch.int32)
    guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
    out = tuple(g.array for g in guarded)
    got = call(out=out)
    assert all(x is y for x, y in zip(got, out))
    _same(_host(got), want)
    assert all(g.intact() for g in guarded)
    mask = np.arange(b) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
        before = [bits(g.array).copy() for g in guarded]
        got = _host(call(out=tuple(g.array for g in guarded), env_mask=m))
        for x, y, was in zip(got, want, before):
            assert np.array_equal(x[mask].view(np.uint8), y[mask].view(np.uint8))
            assert np.array_equal(x[~mask].view(np.uint8).ravel(), was.reshape(b, -1)[~mask].ravel())     # masked envs keep all seven rows
        assert all(g.intact() for g in guarded)
    launches = _native.tabascent_launches
    o = [torch.empty(s, dtype=dt, device=env.device) for s, dt in zip(shapes, dtypes)]
    shared = torch.empty(b, dtype=torch.int32, device=env.device)
    for bad in (o[:6], (*o[:3], shared, shared, *o[5:]), (*o[:6], torch.empty(b, dtype=torch.uint8, device=env.device)),
                (o[0], torch.empty((b, n + 1), device=env.device), *o[2:]), o[0],
                (o[0], torch.empty((b, 2 * n), device=env.device)[:, ::2], *o[2:]), (o[0].cpu(), *o[1:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, sinr_db, capacity_mbps, rounds, moves, converged, domain\)'):
            call(out=bad)
    with pytest.raises(ValueError, match='env_mask must be'):
        call(env_mask=np.ones(b + 1, bool))
    with pytest.raises(ValueError, match='allowed must be'):
        call(allowed=np.ones((n, c.r + 1), bool))
    with pytest.raises(ValueError, match='movable must be'):
        call(movable=np.ones(n + 1, bool))
    with pytest.raises(ValueError, match='floor_sinr_db'):
        env.rb_ascent_table(table, rb, pwr, floor_sinr_db={'cue': 1.0})
    with pytest.raises(ValueError, match='min_gain_mbps'):
        call(min_gain_mbps=-1.0)
    with pytest.raises(ValueError, match='max_rounds'):
        call(max_rounds=0)
    for bad in (table.cpu(), table[:, :, :-1], table.transpose(1, 2), table.to(torch.float16), table[:, :-2].contiguous(), table[0]):
        with pytest.raises(ValueError, match='table must be'):
            env.rb_ascent_table(bad, rb, pwr)
    for bad_rb, bad_pwr, text in ((rb.long(), pwr, 'rb must be'), (rb[:, :-1].contiguous(), pwr, 'rb must be'), (rb.cpu(), pwr, 'rb must be'),
                                  (rb, pwr.float(), 'power_dbm must be'), (rb, pwr[:-1].contiguous(), 'power_dbm must be')):
        with pytest.raises(ValueError, match=text):
            env.rb_ascent_table(table, bad_rb, bad_pwr)
    with pytest.raises(ValueError, match=r"rb_ascent_table\(\) has no live dB table.*'native'.*pass table="):
        env.rb_ascent_table()
    with pytest.raises(ValueError, match=r"rb_ascent_table\(\) has no live dB table.*'native'.*pass table="):
        env.rb_ascent_table_actions()
    assert _native.tabascent_launches == launches                       # refused before any launch


# ------------------------------------------------------------------------------------------ 3: the domain word
def test_the_domain_word_is_raised_for_exactly_the_envs_whose_block_holds_a_bad_entry():
    from guard_util import bits
    env, c, table, rb, pwr = _build('n37_r5')
    base = _host(env.rb_ascent_table(table, rb, pwr))
    bad = table.clone()
    # env 1: a NaN between two links, wherever they sit; env 4: a -inf in the last column of the last row of the block; env 2: a
    # +inf, which is a gain of 0 and no domain error; env 7: a -inf in row N, which is no part of the block
    bad[1, 3, 30], bad[4, c.n - 1, c.n - 1], bad[2, 5, 6], bad[7, c.n, 4] = float('nan'), float('-inf'), float('inf'), float('-inf')
    got = _host(env.rb_ascent_table(bad, rb, pwr))
    print('flagged envs:', np.flatnonzero(got[6]).tolist())
    assert got[6].tolist() == tu.domain_of(bad.cpu().numpy(), c.n).tolist() == [0, 1, 0, 0, 1] + [0] * (c.b - 5)
    untouched = np.ones(c.b, bool)
    untouched[[1, 2, 4]] = False
    for x, y in zip(got, base):
        assert np.array_equal(bits(x[untouched]), bits(y[untouched]))   # the other envs' words are unchanged
    # the +inf env is the host loop's on that table, and its word stays 0
    want, _ = tu.table_rb_ascent_by_evaluate(env, bad, rb, pwr)
    for x, y in zip(got, want):
        assert np.array_equal(bits(x[2]), bits(y[2]))
    assert got[6][2] == 0 and np.isfinite(got[1][2]).all()
    # a flagged env still ends (a NaN D is never chosen, a NaN gain does not move) and a masked env's word is not written
    assert (got[3][[1, 4]] <= 16).all()
    out = tuple(t.clone() for t in env.rb_ascent_table(table, rb, pwr))
    mask = np.ones(c.b, bool)
    mask[1] = False
    masked = _host(env.rb_ascent_table(bad, rb, pwr, out=out, env_mask=mask))
    assert masked[6].tolist() == [0, 0, 0, 0, 1] + [0] * (c.b - 5)
    assert all(np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(masked, base))


# ------------------------------------------------------------------------------------------ 4: through the env
def _channel_model(**kw):
    from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss
    return type('Channel', (SpatialChannelPathLoss,), dict(median=LogDistancePathLoss, median_kwargs={'ple': 3.5}, **kw))


def _per_step_model():
    from gym_d2d_amd.path_loss import ArrayPathLoss

    class EveryStep(ArrayPathLoss):
        """Evaluated on every step and drawing nothing: the table of the last step is the next step's."""
        per_step = True

        def compute(self, view):
            pl = 35.0 * view.xp.log10(view.distance()) + 30.0 + 0.01 * view.tx_column(lambda d: d.antenna_height_m)
            return pl, view.xp.diagonal(pl, dim1=1, dim2=2)
    return EveryStep


def _actions(env, rng):
    highs = env._initial_action_highs()
    return torch.as_tensor(np.stack([rng.integers(0, h, (env.num_envs,)) for h in highs], -1).astype(np.int32), device='cuda')


def _eq(a, m):
    return a.shape == m.shape and bool(torch.equal(a.contiguous().view(torch.int32), m.contiguous().view(torch.int32)))


def _through_the_env(env, route, monkeypatch):
    from guard_util import bits
    from gym_d2d_amd import _native
    opened = []
    load = _native.load_tabascent_library
    monkeypatch.setattr(_native, 'load_tabascent_library', lambda: opened.append(1) or load())
    rng = np.random.default_rng(5)
    env.reset(seed=11)
    env.step(_actions(env, rng))
    table = env.simulator.path_loss_table
    live = table.live
    assert table.route == route and tuple(live.shape) == (env.num_envs, env.num_links + 1, env.num_links)
    env.evaluate_table(env._t['rb'][:, None].contiguous(), env._t['pwr'][:, None].contiguous())
    assert opened == [] and env._table_rbascent is None                 # nothing of this API has been asked for yet
    names = [k for k in ('rb', 'pwr', 'pos_x', 'pos_y', 'reward', 'sinr_db', 'snr_db', 'rate_bps', 'capacity_mbps', 'env_flags')
             if env._t.get(k) is not None]
    torch.cuda.synchronize()
    before = {k: env._t[k].clone() for k in names}
    tab0, steps, flags, fills = live.clone(), env.num_steps, env.status_flags(), _native.channel_launches
    # all defaults = the explicit call = the host loop
    default = tuple(t.clone() for t in env.rb_ascent_table(floor_sinr_db=tu.FLOORS))
    assert opened != []
    explicit = env.rb_ascent_table(table=live, rb=env._t['rb'], power_dbm=env._t['pwr'], floor_sinr_db=tu.FLOORS)
    _same(_host(explicit), _host(default))
    want, _ = tu.table_rb_ascent_by_evaluate(env, None, env._t['rb'], env._t['pwr'], floor=tu.FLOORS)
    _same(_host(default), want)
    assert int(default[4].sum()) > 0 and int(default[6].sum()) == 0
    # the env is untouched: planes, counters and the table
    torch.cuda.synchronize()
    assert env.num_steps == steps and env.status_flags() == flags and _native.channel_launches == fills
    assert env.simulator.path_loss_table.live is live and np.array_equal(bits(live), bits(tab0))
    for k in names:
        assert np.array_equal(bits(env._t[k]), bits(before[k])), k
    # nothing moves and nothing is drawn: the step on the solved RBs exports the solver's planes, bit for bit
    actions = env.rb_ascent_table_actions(floor_sinr_db=tu.FLOORS)
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (env.num_envs, env.num_agents)
    _, _, _, info = env.step(actions)
    assert torch.equal(info['rb'], default[0]) and torch.equal(info['tx_pwr_dbm'], before['pwr'])
    assert _eq(info['sinr_db'], default[1]) and _eq(info['capacity_mbps'], default[2])
    assert env.status_flags() == 0


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
def test_on_the_channel_route_the_defaults_are_the_live_table_and_the_step_delivers_the_solvers_planes(dtype, monkeypatch):
    env = _env(6, 14, 5, 4, _channel_model(fading=None, table_dtype=dtype, num_sinusoids=8))
    try:
        _through_the_env(env, 'channel', monkeypatch)
        assert str(env.simulator.path_loss_table.live.dtype) == 'torch.' + dtype
    finally:
        env.close()


def test_on_the_per_step_route_likewise(monkeypatch):
    env = _env(6, 14, 5, 4, _per_step_model())
    try:
        _through_the_env(env, 'per_step', monkeypatch)
    finally:
        env.close()


def test_a_native_env_without_exported_actions_is_served_with_table_rb_and_power():
    c = tu.make_case('n37_r5')
    env = _env(c.cues, c.dues, c.r, c.b, export_actions=False)
    try:
        env.reset(seed=3)
        table, rb, pwr = (torch.as_tensor(np.array(a), device=env.device) for a in (c.table, c.rb, c.pwr))
        for kw in (dict(), dict(rb=rb), dict(power_dbm=pwr)):
            with pytest.raises(ValueError, match=r'rb_ascent_table\(\).*export_actions=True, or pass rb= and power_dbm='):
                env.rb_ascent_table(table, **kw)
        with pytest.raises(ValueError, match=r'rb_ascent_table_actions\(\).*export_actions=True'):
            env.rb_ascent_table_actions(table)
        got = _host(env.rb_ascent_table(table, rb, pwr, floor_sinr_db=tu.FLOORS))
        # the words of the env that exports its actions: the start state came with the call in both
        other, _, t2, rb2, pwr2 = _build('n37_r5')
        _same(got, _host(other.rb_ascent_table(t2, rb2, pwr2, floor_sinr_db=tu.FLOORS)))
        with pytest.raises(ValueError, match=r'rb_ascent\(\).*export_actions'):
            env.rb_ascent()
    finally:
        env.close()


def test_rb_ascent_keeps_refusing_the_table_routes_and_a_shape_past_160_kib_is_refused_in_bytes():
    from gym_d2d_amd import _native, table_rb_ascent
    env = _env(3, 3, 4, 2, _channel_model(fading=None, num_sinusoids=8))
    try:
        env.reset(seed=1)
        with pytest.raises(ValueError) as info:
            env.rb_ascent()
        assert str(info.value) == ("rb_ascent() does not serve the 'channel' path-loss route (a table, not a law its kernel can evaluate "
                                   'for the RBs no step has applied); it serves the native power-law models')
        assert env._rbascent is None
    finally:
        env.close()
    need = table_rb_ascent.lds_bytes(2048, 384)
    assert need > _native.TABASCENT_MAX_LDS_BYTES
    env = _env(512, 1536, 384, 1)
    try:
        env.reset(seed=1)
        before = _native.tabascent_launches
        with pytest.raises(ValueError, match=rf'rb_ascent_table\(\).*2048 links on 384 RBs need {need} bytes, more than 163840'):
            env.rb_ascent_table(torch.zeros((1, 2048, 2048), device=env.device))
        assert _native.tabascent_launches == before and env._table_rbascent is None
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 5: the float64 reference
@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n37_r5_f32', True), ('n50_r6_no_rb', False)])
def test_no_admissible_rb_gains_more_than_the_bar_allows_in_float64(name, floors):
    """The figures of the build this was written on (the largest left side less min_gain, over the allowed slack; <= 1 passes) are
    recorded in CHANGELOG.md and DESIGN.md 4.27."""
    env, c, table, rb0, pwr = _build(name)
    floor = tu.FLOORS if floors else None
    rb, sinr, cap, rounds, moves, conv, domain = _host(env.rb_ascent_table(table, rb0, pwr, floor_sinr_db=floor))
    assert conv.any() and (domain == 0).all()
    chk = tu.reference_check(c, np.arange(c.b), rb, conv.astype(bool), None, None, floor, 0.0)
    print(f'{name} floors={floors}: checks {chk.checks}, left_out {chk.left_out}, worst {chk.worst:.3e} of the allowed slack')
    assert chk.checks > 500 and chk.left_out <= tu.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 1.0


# ------------------------------------------------------------------------------------------ 6: the example
def test_the_example_gains_on_random_actions_and_the_step_delivers_it():
    res = runpy.run_path(str(ROOT / 'examples' / 'channel_rb_ascent.py'), run_name='__main__')['results']
    assert res['random_mbps'].shape == res['rb_ascent_table_mbps'].shape == res['delivered_mbps'].shape == (64,)
    assert (res['rb_ascent_table_mbps'] >= res['random_mbps']).all() and (res['rb_ascent_table_mbps'] > res['random_mbps']).any()
    assert np.array_equal(res['delivered_mbps'], res['rb_ascent_table_mbps'])     # the same planes, summed the same way
    assert int(res['domain']) == 0

"""Unilateral-deviation gains on the GPU (VecD2DEnv.deviation_gains, best_deviation, best_deviation_actions,
csrc/d2d_deviate.hip).

Two yardsticks.  EXACT, no tolerance: the table of ONE deviation_gains() launch and the five outputs of one best_deviation() call
equal deviation_util.by_evaluate, the statement in NumPy on the float32 planes of env.evaluate() launches - one per selected link
with R Lmax + 1 candidates - word for word, on the smallest shapes at which the kernel can go wrong.  REFERENCE: the table against
the float64 oracle (deviation_util.by_oracle) to the project's 1e-5 bar, |d| <= 1e-5 max(|ref|, 1), on the entries that carry no
near-threshold mark, and openness on the same entries; test_deviation_cpu.py holds the marks under 1 % of every case's entries."""
import numpy as np
import pytest

import deviation_util as du

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

_cache = {}
GUARD = 0x5A5A5A5A
MIN_GAIN = 0.5                                       # Mbps: holds some links back, asserted


def _build(case, cue_actions='agent'):
    """The env of a case, stepped once on the case's layout with the case's actions; built once."""
    key = (case, cue_actions)
    if key not in _cache:
        from gym_d2d_amd.envs import VecD2DEnv
        c = du.make_case(case)
        env = VecD2DEnv(du.env_config(c), num_envs=c.b, cue_actions=cue_actions)
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


def _words(x):
    return np.ascontiguousarray(x).view(np.uint8)


def _same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_words(got), _words(want)), (name, int((_words(got) != _words(want)).sum()))


def _links_of(case, c):
    """The selection of a case: every agent link, or - SUBSET_CASE - a non-contiguous subset."""
    return None if case != du.SUBSET_CASE else np.array([j for j in range(c.n) if j % 3 == 1 or j in (0, 64, 65, c.n - 1)])


def _check_exact(env, c, links, settings):
    """One deviation_gains() launch and one best_deviation() call per setting against the statement on evaluate()'s planes, word
    for word.  settings: (allowed, floor, min_gain).  Returns [(the table, best_deviation's host arrays, the restatement)]."""
    from gym_d2d_amd import _native
    wants, calls = du.by_evaluate(env, links, settings)
    out = []
    for (allowed, floor, min_gain), want in zip(settings, wants):
        before = _native.deviate_launches
        table, sel, levels = _host(env.deviation_gains(links, allowed, floor))
        best = _host(env.best_deviation(links, allowed, floor, min_gain))
        assert _native.deviate_launches == before + 2
        _same('links', sel, want.links.astype(np.int32))
        _same('levels', levels, (c.p_max - c.p_min + 1)[want.links].astype(np.int32))
        _same('table', table, want.table)
        for name, x, y in zip(('rb', 'power_dbm', 'gain_mbps', 'regret_mbps', 'leader'), best,
                              (want.rb_out, want.pwr_out, want.gain_link, want.regret, want.leader)):
            _same(name, x, y)
        out.append((table, best, want))
    print(f'{calls} evaluate() calls; table {list(out[0][0].shape)}, closed {[float(np.isinf(t).mean().round(3)) for t, _, _ in out]}, '
          f'movers {[int((b[2] > 0).sum()) for _, b, _ in out]}, regret {[b[3].round(3).tolist() for _, b, _ in out]}')
    return out


# ------------------------------------------------------------------------------------------ 1: exact, against evaluate()
@pytest.mark.parametrize('case', list(du.CASES))
def test_table_and_best_deviation_equal_the_statement_on_evaluate_planes(case):
    from gym_d2d_amd import deviation
    env, c, _ = _build(case)
    links = _links_of(case, c)
    floors = du.FLOOR_SETTINGS
    res = _check_exact(env, c, links, [(None, floors['none'], 0.0), (None, floors['cue0'], 0.0), (None, floors['below'], 0.0),
                                       (None, floors['below'], MIN_GAIN)])
    free, cue0, below, gated = res
    assert env._deviation.law == du.LAWS[c.law]
    # floors close entries, never open one; min_gain holds some links back and moves nobody else
    assert not (cue0[2].open & ~free[2].open).any() and (below[2].open != free[2].open).any()
    if case != 'd40_r1':                             # (one RB, every link in one group: few gains reach half a Mbps)
        assert 0 < (gated[1][2] > 0).sum() < (below[1][2] > 0).sum()
    assert ((gated[1][2] > 0) <= (below[1][2] > 0)).all() and (gated[1][2][gated[1][2] > 0] > MIN_GAIN).all()
    on = (c.rb >= 0) & (c.rb < c.r)
    sel = np.arange(c.n) if links is None else links
    for table, best, want in res:
        held = np.zeros(table.shape, bool)
        for a, i in enumerate(sel):
            for e in range(c.b):
                if on[e, i]:
                    held[e, a, c.rb[e, i], c.pwr[e, i] - c.p_min[i]] = True
        assert (_words(table[held]) == _words(np.zeros(held.sum(), np.float32))).all()         # +0.0 on the held action
        assert np.isinf(table[:, :, :, :][~np.broadcast_to(on[:, sel][:, :, None, None], table.shape)]).all()
        assert (best[4] == -1).all() == (best[3] == 0.0).all()
    # what the case is there for
    size = max(np.bincount(c.rb[e][on[e]], minlength=c.r).max() for e in range(c.b))
    if case == 'd6_r4':
        assert c.r * free[0].shape[3] * 1 < 256 and free[0].shape[3] == 24
    if case == 'd50_r25':
        assert (~on).any() and np.isinf(free[0][~on[:, sel]]).all() and (free[1][2][~on] == 0).all()        # a link on no RB
    if case == du.SUBSET_CASE:
        assert c.r % 32 != 0 and (c.r + 31) // 32 == 3 and (np.diff(sel) > 1).any() and len(sel) < c.n
        untouched = np.setdiff1d(np.arange(c.n), sel)
        assert np.array_equal(free[1][0][:, untouched], c.rb[:, untouched]) and (free[1][2][:, untouched] == 0).all()
    if case == 'd40_r1':
        assert c.r == 1 and size == 40
    if case == 'd40_r2':
        assert size > 32
    if case == 'd16_r8_lv':
        lv = (c.p_max - c.p_min + 1)
        assert set(lv) == {64, 1} and free[0].shape[3] == 64
        assert np.isinf(free[0][:, lv[sel] == 1][:, :, :, 1:]).all()                           # padding: the columns behind L_i are closed
        assert np.isfinite(free[0][:, lv[sel] == 1][:, :, :, 0]).all()                         # an all-RB row, one level
    if case == 'd300_r8':
        assert size > 32 and c.n * c.r * 24 > 2 * 4096 and deviation.lds_bytes(c.n, c.r) == du.lds_bytes(c.n, c.r)
    assert any((want.rows[e][a].on and (want.rows[e][a].adm.sum() < want.rows[e][a].adm.size))
               for e in range(c.b) for a in range(len(sel))) or case in ('d40_r1',), 'the floors close something'
    # some link starts below its floor
    fl = du.floor_vector(floors['below'], c.cues, c.dues)
    sinr = env.evaluate(env._t['rb'][:, None, :].contiguous(), env._t['pwr'][:, None, :].contiguous())['sinr_db'][:, 0].cpu().numpy()
    assert (sinr[on] < np.broadcast_to(fl, sinr.shape)[on]).any()


@pytest.mark.parametrize('case', ['d6_r4', du.SUBSET_CASE, 'd16_r8_lv'])
def test_an_allowed_mask_equals_the_statement(case):
    env, c, _ = _build(case)
    links = _links_of(case, c)
    allowed = du.allowed_mask(c.n, c.r, 5, c.rb[0])
    assert (~allowed.any(axis=1)).any() and any(0 <= c.rb[0, i] < c.r and not allowed[i, c.rb[0, i]] for i in range(c.n))
    (table, best, want), = _check_exact(env, c, links, [(allowed, du.FLOOR_SETTINGS['below'], 0.0)])
    sel = np.arange(c.n) if links is None else links
    on = (c.rb >= 0) & (c.rb < c.r)
    for a, i in enumerate(sel):
        for e in range(c.b):
            closed = ~allowed[i].copy()
            if on[e, i]:
                closed[c.rb[e, i]] = False                               # the held RB is open whatever allowed says
            assert np.isinf(table[e, a][closed]).all()
    moved = best[2] > 0
    assert moved.any() and all(allowed[i, best[0][e, i]] or best[0][e, i] == c.rb[e, i] for e, i in zip(*np.nonzero(moved)))
    # a tensor mask gives the same words
    t2 = _host(env.deviation_gains(links, torch.as_tensor(allowed, device=env.device), du.FLOOR_SETTINGS['below']))[0]
    _same('table', t2, table)


def test_one_launch_for_all_links_fills_the_same_planes():
    env, c, _ = _build('d6_r4')
    (a,), calls_a = du.by_evaluate(env, None, [(None, du.FLOOR_SETTINGS['below'], 0.0)])
    (b,), calls_b = du.by_evaluate(env, None, [(None, du.FLOOR_SETTINGS['below'], 0.0)], one_launch=True)
    assert calls_a == c.n and calls_b == 1
    _same('table', a.table, b.table)
    _same('gain', a.gain_link, b.gain_link)


# ------------------------------------------------------------------------------------------ 2: masks, out=, repeatability
def test_env_mask_and_out_leave_masked_rows_and_guards_untouched_and_two_calls_give_the_same_words():
    env, c, _ = _build('d50_r25')
    b, n, r = c.b, c.n, c.r
    floor = du.FLOOR_SETTINGS['below']
    own_t = _host(env.deviation_gains(None, None, floor))[0]
    own_b = _host(env.best_deviation(None, None, floor))
    _same('table', _host(env.deviation_gains(None, None, floor))[0], own_t)        # two calls, the same words
    for name, x, y in zip('abcde', _host(env.best_deviation(None, None, floor)), own_b):
        _same(name, x, y)
    m, lmax = own_t.shape[1], own_t.shape[3]
    mask = np.array([1, 0, 1, 0], dtype=bool)
    # out= inside a guarded arena
    count = b * m * r * lmax
    arena = torch.full((count + 64,), GUARD, dtype=torch.int32, device=env.device)
    out = arena[32:32 + count].view(torch.float32).view(b, m, r, lmax)
    got = env.deviation_gains(None, None, floor, out=out, env_mask=mask)[0]
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    assert (host[:32] == GUARD).all() and (host[32 + count:] == GUARD).all()
    tab = host[32:32 + count].view(np.float32).reshape(b, m, r, lmax)
    _same('live rows', tab[mask], own_t[mask])
    assert (tab[~mask].view(np.int32) == GUARD).all()
    # best_deviation: five guarded outputs
    shapes = ((b, n), (b, n), (b, n), (b,), (b,))
    dtypes = (torch.int32, torch.int32, torch.float64, torch.float64, torch.int32)
    arenas = [torch.full((int(np.prod(s)) + 16,), GUARD, dtype=torch.int32 if dt != torch.float64 else torch.int64, device=env.device)
              for s, dt in zip(shapes, dtypes)]
    outs = tuple(a[8:8 + int(np.prod(s))].view(dt).view(s) for a, s, dt in zip(arenas, shapes, dtypes))
    env.best_deviation(None, None, floor, 0.0, out=outs, env_mask=torch.as_tensor(mask, device=env.device))
    torch.cuda.synchronize()
    for a, s, dt, want in zip(arenas, shapes, dtypes, own_b):
        host = a.cpu().numpy()
        k = int(np.prod(s))
        assert (host[:8] == GUARD).all() and (host[8 + k:] == GUARD).all()
        body = host[8:8 + k].view(want.dtype).reshape(s)
        _same('live rows', body[mask], want[mask])
        assert (host[8:8 + k].reshape((b, -1))[~mask] == GUARD).all()
    with pytest.raises(ValueError, match='out must be'):
        env.deviation_gains(None, None, floor, out=out.view(b, m, r * lmax))
    with pytest.raises(ValueError, match='out must be'):
        env.best_deviation(None, None, floor, out=outs[:4])


# ------------------------------------------------------------------------------------------ 3: through step()
@pytest.mark.parametrize('case', ['d6_r4', 'd16_r8_lv'])
def test_steepest_ascent_through_step_raises_the_total_by_the_regret_and_ends_at_regret_zero(case):
    env, c, raw = _build(case)                                          # no mobility=: the next step sees the positions the gains were taken at
    try:
        total = du.sequential_sum(env.step(raw)[3]['capacity_mbps'].cpu().numpy(), axis=1)
        steps = 0
        while True:
            res = _host(env.best_deviation())
            actions = env.best_deviation_actions()
            assert actions.dtype == torch.int32 and tuple(actions.shape) == (c.b, env.num_agents)
            regret, leader = res[3], res[4]
            if (regret == 0.0).all():
                assert (leader == -1).all()
                break
            assert ((leader == -1) == (regret == 0.0)).all()
            info = env.step(actions)[3]
            new = du.sequential_sum(info['capacity_mbps'].cpu().numpy(), axis=1)
            print(f'step {steps}: regret {regret.round(4).tolist()}, leader {leader.tolist()}, total {new.round(4).tolist()}')
            assert (np.abs(new - total - regret) <= 1e-9 * np.maximum(np.abs(total), np.abs(new))).all()
            # only the leader moved
            rb_now, pw_now = info['rb'].cpu().numpy(), info['tx_pwr_dbm'].cpu().numpy()
            for e in range(c.b):
                want_rb, want_pw = res[0][e].copy(), res[1][e].copy()
                keep = np.arange(c.n) != leader[e]
                assert np.array_equal(rb_now[e][~keep], want_rb[~keep]) and np.array_equal(pw_now[e][~keep], want_pw[~keep])
            total = new
            steps += 1
            assert steps < 400
        assert steps > 0
        again = env.step(env.best_deviation_actions())[3]                # leader -1 everywhere: the actions repeat
        assert np.array_equal(again['rb'].cpu().numpy(), rb_now) and np.array_equal(again['tx_pwr_dbm'].cpu().numpy(), pw_now)
    finally:
        env.step(raw)                                                   # the case's own actions back


def test_links_on_fixed_actions_are_never_selected():
    env, c, raw = _build('d6_r4', cue_actions='traffic')
    table, sel, levels = _host(env.deviation_gains())
    assert env.num_agents == c.dues and np.array_equal(sel, np.arange(c.cues, c.n)) and table.shape[1] == c.dues
    (want,), _ = du.by_evaluate(env, None, [(None, None, 0.0)])
    _same('table', table, want.table)
    with pytest.raises(ValueError, match='fixed actions'):
        env.deviation_gains(links=[0, c.cues])
    actions = env.best_deviation_actions()
    assert tuple(actions.shape) == (c.b, c.dues)


# ------------------------------------------------------------------------------------------ 4: the float64 cross-check
@pytest.mark.parametrize('floors', ['none', 'below'])
@pytest.mark.parametrize('case', [k for k in du.CASES if du.CASES[k]['oracle'] is not None])
def test_the_table_holds_the_bar_against_the_float64_oracle(case, floors):
    env, c, _ = _build(case)
    envs, links = du.oracle_links(case)
    ref = du.oracle_side(case, floors)
    table = _host(env.deviation_gains(list(links), None, du.FLOOR_SETTINGS[floors]))[0][envs]
    keep = ~ref.near
    assert ref.near.mean() <= du.MARK_CAP
    assert np.array_equal(np.isfinite(table)[keep], ref.open[keep])                # openness, on every unmarked entry
    both = keep & ref.open
    err = np.abs(table[both].astype(np.float64) - ref.gain[both]) / np.maximum(np.abs(ref.gain[both]), 1.0)
    print(f'{case} {floors}: {both.sum()} open entries compared, {ref.near.sum()} marked, worst error {err.max():.3e} of the bar {du.BAR:.0e}')
    assert err.max() <= du.BAR


# ------------------------------------------------------------------------------------------ 5: the example
def test_the_example_runs_and_steepest_ascent_ends_at_regret_zero_above_the_random_total():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'deviation_gains.py'), run_name='__main__')['results']
    assert (res['steepest_ascent_regret_mbps'] == 0.0).all() and 0 < res['steepest_steps'] < 400
    assert (res['random_regret_mbps'] > 0.0).all() and (res['steepest_ascent_mbps'] > res['random_mbps']).all()
    assert (res['alternating_mbps'] > res['random_mbps']).all() and (res['alternating_regret_mbps'] >= 0.0).all()

"""Sum-capacity RB ascent on the GPU (VecD2DEnv.rb_ascent, rb_ascent_actions, csrc/d2d_rbascent.hip).

Two yardsticks.  EXACT, no tolerance: all six outputs of ONE rb_ascent() launch equal rb_ascent_util.rb_ascent_by_evaluate, the
statement as a host loop with one evaluate() launch per link turn, and the two planes equal evaluate(rb, pwr)'s for every link.
REFERENCE: at the returned RBs of every converged env the float64 oracle finds no admissible RB that gains more than min_gain_mbps
plus what the project's bar allows on the four group sums (rb_ascent_util.reference_check; test_rb_ascent_cpu.py holds the share of
checks left out under 25 % on the restatement's own fixed point)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import power_control_util as pcu
import rb_ascent_util as ru

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

_cache = {}


def _state(case):
    if case == pcu.MIXED[0]:
        cues, dues, r = pcu.MIXED[1]
        pos, raw, rb, pwr = pcu.state(cues, dues, r, 77)
        p_min, p_max, levels = pcu.bounds(cues, dues)
        return SimpleNamespace(name=case, cues=cues, dues=dues, n=cues + dues, r=r, law='mixed', cell=500.0, b=pcu.B, pos=pos, raw=raw,
                               rb=rb, pwr=pwr, p_min=p_min, p_max=p_max, levels=levels)
    return ru.make_case(case)


def _build(case, b, cue_actions='agent'):
    """The env of a case on its first b envs, stepped once on the case's layout with the case's actions; built once."""
    key = (case, b, cue_actions)
    if key not in _cache:
        from gym_d2d_amd.envs import VecD2DEnv
        c = _state(case)
        cfg = {'num_rbs': c.r, 'num_cues': c.cues, 'num_due_pairs': c.dues, 'path_loss_model': pcu.models()[c.law][0]}
        if c.n > 300:                                                   # no [B, N, 6 N] observation block at these sizes
            from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
            cfg['obs_fn'] = SignalPlanesObsFunction
        env = VecD2DEnv(cfg, num_envs=b, cue_actions=cue_actions)
        env.reset(seed=3)
        env.simulator.set_positions(c.pos[:b])
        first = c.n - env.num_agents
        raw = torch.as_tensor(np.ascontiguousarray(c.raw[:b, first:]), device=env.device)
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


NAMES = ('rb', 'sinr_db', 'capacity_mbps', 'rounds', 'moves', 'converged')


def _same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name


def _check_exact(env, allowed=None, movable=None, floor=None, min_gain=0.0, max_rounds=16):
    """One launch against the host loop, word for word; returns the launch's host arrays."""
    from gym_d2d_amd import _native
    want, calls = ru.rb_ascent_by_evaluate(env, allowed, movable, floor, min_gain, max_rounds)
    before = _native.rbascent_launches
    got = _host(env.rb_ascent(allowed, movable, floor, min_gain, max_rounds))
    assert _native.rbascent_launches == before + 1
    print(f'rounds {got[3].tolist()}, moves {got[4].tolist()}, converged {got[5].tolist()}; the host loop made {calls} evaluate() calls')
    _same(got, want)
    return got


def _total(env, rb):
    """The host double sum of evaluate()'s capacity plane at the RBs rb [B, N] (host or device) and the held powers, per env."""
    rb = torch.as_tensor(np.asarray(rb), device=env.device) if not torch.is_tensor(rb) else rb
    cap = env.evaluate(rb[:, None, :].to(torch.int32).contiguous(), env._t['pwr'][:, None, :].contiguous())['capacity_mbps']
    torch.cuda.synchronize()
    return ru.sequential_sum(cap.cpu().numpy()[:, 0], axis=1)


# ------------------------------------------------------------------------------------------ 1: exact, against the host loop
@pytest.mark.parametrize('max_rounds', [16, 1, 2])
@pytest.mark.parametrize('floors', [False, True])
def test_n37_r5_equals_the_host_loop_over_evaluate(floors, max_rounds):
    env, c, _ = _build('n37_r5', 16)
    got = _check_exact(env, floor=ru.FLOORS if floors else None, max_rounds=max_rounds)
    assert (got[4] > 0).all()
    if max_rounds == 16:
        assert (got[5] == 1).all() and len(np.unique(got[3])) >= 2
    else:
        assert (got[5] == 0).any() and (got[3] <= max_rounds).all()


def test_n37_r5_min_gain_equals_the_host_loop_over_evaluate():
    env, c, _ = _build('n37_r5', 16)
    free = _check_exact(env)
    gated = _check_exact(env, min_gain=0.5)
    fl = _check_exact(env, floor=ru.FLOORS, min_gain=0.5)
    # half a Mbps is a real bar: it stops most moves, and in some env all of them
    assert (gated[4] <= free[4]).all() and (gated[4] < free[4]).any() and (gated[4] > 0).any() and (fl[4] > 0).any()


@pytest.mark.parametrize('name', ['n20_r64', 'n20_r300', 'n96_r2', 'n96_r1', 'n50_r6_hata', 'n50_r6_ld35', 'n50_r6_no_rb', 'n300_r7',
                                  'n1000_r64_ld35'])
def test_the_cases_equal_the_host_loop_over_evaluate(name):
    from gym_d2d_amd import rb_ascent
    case, b, every = ru.CASES[name]
    env, c, _ = _build(case, b)
    mov = None if every == 1 else ru.movable_mask(c.n, every)
    got = _check_exact(env, movable=mov)
    rb, sinr, cap, rounds, moves, conv = got
    on = (c.rb[:b] >= 0) & (c.rb[:b] < c.r)
    still = ~on | ~(np.ones(c.n, bool) if mov is None else mov)[None, :]
    assert np.array_equal(rb[still], c.rb[:b][still])
    if name == 'n96_r1':
        assert (moves == 0).all() and (conv == 1).all() and (rounds == 0).all() and np.array_equal(rb, c.rb[:b])
    elif name in ('n20_r64', 'n20_r300'):
        assert c.r > c.n and (moves > 0).any()                          # most links are alone already: an empty RB gains them nothing
    else:
        assert (moves > 0).all()
    if name == 'n20_r300':
        assert c.r > 256 and c.r % 32 != 0
    if name == 'n96_r2':
        assert max(np.bincount(rb[e], minlength=2).max() for e in range(b)) >= 40
    if name == 'n50_r6_no_rb':
        assert (~on).any() and np.isfinite(sinr[~on]).all()                         # evaluate()'s SNR for a link on no RB
    if name == 'n300_r7':
        assert c.n > 256 and (c.n + 31) // 32 == 10
    if name == 'n1000_r64_ld35':
        assert rb_ascent.lds_bytes(c.n, c.r, True) > 64 * 1024 and env._rbascent.law != 0
    if name in ('n50_r6_hata', 'n50_r6_ld35'):
        assert env._rbascent.law == 2


def test_the_general_power_law_equals_the_host_loop_over_evaluate():
    env, c, _ = _build(*ru.MIXED[:2])
    got = _check_exact(env)
    assert env._rbascent.law == 1 and (got[4] > 0).all()


@pytest.mark.parametrize('name,b', [('n37_r5', 16), ('n20_r300', 8)])
def test_an_allowed_mask_and_a_movable_subset_equal_the_host_loop(name, b):
    env, c, _ = _build(name, b)
    allowed = ru.allowed_mask(c.n, c.r, 5, c.rb[0])
    movable = np.arange(c.n) % 4 != 2
    assert (~allowed.any(axis=1)).any() and allowed.any(axis=1).any()
    assert any(0 <= c.rb[0, i] < c.r and not allowed[i, c.rb[0, i]] and allowed[i].any() for i in range(c.n))
    got = _check_exact(env, allowed, movable, ru.FLOORS)
    never = ~allowed.any(axis=1) | ~movable
    assert np.array_equal(got[0][:, never], c.rb[:b][:, never]) and (got[4] > 0).any()
    moved = got[0] != c.rb[:b]
    assert allowed[np.nonzero(moved)[1], got[0][moved]].all()            # a link that moved sits on an allowed RB
    _check_exact(env, torch.as_tensor(allowed, device=env.device), torch.as_tensor(movable, device=env.device))


# ------------------------------------------------------------------------------------------ 2: planes, monotone, certificate
@pytest.mark.parametrize('name', ['n37_r5', 'n50_r6_no_rb', 'n20_r300'])
def test_the_planes_are_evaluates_and_the_total_never_falls(name):
    case, b, every = ru.CASES[name]
    env, c, _ = _build(case, b)
    rb, sinr, cap, rounds, moves, conv = _host(env.rb_ascent(floor_sinr_db=ru.FLOORS))
    res = env.evaluate(torch.as_tensor(rb[:, None, :], device=env.device), env._t['pwr'][:, None, :].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(res['sinr_db'].cpu().numpy()[:, 0].view(np.uint32), sinr.view(np.uint32))
    assert np.array_equal(res['capacity_mbps'].cpu().numpy()[:, 0].view(np.uint32), cap.view(np.uint32))
    start, end = _total(env, env._t['rb']), _total(env, rb)
    assert (end >= start).all() and (end[moves > 0] > start[moves > 0]).all() and (moves > 0).any()


def _sixteen(b=16):
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
    env = VecD2DEnv({'num_rbs': 6, 'num_cues': 6, 'num_due_pairs': 10, 'obs_fn': SignalPlanesObsFunction}, num_envs=b, cue_actions='traffic')
    env.reset(seed=7)
    gen = torch.Generator(device=env.device).manual_seed(7)
    env.step(torch.randint(0, 6 * env.num_pwr_actions['due'], (b, 10), generator=gen, device=env.device, dtype=torch.int32))
    return env


def test_the_ascent_never_beats_the_exact_optimum_of_share_rbs():
    env = _sixteen()
    try:
        best = _total(env, env.share_rbs().rb.clone())
        res = env.rb_ascent()
        got = _total(env, res.rb.clone())
        print('ascent / optimum per env:', np.round(got / best, 4).tolist())
        assert (got <= best + 1e-9).all() and (_host(res)[4] > 0).all()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 3: the float64 reference
@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False)])
def test_no_admissible_rb_gains_more_than_the_bar_allows_in_float64(name, floors):
    """The figures of the build this was written on (the largest left side less min_gain, over the allowed slack; <= 1 passes):
    -0.54, -1.54 and -0.24, with none of the 2368, 1281 and 2000 checks left out."""
    case, b, every = ru.CASES[name]
    env, c, _ = _build(case, b)
    floor = ru.FLOORS if floors else None
    rb, sinr, cap, rounds, moves, conv = _host(env.rb_ascent(floor_sinr_db=floor))
    assert conv.any()
    chk = ru.reference_check(c, np.arange(b), rb, conv.astype(bool), None, None, floor, 0.0)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e} of the allowed slack')
    assert chk.checks > 1000 and chk.left_out <= ru.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 1.0


# ------------------------------------------------------------------------------------------ 4: the interface
def test_env_mask_out_and_two_calls():
    from guard_util import Guarded, bits
    from gym_d2d_amd import _native
    env, c, _ = _build('n37_r5', 16)
    b, n = 16, c.n
    want = _host(env.rb_ascent(None, None, ru.FLOORS))
    own = env.rb_ascent(None, None, ru.FLOORS)
    assert all(x is y for x, y in zip(own, env.rb_ascent(None, None, ru.FLOORS)))      # the env's one tuple, reused
    assert own.rb is own[0] and own.capacity_mbps is own[2] and own.converged is own[5]
    _same(_host(own), want)                                                         # two calls, the same words
    shapes = ((b, n),) * 3 + ((b,),) * 3
    dtypes = (torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8)
    guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
    out = tuple(g.array for g in guarded)
    got = env.rb_ascent(None, None, ru.FLOORS, out=out)
    assert all(x is y for x, y in zip(got, out))
    _same(_host(got), want)
    assert all(g.intact() for g in guarded)
    mask = np.arange(b) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
        before = [bits(g.array).copy() for g in guarded]
        got = _host(env.rb_ascent(None, None, ru.FLOORS, out=tuple(g.array for g in guarded), env_mask=m))
        for x, y, was in zip(got, want, before):
            assert np.array_equal(x[mask].view(np.uint8), y[mask].view(np.uint8))
            assert np.array_equal(x[~mask].view(np.uint8).ravel(), was.reshape(b, -1)[~mask].ravel())     # masked rows untouched
        assert all(g.intact() for g in guarded)
    launches = _native.rbascent_launches
    o = [torch.empty(s, dtype=dt, device=env.device) for s, dt in zip(shapes, dtypes)]
    shared = torch.empty(b, dtype=torch.int32, device=env.device)
    for bad in (o[:5], (*o[:3], shared, shared, o[5]), (*o[:5], torch.empty(b, dtype=torch.int32, device=env.device)),
                (o[0], torch.empty((b, n + 1), device=env.device), *o[2:]), o[0],
                (o[0], torch.empty((b, 2 * n), device=env.device)[:, ::2], *o[2:]), (o[0].cpu(), *o[1:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, sinr_db, capacity_mbps, rounds, moves, converged\)'):
            env.rb_ascent(out=bad)
    with pytest.raises(ValueError, match='env_mask must be'):
        env.rb_ascent(env_mask=np.ones(b + 1, bool))
    with pytest.raises(ValueError, match='allowed must be'):
        env.rb_ascent(np.ones((n, c.r + 1), bool))
    with pytest.raises(ValueError, match='movable must be'):
        env.rb_ascent(movable=np.ones(n + 1, bool))
    with pytest.raises(ValueError, match='floor_sinr_db'):
        env.rb_ascent(floor_sinr_db={'cue': 1.0})
    with pytest.raises(ValueError, match='min_gain_mbps'):
        env.rb_ascent(min_gain_mbps=-1.0)
    with pytest.raises(ValueError, match='max_rounds'):
        env.rb_ascent(max_rounds=0)
    assert _native.rbascent_launches == launches                        # refused before any launch


# ------------------------------------------------------------------------------------------ 5: through step()
@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_actions_fed_to_step_export_the_solved_rbs(cue_actions):
    env, c, raw = _build('n37_r5', 16, cue_actions=cue_actions)
    held_rb, held_pwr = env._t['rb'].cpu().numpy().copy(), env._t['pwr'].cpu().numpy().copy()
    rb, sinr, cap, _, moves, _ = _host(env.rb_ascent(None, None, ru.FLOORS))
    actions = env.rb_ascent_actions(None, None, ru.FLOORS)
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (16, env.num_agents)
    _, _, _, info = env.step(actions)
    got = info['rb'].cpu().numpy(), info['tx_pwr_dbm'].cpu().numpy(), info['sinr_db'].cpu().numpy(), info['capacity_mbps'].cpu().numpy()
    env.step(raw)                                                       # the case's own actions back
    first = c.n - env.num_agents
    assert np.array_equal(got[0][:, first:], rb[:, first:]) and np.array_equal(got[0], rb) and np.array_equal(got[1], held_pwr)
    assert np.array_equal(got[2].view(np.uint32), sinr.view(np.uint32)) and np.array_equal(got[3].view(np.uint32), cap.view(np.uint32))
    assert (moves > 0).all()
    if cue_actions == 'traffic':
        assert first == c.cues and np.array_equal(rb[:, :first], held_rb[:, :first])        # the CUE links never move
        with_all = _host(env.rb_ascent(None, np.ones(c.n, bool), ru.FLOORS))
        assert np.array_equal(with_all[0], rb)


# ------------------------------------------------------------------------------------------ 6: refusals
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
    before = _native.rbascent_launches

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            with pytest.raises(ValueError, match=text):
                env.rb_ascent()
            with pytest.raises(ValueError, match=text):
                env.rb_ascent_actions()
            assert env._rbascent is None
            with pytest.raises(ValueError, match=text.replace('rb_ascent', 'power_ascent')):       # refused where power_ascent() is
                env.power_ascent()
        finally:
            env.close()
    refused(r'rb_ascent\(\).*export_actions', export_actions=False)
    refused(r'rb_ascent\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"rb_ascent\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"rb_ascent\(\).*'array'", {'path_loss_model': Arr})
    refused(r"rb_ascent\(\).*'per_step'", {'path_loss_model': PerStep})
    refused(r"rb_ascent\(\).*'channel'", {'path_loss_model': SpatialChannelPathLoss})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'rb_ascent\(\).*float32 cannot hold', {'device_config_file': pinned})
    refused(r'rb_ascent\(\) needs the torch path', use_torch=False)
    assert _native.rbascent_launches == before


def test_a_shape_past_160_kib_is_refused_in_bytes():
    from gym_d2d_amd import _native, rb_ascent
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
    need = rb_ascent.lds_bytes(2048, 256, False)
    assert need > _native.RBASCENT_MAX_LDS_BYTES
    env = VecD2DEnv({'num_rbs': 256, 'num_cues': 512, 'num_due_pairs': 1536, 'obs_fn': SignalPlanesObsFunction}, num_envs=1)
    try:
        env.reset(seed=1)
        before = _native.rbascent_launches
        with pytest.raises(ValueError, match=rf'rb_ascent\(\).*2048 links on 256 RBs need {need} bytes, more than 163840'):
            env.rb_ascent()
        assert _native.rbascent_launches == before
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 7: the example
def test_example_runs_and_the_ascent_gains_on_random_actions():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'rb_ascent.py'), run_name='__main__')['results']
    assert res['random_mbps'].shape == (64,)
    assert (res['rb_ascent_mbps'] >= res['random_mbps']).all() and (res['rb_ascent_mbps'] > res['random_mbps']).any()
    assert (res['alternating_mbps'] >= res['rb_ascent_mbps']).all()
    # share_rbs() applies: 10 movable DUE links, the optimum over their RBs at the powers each plane was scored at
    assert (res['rb_ascent_mbps'] <= res['share_rbs_mbps'] * (1 + 1e-6)).all()
    assert (res['alternating_mbps'] <= res['share_rbs_alternating_mbps'] * (1 + 1e-6)).all()
    assert res['best_response_dynamics_mbps'].shape == (64,)

"""Max-min SINR balancing on the GPU (VecD2DEnv.balance_sinr, balance_sinr_actions, csrc/d2d_balance.hip).

Two yardsticks.  Exact, no tolerance: the search of include/d2d_balance.h run on the host with the existing power_control() launch
as its probe and the pass rule evaluated on that kernel's outputs must give the level, probes, margin and powers, and the bits of
sinr_db, of ONE balance_sinr() launch.  Within the project's bar: the float64 reference (balance_util.balance_ref), compared on the
envs it does not call ambiguous (test_balance_cpu.py holds their share under 25 % on the reference alone)."""
from types import SimpleNamespace

import numpy as np
import pytest

import balance_util as bu
import power_control_util as pcu
from golden_util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BAR = bu.BAR
_cache = {}


def _state(case):
    if case == pcu.MIXED[0]:
        cues, dues, r = pcu.MIXED[1]
        pos, raw, rb, pwr = pcu.state(cues, dues, r, 77)
        p_min, p_max, levels = pcu.bounds(cues, dues)
        return SimpleNamespace(name=case, cues=cues, dues=dues, n=cues + dues, r=r, law='mixed', cell=500.0, b=pcu.B, pos=pos, raw=raw,
                               rb=rb, pwr=pwr, p_min=p_min, p_max=p_max, levels=levels)
    return pcu.make_case(case)


def _build(case, cue_actions='agent'):
    """The env of a power_control_util case, stepped once on the case's layout with the case's actions; built once."""
    key = (case, cue_actions)
    if key not in _cache:
        from gym_d2d_amd.envs import VecD2DEnv
        c = _state(case)
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


def _vec(c, v):
    return pcu.target_vector(v, c.cues, c.dues).astype(np.float32)


# every case of yardstick 1: name -> (power_control_util case, base, margins, floor, 'due' or None); the rows of balance_util first
_CD = lambda cue, due: {'cue': cue, 'due': due}
_rng = np.random.default_rng(41)
EXTRA = {
    'mixed_law': (pcu.MIXED[0], _CD(-10.0, 0.0), bu.grid(-30, 30, 1), None, None),
    # more than 64 KiB of LDS; the base is the case's own target vector (most links at one their lowest power meets, see
    # power_control_util.CASES), the grid from far below it to a few dB above
    'n1000_r64_ld35': ('n1000_r64_ld35', 'target', bu.grid(-40, 8, 4), None, None),          # 13 levels
    'n2048_r256': ('n2048_r256', 'target', bu.grid(-8, 8, 2), None, None),              # 9 levels
    'k1': ('n37_r5', _CD(-10.0, 0.0), np.array([-10.0], dtype=np.float32), None, None),
    'k1_infeasible': ('n37_r5', _CD(-10.0, 0.0), np.array([35.0], dtype=np.float32), None, None),
    'k4096_n1': ('n1', 0.0, bu.grid(0, 4095 / 32, 1 / 32), None, None),                 # 13 probes
    'non_uniform': ('n37_r5', _CD(-10.0, 0.0), (np.cumsum(_rng.uniform(0.05, 3.0, 40)) - 30.0).astype(np.float32), _CD(-12.0, bu.NEG), None),
}
EXACT = list(bu.TABLE) + list(bu.EXACT_ONLY) + list(EXTRA)


def _row(name):
    if name not in EXTRA:
        return bu.row(name)
    case, base, margins, floor, adj = EXTRA[name]
    c = _state(case)
    base = _vec(c, c.target) if isinstance(base, str) else _vec(c, base)
    return c, base, margins, None if floor is None else _vec(c, floor), None if adj is None else np.arange(c.n) >= c.cues


def _host_bisection(env, c, base, margins, floor, adjustable, max_iters=64):
    """The search of include/d2d_balance.h on the host: probe k of an env is env.power_control(base + margins[k]) - the parent
    commit's kernel, launched for the envs that ask for level k - and the pass rule is evaluated on that kernel's outputs in float32.
    Returns host arrays (power_dbm, sinr_db, margin_db, level, probes) and the number of power_control launches."""
    b, n, k_all = c.b, c.n, len(margins)
    first = n - env.num_agents
    adj = np.arange(n) >= first
    if adjustable is not None:
        adj &= adjustable
    fl = np.full(n, -np.inf, dtype=np.float32) if floor is None else floor
    p_max = c.p_max.astype(np.int32)
    out = tuple(torch.empty(s, dtype=dt, device=env.device) for s, dt in (((b, n), torch.int32), ((b, n), torch.float32),
                                                                         ((b,), torch.int32), ((b,), torch.uint8)))
    rb = env._t['rb'].cpu().numpy()
    on_rb = (rb >= 0) & (rb < c.r)
    lo, hi = np.full(b, -1), np.full(b, k_all)
    probes = np.zeros(b, dtype=np.int32)
    power, sinr = np.zeros((b, n), dtype=np.int32), np.zeros((b, n), dtype=np.float32)
    mid, live, launches, it = np.zeros(b, dtype=np.int64), np.ones(b, dtype=bool), 0, 0
    while live.any():
        for k in np.unique(mid[live]):
            e = live & (mid == k)
            t = base + margins[k]                                       # float32 + float32: the kernel's one addition
            assert t.dtype == np.float32
            res = env.power_control(torch.as_tensor(t, device=env.device), adjustable, max_iters, out=out, env_mask=e)
            launches += 1
            p, s, _, conv = _host(res)
            with np.errstate(invalid='ignore'):
                short = adj[None, :] & on_rb & (p == p_max[None, :]) & (s < t[None, :])
                low = on_rb & (s < fl[None, :])
            ok = (conv == 1) & ~short.any(axis=1) & ~low.any(axis=1)
            keep = e & (ok | (it == 0))                                 # probe 0 is kept whatever it says
            power[keep], sinr[keep] = p[keep], s[keep]
            probes[e] += 1
            lo[e & ok] = k
            hi[e & ~ok] = k
        it += 1
        live = (hi - lo > 1) & (lo >= 0)
        mid = (lo + hi) // 2
    margin = np.where(lo >= 0, margins[np.maximum(lo, 0)], np.float32(-np.inf)).astype(np.float32)
    return (power, sinr, margin, lo.astype(np.int32), probes), launches


def _solve(env, c, base, margins, floor, adjustable, **kw):
    return env.balance_sinr(torch.as_tensor(base, device=env.device), margins, None if floor is None else torch.as_tensor(floor, device=env.device),
                            adjustable, **kw)


# ------------------------------------------------------------------------------------------ 1: exact, against the host bisection
@pytest.mark.parametrize('name', EXACT)
def test_one_launch_equals_the_host_bisection_over_power_control(name):
    from gym_d2d_amd import _native, balance
    c, base, margins, floor, adj = _row(name)
    env, _, _ = _build(c.name)
    want, launches = _host_bisection(env, c, base, margins, floor, adj)
    before = _native.balance_launches
    got = _host(_solve(env, c, base, margins, floor, adj))
    assert _native.balance_launches == before + 1
    power, sinr, margin, level, probes = got
    assert power.dtype == np.int32 and sinr.dtype == np.float32 and margin.dtype == np.float32 and level.dtype == probes.dtype == np.int32
    assert power.shape == sinr.shape == (c.b, c.n) and margin.shape == level.shape == probes.shape == (c.b,)
    k_all = len(margins)
    print(f'{name}: K = {k_all}, levels {level.min()}..{level.max()} ({int((level < 0).sum())} infeasible, {int((level == k_all - 1).sum())} at '
          f'K - 1), probes {probes.min()}..{probes.max()}; the host bisection took {launches} power_control launches; LDS '
          f'{balance.lds_bytes(c.n, c.r, env._balance.law)} bytes')
    assert np.array_equal(level, want[3]) and np.array_equal(probes, want[4])
    assert np.array_equal(_bits(margin), _bits(want[2]))
    assert np.array_equal(power, want[0])
    assert np.array_equal(_bits(sinr), _bits(want[1]))
    assert (level >= -1).all() and (level < k_all).all() and (probes >= 1).all() and (probes <= 1 + int(np.ceil(np.log2(k_all)))).all()
    assert (probes[level < 0] == 1).all() and np.isneginf(margin[level < 0]).all()
    assert np.array_equal(margin[level >= 0], margins[level[level >= 0]])
    if name in ('n1000_r64_ld35', 'n2048_r256'):
        assert balance.lds_bytes(c.n, c.r, env._balance.law) > 64 * 1024
    if name == 'k4096_n1':
        assert (probes == 13).all() and len(np.unique(level)) > 8
    if name == 'k1':
        assert (level == 0).all() and (probes == 1).all()
    if name == 'k1_infeasible':
        assert (level == -1).all()
    if name in ('n300_r7', 'n96_r1', 'mixed_law', 'non_uniform'):
        assert len(np.unique(level)) >= 3
    again = _host(_solve(env, c, base, margins, floor, adj))             # two calls, the same words
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------ 2: the float64 reference
@pytest.mark.parametrize('name', list(bu.TABLE))
def test_against_the_float64_reference(name):
    c, base, margins, floor, adj = bu.row(name)
    env, _, _ = _build(c.name)
    ref = bu.reference(name)
    power, sinr, margin, level, probes = _host(_solve(env, c, base, margins, floor, adj))
    ok = ~ref.ambiguous
    fin = ref.on_rb & ok[:, None]
    same = (level == ref.level) & (power == ref.power_dbm).all(axis=1)
    print(f'{name}: {ref.ambiguous.mean():.2%} of {c.b} envs ambiguous; level and power_dbm equal in {same.mean():.2%} of all envs; sinr_db '
          f'rel_err {rel_err(sinr[fin], ref.sinr_db[fin]):.3e}')
    assert ref.ambiguous.mean() <= bu.CAP and ok.sum() >= 3
    assert np.array_equal(level[ok], ref.level[ok]) and np.array_equal(probes[ok], ref.probes[ok])
    assert np.array_equal(power[ok], ref.power_dbm[ok])
    assert np.array_equal(margin[ok].astype(np.float64), ref.margin_db[ok])
    assert rel_err(sinr[fin], ref.sinr_db[fin]) <= BAR
    assert np.isnan(sinr[~ref.on_rb]).all()


# ------------------------------------------------------------------------------------------ 3: through step()
@pytest.mark.parametrize('name', ['n37_r5_floor', 'n50_r6_ld35_floor', 'n50_r6_no_rb'])
def test_balanced_powers_through_step_give_the_returned_plane_and_keep_the_floors(name):
    c, base, margins, floor, adj = bu.row(name)
    env, _, raw = _build(c.name)
    power, sinr, margin, level, probes = _host(_solve(env, c, base, margins, floor, adj))
    actions = env.balance_sinr_actions(torch.as_tensor(base, device=env.device), margins,
                                       None if floor is None else torch.as_tensor(floor, device=env.device), adj)
    assert actions.dtype == torch.int32 and tuple(actions.shape) == (c.b, env.num_agents)
    _, _, _, info = env.step(actions)
    pwr_h, s_h, rb_h = info['tx_pwr_dbm'].cpu().numpy(), info['sinr_db'].cpu().numpy(), info['rb'].cpu().numpy()
    env.step(raw)                                                       # the case's own actions back
    on = (rb_h >= 0) & (rb_h < c.r)
    assert np.array_equal(on, (c.rb >= 0) & (c.rb < c.r)) and np.array_equal(rb_h[on], c.rb[on]) and np.array_equal(pwr_h, power)
    assert np.array_equal(_bits(s_h[on]), _bits(sinr[on])) and np.isnan(sinr[~on]).all()
    ok = level >= 0
    assert ok.any()
    t = base[None, :] + margin[:, None]
    held = on & ~(np.ones(c.n, bool) if adj is None else adj)[None, :]
    assert np.array_equal(power[held], c.pwr[held]) and np.array_equal(power[~on], c.pwr[~on])
    adjusted = on & (np.ones(c.n, bool) if adj is None else adj)[None, :]
    capped = adjusted & (power == c.p_max[None, :])
    with np.errstate(invalid='ignore'):
        assert not (capped & (s_h < t))[ok].any()                       # the level passes: nobody at its maximum is short of it
        if floor is not None:
            assert (~ok).any()
            assert not (on & (s_h < floor[None, :]))[ok].any()          # no floor-protected link ends under its floor
    # what the balanced level means: every adjusted link sees it.  A link under its maximum stopped because ceilf((float)p + (t - s))
    # <= p, which float32 also grants when 0 < t - s < ulp(p) / 2 <= 1e-6 (p < 32): far inside the bar's 1e-5 max(|t|, 1)
    slack = BAR * np.maximum(np.abs(t), 1.0)
    assert (s_h[ok][adjusted[ok]] >= (t - slack)[ok][adjusted[ok]]).all()


# ------------------------------------------------------------------------------------------ 4: env_mask, out=
def test_env_mask_and_out_planes():
    from gym_d2d_amd import _native
    name = 'n37_r5_floor'
    c, base, margins, floor, adj = bu.row(name)
    env, _, _ = _build(c.name)
    b = c.b
    want = _host(_solve(env, c, base, margins, floor, adj))
    own = _solve(env, c, base, margins, floor, adj)
    assert all(x is y for x, y in zip(own, _solve(env, c, base, margins, floor, adj)))      # the env's one quintuple, reused
    assert own.power_dbm is own[0] and own.sinr_db is own[1] and own.margin_db is own[2] and own.level is own[3] and own.probes is own[4]

    def fresh():
        return (torch.full((b, c.n), -77, dtype=torch.int32, device=env.device), torch.full((b, c.n), 123.25, device=env.device),
                torch.full((b,), -3.5, device=env.device), torch.full((b,), -5, dtype=torch.int32, device=env.device),
                torch.full((b,), 99, dtype=torch.int32, device=env.device))
    out = fresh()
    got = _solve(env, c, base, margins, floor, adj, out=out)
    assert all(x is y for x, y in zip(got, out))
    for x, y in zip(_host(got), want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    mask = np.arange(b) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        out = fresh()
        got = _host(_solve(env, c, base, margins, floor, adj, out=out, env_mask=m))
        for x, y in zip(got, want):
            assert np.array_equal(x[mask].view(np.uint8), y[mask].view(np.uint8))
        assert (got[0][~mask] == -77).all() and (got[1][~mask] == 123.25).all() and (got[2][~mask] == -3.5).all()
        assert (got[3][~mask] == -5).all() and (got[4][~mask] == 99).all()
    # host-side arguments are the same call: dicts, numbers, lists
    host = _host(env.balance_sinr(0.0, margins.tolist(), {'cue': -5.0, 'due': -np.inf}, adj))
    for x, y in zip(host, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    before = _native.balance_launches
    o = fresh()
    for bad in (o[:4], (o[0], o[1], o[2], o[3], o[3]), (o[0], o[0].view(torch.float32), o[2], o[3], o[4]), o[0],
                (o[0], o[1], o[2], o[3], torch.empty(b, dtype=torch.uint8, device=env.device)),
                (o[0], torch.empty((b, c.n + 1), device=env.device), o[2], o[3], o[4]), (o[0].cpu(), o[1], o[2], o[3], o[4])):
        with pytest.raises(ValueError, match='out must be'):
            env.balance_sinr(0.0, out=bad)
    with pytest.raises(ValueError, match='env_mask must be'):
        env.balance_sinr(0.0, env_mask=np.ones(b + 1, bool))
    for bad in ({'cue': 1.0}, np.zeros(c.n + 1), float('nan')):
        with pytest.raises(ValueError, match='base_sinr_db'):
            env.balance_sinr(bad)
        with pytest.raises(ValueError, match='floor_sinr_db'):
            env.balance_sinr(0.0, floor_sinr_db=bad)
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [0.0, np.inf], np.arange(4097), torch.zeros(3, dtype=torch.float64, device=env.device), torch.zeros(3)):
        with pytest.raises(ValueError, match='margins_db'):
            env.balance_sinr(0.0, bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_iters'):
            env.balance_sinr(0.0, max_iters=bad)
    with pytest.raises(ValueError, match='adjustable must be'):
        env.balance_sinr(0.0, adjustable=np.ones(c.n + 1, bool))
    assert _native.balance_launches == before                          # refused before any launch


def test_the_default_grid_and_the_iteration_cap():
    """margins_db=None is -20, -19, ..., 40; a max_iters below what a probe needs fails that probe (it has not converged), exactly as
    the host bisection over power_control(max_iters=...) decides."""
    c, base, margins, floor, adj = bu.row('n37_r5')
    env, _, _ = _build(c.name)
    default = np.arange(-20, 41).astype(np.float32)
    got = _host(env.balance_sinr({'cue': -10.0, 'due': 0.0}))
    want, _ = _host_bisection(env, c, base, default, None, None)
    for x, y in zip(got, want):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    for cap in (1, 3):
        got = _host(_solve(env, c, base, default, None, None, max_iters=cap))
        want, _ = _host_bisection(env, c, base, default, None, None, max_iters=cap)
        for x, y in zip(got, want):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ------------------------------------------------------------------------------------------ 5: links on fixed actions
def test_cue_links_on_traffic_actions_never_move():
    c, base, margins, floor, adj = bu.row('n37_r5_floor')
    env, _, raw = _build(c.name, cue_actions='traffic')
    held_rb, held_pwr = env._t['rb'].cpu().numpy().copy(), env._t['pwr'].cpu().numpy().copy()
    for adjustable in (None, np.ones(c.n, bool)):
        res = _host(_solve(env, c, base, margins, floor, adjustable))
        assert np.array_equal(res[0][:, :c.cues], held_pwr[:, :c.cues])                   # held, whatever is asked
        want, _ = _host_bisection(env, c, base, margins, floor, adjustable)
        for x, y in zip(res, want):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert (res[3] >= 0).any() and (res[0][:, c.cues:] != held_pwr[:, c.cues:]).any()
    a = env.balance_sinr_actions(torch.as_tensor(base, device=env.device), margins, torch.as_tensor(floor, device=env.device))
    assert a.dtype == torch.int32 and tuple(a.shape) == (c.b, c.dues) == (c.b, env.num_agents)
    _, _, _, info = env.step(a)
    assert np.array_equal(info['rb'].cpu().numpy(), held_rb) and np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), res[0])
    assert np.array_equal(_bits(info['sinr_db'].cpu().numpy()), _bits(res[1]))
    env.step(raw)


# ------------------------------------------------------------------------------------------ 6: one direct launch inside an arena
def test_direct_launch_at_37_links_writes_nothing_outside_its_outputs():
    """d2d_balance_sinr on raw pointers: the five outputs carved out of one int32 arena with guard words before, between and behind
    them.  The results are the env's own call's, and every guard word is as it was."""
    from gym_d2d_amd import _native
    c, base, margins, floor, adj = bu.row('n37_r5_floor')
    env, _, _ = _build(c.name)
    want = _host(_solve(env, c, base, margins, floor, adj))
    k = env._balance
    b, n, guard, fill = c.b, c.n, 64, 0x5A5A5A5A
    sizes = (b * n, b * n, b, b, b)
    offs, at = [], guard
    for sz in sizes:
        offs.append(at)
        at += sz + guard
    arena = torch.full((at,), fill, dtype=torch.int32, device=env.device)
    ptr = [arena.data_ptr() + 4 * o for o in offs]
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=env.device)
    base_t, floor_t, margins_t, adj_t = dev(base, np.float32), dev(floor, np.float32), dev(margins, np.float32), dev(adj, np.uint8)
    t = env._t
    before = _native.balance_launches
    _native.balance_sinr(t['pos_x'].data_ptr(), t['pos_y'].data_ptr(), t['rb'].data_ptr(), t['pwr'].data_ptr(), *k.ptrs, k.law, k.pow_k,
                         b, k.d, n, c.r, base_t.data_ptr(), floor_t.data_ptr(), margins_t.data_ptr(), len(margins), k.p_min.data_ptr(),
                         k.p_max.data_ptr(), adj_t.data_ptr(), 64, 0, *ptr, torch.cuda.current_stream().cuda_stream)
    assert _native.balance_launches == before + 1
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    views = [host[o:o + sz] for o, sz in zip(offs, sizes)]
    got = (views[0].reshape(b, n), views[1].view(np.float32).reshape(b, n), views[2].view(np.float32), views[3], views[4])
    for x, y in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), y.view(np.uint8))
    inside = np.zeros(at, dtype=bool)
    for o, sz in zip(offs, sizes):
        inside[o:o + sz] = True
    assert (~inside).sum() == 6 * guard and (host[~inside] == fill).all()


# ------------------------------------------------------------------------------------------ 7: refusals, and envs that do not ask
def test_unsupported_envs_are_refused_by_name_and_envs_that_do_not_ask_launch_nothing():
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.path_loss import ArrayPathLoss, ShadowingPathLoss
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Arr(ArrayPathLoss):
        def compute(self, view):
            return 20 * view.xp.log10(view.distance()) + 40.0
    before = _native.balance_launches

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            for call in (env.balance_sinr, env.balance_sinr_actions):
                with pytest.raises(ValueError, match=text):
                    call(5.0)
                with pytest.raises(ValueError, match=text.replace('balance_sinr', 'power_control')):
                    env.power_control(5.0)                              # refused exactly where power_control() is
            assert env._balance is None
        finally:
            env.close()
    refused(r'balance_sinr\(\).*export_actions', export_actions=False)
    refused(r'balance_sinr\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"balance_sinr\(\).*'array'", {'path_loss_model': Arr})
    refused(r'balance_sinr\(\) needs the torch path', use_torch=False)
    env = VecD2DEnv(dict(small), num_envs=2)
    try:
        env.reset(seed=1)
        env.step(env.action_buffer().clone())
        assert env._balance is None and _native.balance_launches == before
        res = env.balance_sinr()
        assert env._balance is not None and _native.balance_launches == before + 1
        assert [tuple(t.shape) for t in res] == [(2, 6), (2, 6), (2,), (2,), (2,)]
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ the example
def test_example_runs_and_balancing_is_at_least_the_fixed_target_on_every_feasible_env():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'sinr_balancing.py'), run_name='__main__')['results']
    ok = res['feasible']
    assert ok.any() and np.array_equal(ok, res['level'] >= 0)
    assert (res['balanced_min_db'][ok] >= res['fixed_min_db'][ok]).all()
    assert (res['balanced_min_db'][ok] > res['fixed_min_db'][ok]).any() and res['balanced_floors_kept'][ok].all()
    assert (res['probes'][~ok] == 1).all() and (res['probes'][ok] > 1).all()

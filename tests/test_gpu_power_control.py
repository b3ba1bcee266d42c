"""Target-SINR power control on the GPU (VecD2DEnv.power_control, power_control_actions, csrc/d2d_powerctl.hip).

Two yardsticks.  Exact, no tolerance: the step kernel itself - the solved powers go through step() and the float32 update expression,
formed in torch on the step's own planes, must not ask any adjustable link for more; the returned sinr_db is the step's plane bit
for bit.  Within the project's bar: the float64 restatement on the oracle's step (power_control_util.solve), compared on the envs
it does not call ambiguous (test_power_control_cpu.py holds their share under 25 % on the oracle alone)."""
import json

import numpy as np
import pytest

import power_control_util as pcu
from golden_util import rel_err
from oracle import d2d_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

B, BAR = pcu.B, pcu.BAR
ALL = list(pcu.CASES) + [pcu.MIXED[0]]
_cache = {}


def _case(name):
    if name == pcu.MIXED[0]:
        from types import SimpleNamespace
        cues, dues, r = pcu.MIXED[1]
        pos, raw, rb, pwr = pcu.state(cues, dues, r, 77)
        p_min, p_max, levels = pcu.bounds(cues, dues)
        return SimpleNamespace(name=name, cues=cues, dues=dues, n=cues + dues, r=r, law='mixed', cell=500.0, b=B,
                               target={'cue': -4.0, 'due': 9.0}, pos=pos, raw=raw, rb=rb, pwr=pwr, p_min=p_min, p_max=p_max, levels=levels)
    return pcu.make_case(name)


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
    env, c, raw = _cache[key]
    return env, c, raw


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


def _target_t(c, env, target=None):
    return torch.as_tensor(pcu.target_vector(c.target if target is None else target, c.cues, c.dues).astype(np.float32), device=env.device)


def _step_check(env, c, raw, res, target, adjustable=None):
    """Check 1: the solved powers through step(); `res` are the host copies of the solve.  Puts the case's own actions back."""
    power, sinr, iters, conv = res
    actions = env.power_control_actions(target, adjustable)
    _, _, _, info = env.step(actions)
    pwr, s_step, rb = info['tx_pwr_dbm'], info['sinr_db'], info['rb']
    tgt = _target_t(c, env, target)
    lo, hi = (torch.as_tensor(a.astype(np.float32), device=env.device) for a in (c.p_min, c.p_max))
    need = torch.ceil(pwr.to(torch.float32) + (tgt - s_step))           # float32, the kernel's expression on the step's planes
    want = torch.minimum(hi, torch.maximum(lo, need))
    on = (rb >= 0) & (rb < c.r)
    adj = on.clone()
    first = c.n - env.num_agents
    adj[:, :first] = False
    if adjustable is not None:
        adj &= torch.as_tensor(adjustable, device=env.device)[None, :]
    assert bool(adj.any()) and bool(torch.isfinite(need[adj]).all())
    assert bool((want[adj] <= pwr[adj].to(torch.float32)).all())        # nobody asks for more: a fixed point of the step itself
    pwr_h, s_h, on_h = pwr.cpu().numpy(), s_step.cpu().numpy(), on.cpu().numpy()
    done = conv == 1
    assert np.array_equal(pwr_h[done], power[done])                     # the decoded plane is the solved plane
    assert np.array_equal(pwr_h[:, first:], power[:, first:])
    assert np.array_equal(_bits(sinr[on_h]), _bits(s_h[on_h])) and np.isnan(sinr[~on_h]).all()
    env.step(raw)
    return pwr_h, on_h


# ------------------------------------------------------------------------------------------ 1: the exact fixed point
@pytest.mark.parametrize('name', ALL)
def test_solved_powers_are_a_fixed_point_of_the_step_itself(name):
    from gym_d2d_amd import _native
    env, c, raw = _build(name)
    law = {'ld2': _native.POWERCTL_LAW_INV_SQUARE, 'mixed': _native.POWERCTL_LAW_POWER}.get(c.law, _native.POWERCTL_LAW_POW_K)
    before = _native.powerctl_launches
    res = _host(env.power_control(c.target))
    assert _native.powerctl_launches == before + 1 and env._powerctl.law == law
    power, sinr, iters, conv = res
    assert power.dtype == np.int32 and sinr.dtype == np.float32 and iters.dtype == np.int32 and conv.dtype == np.uint8
    assert power.shape == sinr.shape == (c.b, c.n) and iters.shape == conv.shape == (c.b,)
    assert (conv == 1).all() and (iters < 64).all()
    if name in pcu.LARGE:
        # more than 64 KiB of LDS (d2d_powerctl.hip: 68 / 76 bytes per link, 4 per RB), and the sweeps reach the upper half of the
        # links: test_power_control_cpu.py asserts that on the reference, here the kernel's own powers show it
        assert c.n * (68 if c.law == 'ld2' else 76) + 4 * c.r > 64 * 1024
        lo = min(1024, c.n // 2)
        assert (iters >= 3).all() and ((power > c.p_min[None]) & (power < c.p_max[None]))[:, lo:].any(axis=1).all()
    assert (power >= c.p_min[None]).all() and (power <= c.p_max[None]).all()
    pwr_h, on = _step_check(env, c, raw, res, c.target)
    assert np.array_equal(power[~on], c.pwr[~on])                       # on no RB: the power is kept
    if name.endswith('no_rb'):
        assert (~on).sum() == B
    again = _host(env.power_control(c.target))                          # 7: two calls, the same bits
    for a, b in zip(res, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    print(f'{name}: sweeps {iters.min()}..{iters.max()}, at p_max {(power == c.p_max[None]).mean():.0%}, at p_min '
          f'{(power == c.p_min[None]).mean():.0%}')


# ------------------------------------------------------------------------------------------ 2: the oracle
@pytest.mark.parametrize('name', list(pcu.CASES))
def test_against_the_oracle_restatement(name):
    env, c, _ = _build(name)
    o = pcu.oracle_side(name)
    power, sinr, iters, conv = _host(env.power_control(c.target))
    ok = ~o.ambiguous
    share = float(o.ambiguous.mean())
    fin = o.on_rb & ok[:, None]
    dev = np.abs(sinr.astype(np.float64) - o.sinr_db)[fin]
    same = (power == o.power_dbm).all(axis=1)
    print(f'{name}: {share:.2%} of {c.b} envs ambiguous; power_dbm equal in {same.mean():.2%} of all envs; sinr_db rel_err '
          f'{rel_err(sinr[fin], o.sinr_db[fin]):.3e}, largest deviation {dev.max():.3e} dB (W = {pcu.W:g}); sweeps {iters.min()}..{iters.max()}')
    assert share <= pcu.CAP and ok.sum() >= 3
    if name in pcu.LARGE:                                               # the reference raises links of the upper half after sweep 1
        later = (o.power_dbm != o.after_one) & (o.power_dbm > c.p_min[None]) & (o.power_dbm < c.p_max[None])
        assert o.iters.min() >= 3 and later[:, min(1024, c.n // 2):].any(axis=1).all()
    assert np.array_equal(power[ok], o.power_dbm[ok])
    assert np.array_equal(iters[ok], o.iters[ok]) and np.array_equal(conv[ok], o.converged[ok].astype(np.uint8))
    assert rel_err(sinr[fin], o.sinr_db[fin]) <= BAR
    assert np.isnan(sinr[~o.on_rb]).all()


# ------------------------------------------------------------------------------------------ 3: minimality, monotonicity
@pytest.mark.parametrize('name', ['n37_r5', 'n300_r7', pcu.MIXED[0]])
def test_bounds_monotonicity_and_the_two_trivial_ends(name):
    env, c, _ = _build(name)
    t0 = pcu.target_vector(c.target, c.cues, c.dues)
    base = _host(env.power_control(t0))
    up = _host(env.power_control(t0 + 3.0))
    assert (up[0] >= base[0]).all() and (up[0] > base[0]).any()         # raising every target never lowers a power
    low = _host(env.power_control(-200.0))
    assert np.array_equal(low[0], np.broadcast_to(c.p_min[None], (B, c.n))) and (low[2] == 0).all() and (low[3] == 1).all()
    high = _host(env.power_control(200.0))
    assert np.array_equal(high[0], np.broadcast_to(c.p_max[None], (B, c.n))) and (high[3] == 1).all() and (high[2] == 1).all()
    for res in (base, up, low, high):
        assert (res[0] >= c.p_min[None]).all() and (res[0] <= c.p_max[None]).all() and np.isfinite(res[1]).all()


# ------------------------------------------------------------------------------------------ 4: the iteration cap
def test_iteration_cap_on_the_one_rb_case():
    env, c, raw = _build(pcu.ONE_RB)
    o = pcu.oracle_side(pcu.ONE_RB)
    res = _host(env.power_control(c.target, max_iters=1))
    power, sinr, iters, conv = res
    ok = ~o.ambiguous
    more = o.iters >= 1                                                  # the oracle's first sweep changed something
    assert more.any() and (o.iters > 1).any()
    assert (conv[ok & more] == 0).all() and (iters[ok & more] == 1).all()
    assert (conv[ok & ~more] == 1).all() and (iters[ok & ~more] == 0).all()
    assert np.array_equal(power[ok], o.after_one[ok])
    # sinr_db is still a step at those powers
    a = env.power_control_actions(c.target, max_iters=1)
    _, _, _, info = env.step(a)
    assert np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), power)
    assert np.array_equal(_bits(info['sinr_db'].cpu().numpy()), _bits(sinr))
    env.step(raw)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_iters'):
            env.power_control(c.target, max_iters=bad)


# ------------------------------------------------------------------------------------------ 5: adjustable
def test_links_that_are_not_adjustable_keep_their_power():
    env, c, raw = _build('n37_r5')
    rng = np.random.default_rng(9)
    mask = rng.random(c.n) < 0.5
    for m in (mask, torch.as_tensor(mask), torch.as_tensor(mask, device=env.device)):
        res = _host(env.power_control(c.target, adjustable=m))
        assert np.array_equal(res[0][:, ~mask], c.pwr[:, ~mask])
    assert (res[0][:, mask] != c.pwr[:, mask]).any()
    _step_check(env, c, raw, res, c.target, mask)
    # against the oracle with the same mask (the envs it calls ambiguous aside)
    o = pcu.solve(c.pos, c.tx, c.rx, c.rb, c.pwr, c.cols, c.spec, c.r, pcu.target_vector(c.target, c.cues, c.dues), c.p_min, c.p_max,
                  adjustable=mask)
    ok = ~o.ambiguous
    assert o.ambiguous.mean() <= pcu.CAP and np.array_equal(res[0][ok], o.power_dbm[ok]) and np.array_equal(res[2][ok], o.iters[ok])
    none = _host(env.power_control(c.target, adjustable=np.zeros(c.n, bool)))
    assert np.array_equal(none[0], c.pwr) and (none[2] == 0).all() and (none[3] == 1).all()
    for bad in (np.ones(c.n + 1, bool), np.ones(c.n, np.int32)):
        with pytest.raises(ValueError, match='adjustable must be'):
            env.power_control(c.target, adjustable=bad)


def test_cue_links_on_traffic_actions_never_move():
    env, c, raw = _build('n37_r5', cue_actions='traffic')
    info_rb, info_pwr = env._t['rb'].cpu().numpy().copy(), env._t['pwr'].cpu().numpy().copy()
    for adjustable in (None, np.ones(c.n, bool)):
        res = _host(env.power_control(200.0, adjustable=adjustable))
        assert np.array_equal(res[0][:, :c.cues], info_pwr[:, :c.cues])                  # held, whatever the target
        assert np.array_equal(res[0][:, c.cues:], np.broadcast_to(c.p_max[None, c.cues:], (B, c.dues)))
    a = env.power_control_actions(c.target)
    assert a.dtype == torch.int32 and tuple(a.shape) == (B, c.dues) == (B, env.num_agents)
    res = _host(env.power_control(c.target))
    _, _, _, info = env.step(a)
    assert np.array_equal(info['rb'].cpu().numpy(), info_rb) and np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), res[0])
    assert np.array_equal(_bits(info['sinr_db'].cpu().numpy()), _bits(res[1]))
    env.step(raw)


# ------------------------------------------------------------------------------------------ 6: env_mask, out=
def test_env_mask_and_out_planes():
    from gym_d2d_amd import _native
    env, c, _ = _build('n37_r5')
    want = _host(env.power_control(c.target))
    own = env.power_control(c.target)
    assert all(a is b for a, b in zip(own, env.power_control(c.target)))  # the env's one quadruple, reused
    assert own.power_dbm is own[0] and own.sinr_db is own[1] and own.iters is own[2] and own.converged is own[3]

    def fresh():
        return (torch.full((B, c.n), -77, dtype=torch.int32, device=env.device), torch.full((B, c.n), 123.25, device=env.device),
                torch.full((B,), -5, dtype=torch.int32, device=env.device), torch.full((B,), 9, dtype=torch.uint8, device=env.device))
    out = fresh()
    got = env.power_control(c.target, out=out)
    assert all(a is b for a, b in zip(got, out))
    for a, b in zip(_host(got), want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    mask = np.arange(B) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        out = fresh()
        got = _host(env.power_control(c.target, out=out, env_mask=m))
        for a, b in zip(got, want):
            assert np.array_equal(a[mask].view(np.uint8), b[mask].view(np.uint8))
        assert (got[0][~mask] == -77).all() and (got[1][~mask] == 123.25).all() and (got[2][~mask] == -5).all() and (got[3][~mask] == 9).all()
    before = _native.powerctl_launches
    o = fresh()
    for bad in (o[:3], (o[0], o[1], o[2], o[2]), (o[0], o[0].view(torch.float32), o[2], o[3]), o[0],
                (o[0], o[1], o[2], torch.empty(B, dtype=torch.int32, device=env.device)),
                (o[0], torch.empty((B, c.n + 1), device=env.device), o[2], o[3]),
                (o[0].cpu(), o[1], o[2], o[3])):
        with pytest.raises(ValueError, match='out must be'):
            env.power_control(c.target, out=bad)
    with pytest.raises(ValueError, match='env_mask must be'):
        env.power_control(c.target, env_mask=np.ones(B + 1, bool))
    for bad in ({'cue': 1.0}, np.zeros(c.n + 1), float('nan')):
        with pytest.raises(ValueError, match='target_sinr_db'):
            env.power_control(bad)
    assert _native.powerctl_launches == before                          # refused before any launch


# ------------------------------------------------------------------------------------------ 8: composition
SMALL = {'num_rbs': 5, 'num_cues': 6, 'num_due_pairs': 20}
SMALL_TARGET = {'cue': -4.0, 'due': 9.0}


def _small_env(b=8, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    return VecD2DEnv(dict(SMALL), num_envs=b, **kw)


def _small_actions(env, rng):
    highs = env._initial_action_highs()
    return torch.as_tensor(np.stack([rng.integers(0, h, env.num_envs) for h in highs], axis=1).astype(np.int32), device=env.device)


@pytest.mark.parametrize('moving', [False, True])
def test_after_autoreset_and_mobility_steps_it_agrees_with_the_oracle(moving):
    from gym_d2d_amd.mobility import GaussMarkovMobility
    kw = {'mobility': GaussMarkovMobility(speed_std_mps=8.0, memory=0.7)} if moving else {}
    env = _small_env(autoreset=True, **kw)
    try:
        env.reset(seed=21, elapsed=np.arange(8) % 10)
        rng = np.random.default_rng(4)
        resets = 0
        for _ in range(12):
            _, _, _, info = env.step(_small_actions(env, rng))
            resets += int(info['reset'].sum())
        assert resets >= 8
        res = _host(env.power_control(SMALL_TARGET))
        lp = env.link_positions().cpu().numpy().astype(np.float64)     # [B, N, 4] as moved
        pos = np.stack([env._t['pos_x'].cpu().numpy(), env._t['pos_y'].cpu().numpy()], axis=-1).astype(np.float64)
        tx, rx = env.simulator.link_tx, env.simulator.link_rx
        assert np.array_equal(lp[:, :, :2], pos[:, tx]) and np.array_equal(lp[:, :, 2:], pos[:, rx])
        cues, dues = SMALL['num_cues'], SMALL['num_due_pairs']
        p_min, p_max, _ = pcu.bounds(cues, dues)
        o = pcu.solve(pos, tx, rx, env._t['rb'].cpu().numpy(), env._t['pwr'].cpu().numpy(), orc.device_columns(*orc.device_configs(cues, dues)[1:]),
                      pcu.models()['ld2'][1], SMALL['num_rbs'], pcu.target_vector(SMALL_TARGET, cues, dues), p_min, p_max)
        ok = ~o.ambiguous
        assert o.ambiguous.mean() <= pcu.CAP
        assert np.array_equal(res[0][ok], o.power_dbm[ok]) and np.array_equal(res[2][ok], o.iters[ok])
        assert np.array_equal(res[3][ok], o.converged[ok].astype(np.uint8)) and rel_err(res[1][ok], o.sinr_db[ok]) <= BAR
    finally:
        env.close()


def test_two_shards_equal_the_whole_batch():
    rng = np.random.default_rng(4)
    whole = _small_env()
    acts = [_small_actions(whole, rng) for _ in range(2)]

    def run(env, rows):
        out = []
        env.reset(seed=11)
        out.append(_host(env.power_control(SMALL_TARGET)))
        for a in acts:
            env.step(a[rows].contiguous())
            out.append(_host(env.power_control(SMALL_TARGET)))
        env.close()
        return out
    ref = run(whole, slice(0, 8))
    for k in range(2):
        rows = slice(k * 4, (k + 1) * 4)
        got = run(_small_env(b=4, first_env=k * 4), rows)
        for t, (a, b) in enumerate(zip(ref, got)):
            for x, y, what in zip(a, b, ('power_dbm', 'sinr_db', 'iters', 'converged')):
                assert np.array_equal(x[rows].view(np.uint8), y.view(np.uint8)), f'shard {k}, step {t}: {what}'


def test_composes_with_best_response_actions():
    env = _small_env()
    try:
        env.reset(seed=2)
        for _ in range(3):
            _, _, _, info = env.step(env.best_response_actions(min_gain_db=1.0))
            rb0 = info['rb'].clone()
            res = tuple(t.clone() for t in env.power_control(SMALL_TARGET))
            _, _, _, info = env.step(env.power_control_actions(SMALL_TARGET))
            assert torch.equal(info['rb'], rb0) and torch.equal(info['tx_pwr_dbm'], res[0])      # RBs stay, powers are the solve's
            assert torch.equal(info['sinr_db'].view(torch.int32), res[1].view(torch.int32))
        assert env.status_flags() == 0
    finally:
        env.close()


def test_envs_that_do_not_ask_launch_nothing():
    from gym_d2d_amd import _native
    before = _native.powerctl_launches
    env = _small_env()
    try:
        env.reset(seed=1)
        for _ in range(3):
            env.step(env.action_buffer().clone())
        assert env._powerctl is None and _native.powerctl_launches == before
        env.power_control(0.0)
        assert env._powerctl is not None and _native.powerctl_launches == before + 1
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 9: refusals
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
    before = _native.powerctl_launches

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            with pytest.raises(ValueError, match=text):
                env.power_control(5.0)
            with pytest.raises(ValueError, match=text):
                env.power_control_actions(5.0)
            assert env._powerctl is None
        finally:
            env.close()
    refused(r'power_control\(\).*export_actions', export_actions=False)
    refused(r'power_control\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"power_control\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"power_control\(\).*'array'", {'path_loss_model': Arr})
    refused(r"power_control\(\).*'per_step'", {'path_loss_model': PerStep})
    refused(r"power_control\(\).*'channel'", {'path_loss_model': SpatialChannelPathLoss})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'power_control\(\).*float32 cannot hold', {'device_config_file': pinned})
    env = VecD2DEnv(dict(small), num_envs=2, use_torch=False)
    try:
        with pytest.raises(ValueError, match=r'power_control\(\) needs the torch path'):
            env.power_control(5.0)
    finally:
        env.close()
    assert _native.powerctl_launches == before                          # at the call, not inside a launch


# ------------------------------------------------------------------------------------------ the example
def test_example_runs_and_power_control_meets_more_targets_with_less_power():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'power_control.py'), run_name='__main__')
    assert res['final_met'] > res['random_met'] and res['final_mw'] < res['random_mw']

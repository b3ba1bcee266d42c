"""Queue-aware goodput ascent on the GPU (VecD2DEnv.goodput_ascent, goodput_ascent_actions, csrc/d2d_goodput.hip).

Two yardsticks.  EXACT, no tolerance: all nine outputs of ONE goodput_ascent() launch equal goodput_ascent_util.goodput_by_evaluate,
the statement as a host loop with one evaluate() launch per link turn and the terms formed in NumPy int64 by queue_util.budget_bits.
REFERENCE: at the returned state of every converged env the float64 oracle finds no admissible candidate that gains more than
min_gain_bits plus the slack of goodput_ascent_util.reference_check (test_goodput_ascent_cpu.py holds the share of checks left out
under 25 % on the restatement's own fixed point)."""
import json

import numpy as np
import pytest

import goodput_ascent_util as gu
import power_control_util as pcu
from test_gpu_rb_ascent import _state

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

_cache = {}
NAMES = ('rb', 'power_dbm', 'sinr_db', 'capacity_mbps', 'served_bits', 'value', 'rounds', 'moves', 'converged')


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


def _same(got, want):
    for name, x, y in zip(NAMES, got, want):
        assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype)
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), name


def _check_exact(env, kind='mix', move=('rb', 'power'), allowed=None, movable=None, floor=None, min_gain=0, max_rounds=16, seed=0):
    """One launch against the host loop, word for word; returns the launch's host arrays."""
    from gym_d2d_amd import _native
    demand, weight, bpm = gu.pattern(kind, env.num_envs, env.num_links, seed)
    want, calls = gu.goodput_by_evaluate(env, demand, weight, bpm, move, allowed, movable, floor, min_gain, max_rounds)
    before = _native.goodput_launches
    got = _host(env.goodput_ascent(demand, weight, bpm, move, allowed, movable, floor, min_gain, max_rounds))
    assert _native.goodput_launches == before + 1
    print(f'{kind} {move}: rounds {got[6].tolist()}, moves {got[7].tolist()}, converged {got[8].tolist()}, value {got[5].tolist()}; '
          f'the host loop made {calls} evaluate() calls')
    _same(got, want)
    return got


# ------------------------------------------------------------------------------------------ 1: exact, against the host loop
@pytest.mark.parametrize('move', [('rb', 'power'), ('rb',), ('power',)])
def test_n37_r5_equals_the_host_loop_over_evaluate(move):
    env, c, _ = _build('n37_r5', 16)
    got = _check_exact(env, move=move)
    assert (got[7] > 0).all() and (got[8] == 1).any()
    if move == ('rb',):
        assert np.array_equal(got[1], c.pwr[:16]) and (got[0] != c.rb[:16]).any()
    if move == ('power',):
        assert np.array_equal(got[0], c.rb[:16]) and (got[1] != c.pwr[:16]).any()
    if len(move) == 2:
        assert (got[0] != c.rb[:16]).any() and (got[1] != c.pwr[:16]).any()


def test_n37_r5_floors_min_gain_and_the_round_cap_equal_the_host_loop():
    env, c, _ = _build('n37_r5', 16)
    free = _check_exact(env)
    fl = _check_exact(env, floor=gu.FLOORS)
    assert any(not np.array_equal(x, y) for x, y in zip(free[:2], fl[:2]))          # the floors change the outcome
    gated = _check_exact(env, min_gain=3000)
    assert any(not np.array_equal(x, y) for x, y in zip(free[:2], gated[:2])) and (gated[7] > 0).any()       # the bar changes the outcome
    _check_exact(env, floor=gu.FLOORS, min_gain=3000)
    for cap in (1, 2):
        got = _check_exact(env, max_rounds=cap)
        assert (got[8] == 0).any() and (got[6] <= cap).all() and (got[6][got[8] == 0] == cap).all()


CASE_KIND = {'n20_r64': 'uncapped', 'n20_r300': 'mix', 'n96_r2': 'mix', 'n96_r1': 'mix', 'n50_r6_hata': 'saturate', 'n50_r6_ld35': 'mix',
             'n50_r6_no_rb': 'mix', 'n300_r7': 'uncapped', 'n1000_r64_ld35': 'mix'}


@pytest.mark.parametrize('name', list(CASE_KIND))
def test_the_cases_equal_the_host_loop_over_evaluate(name):
    from gym_d2d_amd import goodput_ascent
    case, b, every = gu.CASES[name]
    env, c, _ = _build(case, b)
    mov = None if every == 1 else gu.movable_mask(c.n, every)
    allowed = gu.allowed_mask(c.n, c.r, 5, c.rb[0]) if name == 'n20_r300' else None
    got = _check_exact(env, CASE_KIND[name], movable=mov, allowed=allowed, seed=sum(map(ord, name)))
    rb, power, sinr, cap, served, value, rounds, moves, conv = got
    on = (c.rb[:b] >= 0) & (c.rb[:b] < c.r)
    still = ~on | ~(np.ones(c.n, bool) if mov is None else mov)[None, :]
    assert np.array_equal(rb[still], c.rb[:b][still]) and np.array_equal(power[still], c.pwr[:b][still])
    assert (moves > 0).all() or CASE_KIND[name] == 'saturate'           # where every budget is at the clip nothing gains
    if name == 'n20_r300':
        assert c.r > 256 and c.r % 32 != 0 and (~allowed.any(axis=1)).any()
        assert any(0 <= c.rb[0, i] < c.r and not allowed[i, c.rb[0, i]] and allowed[i].any() for i in range(c.n))
        moved = rb != c.rb[:b]
        assert allowed[np.nonzero(moved)[1], rb[moved]].all()            # a link that moved its RB sits on an allowed one
    if name == 'n96_r1':
        assert np.array_equal(rb, c.rb[:b])                             # only power candidates exist
        none = _check_exact(env, 'mix', move=('rb',), seed=sum(map(ord, name)))
        assert (none[7] == 0).all() and (none[8] == 1).all() and (none[6] == 0).all() and np.array_equal(none[0], c.rb[:b])
    if name == 'n96_r2':
        assert max(np.bincount(rb[e], minlength=2).max() for e in range(b)) >= 40
    if name == 'n50_r6_no_rb':
        assert (~on).any() and np.isfinite(sinr[~on]).all()             # evaluate()'s SNR for a link on no RB: it counts in value
        demand, weight, _ = gu.pattern('mix', b, c.n, sum(map(ord, name)))
        assert np.array_equal(value, (weight.astype(np.int64) * served).sum(axis=1))
    if name == 'n300_r7':
        assert c.n > 256
    if name == 'n1000_r64_ld35':
        assert goodput_ascent.lds_bytes(c.n, c.r) > 64 * 1024 and env._goodput.law != 0
    if name in ('n50_r6_hata', 'n50_r6_ld35'):
        assert env._goodput.law == 2
    if CASE_KIND[name] == 'saturate':
        assert (served == gu.UNCAPPED).any() and (served < gu.UNCAPPED).any() and (moves > 0).any()     # budgets at the clip, and under it


def test_the_general_power_law_equals_the_host_loop_over_evaluate():
    env, c, _ = _build(*gu.MIXED[:2])
    got = _check_exact(env)
    assert env._goodput.law == 1 and (got[7] > 0).all()


def test_64_due_levels_equal_the_host_loop():
    from test_gpu_ascent import _custom
    env = _custom({'num_rbs': 4, 'num_cues': 6, 'num_due_pairs': 14, 'due_max_tx_power_dBm': 63}, 8, 5)
    try:
        assert env.num_pwr_actions['due'] == 64
        got = _check_exact(env, 'uncapped')
        _check_exact(env, 'mix', move=('power',))
        assert (got[1][:, 6:] > 23).any() and (got[7] > 0).all()
    finally:
        env.close()


@pytest.mark.parametrize('kind,name', [('zero', 'n37_r5'), ('zero', 'n50_r6_ld35'), ('uncapped', 'n37_r5'), ('saturate', 'n37_r5'),
                                       ('mix', 'n50_r6_hata')])
def test_the_demand_and_weight_patterns_equal_the_host_loop(kind, name):
    case, b, every = gu.CASES[name]
    env, c, _ = _build(case, b)
    got = _check_exact(env, kind, floor=gu.FLOORS if kind == 'uncapped' else None, seed=7)
    if kind == 'zero':                                                  # no Delta is positive
        assert (got[7] == 0).all() and (got[5] == 0).all() and (got[8] == 1).all() and (got[4] == 0).all()
        assert np.array_equal(got[0], c.rb[:b]) and np.array_equal(got[1], c.pwr[:b])
    elif kind == 'saturate':                                            # budgets at the clip gain nothing; the others still do
        assert (got[4] == gu.UNCAPPED).any() and (got[4] < gu.UNCAPPED).any() and (got[7] > 0).any()
    else:
        assert (got[7] > 0).all()
    if kind == 'mix':                                                   # capped links end at low powers: ties go to the lowest
        demand, weight, _ = gu.pattern(kind, b, c.n, 7)
        assert (got[4] <= np.maximum(demand, 0)).all()


def test_scalars_and_rows_broadcast():
    env, c, _ = _build('n37_r5', 16)
    row = (np.arange(c.n) % 3 * 700).astype(np.int64)
    full = np.broadcast_to(row, (16, c.n)).astype(np.int32)             # Fortran order, as astype() leaves a broadcast: the host side copies it
    assert not full.flags.c_contiguous
    want, _ = gu.goodput_by_evaluate(env, full, 3, 1000.0)
    _same(_host(env.goodput_ascent(full, np.full((16, c.n), 3, np.int32), 1000.0)), want)
    for demand, weight in ((row, 3), (torch.as_tensor(row, device=env.device), torch.tensor(3, dtype=torch.int32)), (row.astype(np.int32), np.int64(3))):
        _same(_host(env.goodput_ascent(demand, weight, 1000.0)), want)
    assert (want[7] > 0).any()


# ------------------------------------------------------------------------------------------ 2: the float64 reference
@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False)])
def test_no_admissible_candidate_gains_more_than_the_slack_allows_in_float64(name, floors):
    """The figures of the build this was written on are in DESIGN.md 4.24 (the largest left side less min_gain, over the slack;
    <= 1 passes)."""
    c, b, mov, demand, weight, bpm = gu.case_inputs(name, 'mix')
    env, _, _ = _build(gu.CASES[name][0], b)
    floor = gu.FLOORS if floors else None
    got = _host(env.goodput_ascent(demand, weight, bpm, floor_sinr_db=floor))
    assert got[8].any()
    chk = gu.reference_check(c, np.arange(b), got[0], got[1], got[8].astype(bool), demand, weight, bpm, floor=floor)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e} of the slack')
    assert chk.checks > 1000 and chk.left_out <= gu.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 1.0


# ------------------------------------------------------------------------------------------ 3: the interface
def test_env_mask_out_and_two_calls():
    from guard_util import Guarded, bits
    from gym_d2d_amd import _native
    env, c, _ = _build('n37_r5', 16)
    b, n = 16, c.n
    demand, weight, bpm = gu.pattern('mix', b, n)
    args = (demand, weight, bpm, ('rb', 'power'), None, None, gu.FLOORS)
    want = _host(env.goodput_ascent(*args))
    own = env.goodput_ascent(*args)
    assert all(x is y for x, y in zip(own, env.goodput_ascent(*args)))              # the env's one tuple, reused
    assert own.rb is own[0] and own.served_bits is own[4] and own.value is own[5] and own.converged is own[8]
    _same(_host(own), want)                                                         # two calls, the same words
    shapes = ((b, n),) * 5 + ((b,),) * 4
    dtypes = (torch.int32, torch.int32, torch.float32, torch.float32, torch.int32, torch.int64, torch.int32, torch.int32, torch.uint8)
    guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
    out = tuple(g.array for g in guarded)
    got = env.goodput_ascent(*args, out=out)
    assert all(x is y for x, y in zip(got, out))
    _same(_host(got), want)
    assert all(g.intact() for g in guarded)
    mask = np.arange(b) % 3 != 1
    for m in (mask, torch.as_tensor(mask, device=env.device), torch.as_tensor(mask.astype(np.uint8))):
        guarded = [Guarded(s, dt) for s, dt in zip(shapes, dtypes)]
        before = [bits(g.array).copy() for g in guarded]
        got = _host(env.goodput_ascent(*args, out=tuple(g.array for g in guarded), env_mask=m))
        for x, y, was in zip(got, want, before):
            assert np.array_equal(x[mask].view(np.uint8), y[mask].view(np.uint8))
            assert np.array_equal(x[~mask].view(np.uint8).ravel(), was.reshape(b, -1)[~mask].ravel())     # masked rows untouched
        assert all(g.intact() for g in guarded)
    launches = _native.goodput_launches
    o = [torch.empty(s, dtype=dt, device=env.device) for s, dt in zip(shapes, dtypes)]
    for bad in (o[:8], (*o[:6], o[7], o[7], o[8]), (*o[:5], torch.empty(b, dtype=torch.int32, device=env.device), *o[6:]), o[0],
                (o[0], torch.empty((b, n + 1), dtype=torch.int32, device=env.device), *o[2:]), (o[0].cpu(), *o[1:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves, converged\)'):
            env.goodput_ascent(demand, weight, bpm, out=bad)
    for kw, text in ((dict(env_mask=np.ones(b + 1, bool)), 'env_mask must be'), (dict(allowed=np.ones((n, c.r + 1), bool)), 'allowed must be'),
                     (dict(movable=np.ones(n + 1, bool)), 'movable must be'), (dict(floor_sinr_db={'cue': 1.0}), 'floor_sinr_db'),
                     (dict(min_gain_bits=-1), 'min_gain_bits'), (dict(min_gain_bits=0.5), 'min_gain_bits'), (dict(max_rounds=0), 'max_rounds'),
                     (dict(move=()), 'move must name'), (dict(move=('rb', 'both')), 'move must name'),
                     (dict(weight=np.full(n, (1 << 20) + 1)), r'weight must lie in \[0, 1048576\]'), (dict(weight=-1), 'weight must lie'),
                     (dict(weight=np.ones(n)), 'weight must be None or ints'), (dict(demand_bits=np.ones((b, n + 1), np.int32)), 'demand_bits must be')):
        with pytest.raises(ValueError, match=text):
            env.goodput_ascent(**{**dict(demand_bits=demand, weight=weight, bits_per_mbps=bpm), **kw})
    for call in (lambda: env.goodput_ascent(), lambda: env.goodput_ascent(demand), lambda: env.goodput_ascent(bits_per_mbps=bpm),
                 lambda: env.goodput_ascent_actions()):
        with pytest.raises(ValueError, match=r'goodput_ascent\(\) on an env without traffic= needs demand_bits and bits_per_mbps'):
            call()
    for bad in (0.0, -1.0, float('nan'), float('inf'), '1', True):
        with pytest.raises(ValueError, match='bits_per_mbps must be a finite number > 0'):
            env.goodput_ascent(demand, weight, bad)
    assert _native.goodput_launches == launches                         # refused before any launch


# ------------------------------------------------------------------------------------------ 4: through a traffic env and step()
@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_a_traffic_env_defaults_to_its_backlog_and_step_exports_the_solved_planes(cue_actions):
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
    from gym_d2d_amd.queues import PacketTraffic
    b, cues, dues, r = 16, 6, 10, 6
    model = PacketTraffic(packets_per_step=(0.5, 2.5), packet_bits=1000, deadline_steps=4, buffer_bits=8000, dt_s=1e-3)
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'obs_fn': SignalPlanesObsFunction}, num_envs=b,
                    cue_actions=cue_actions, traffic=model)
    try:
        env.reset(seed=11)
        gen = torch.Generator(device=env.device).manual_seed(11)
        highs = torch.as_tensor(np.asarray(env._initial_action_highs(), dtype=np.int64), device=env.device)
        for _ in range(3):
            env.step((torch.rand((b, env.num_agents), generator=gen, device=env.device) * highs).to(torch.int32))
        backlog = env.queues().backlog_bits.clone()
        assert (backlog > 0).any() and (backlog == 0).any()
        explicit = _host(env.goodput_ascent(backlog, None, model.bits_per_mbps_step))
        _same(_host(env.goodput_ascent()), explicit)                    # demand: the live backlog plane; the step length: the model's
        want, _ = gu.goodput_by_evaluate(env, backlog, None, model.bits_per_mbps_step)
        _same(explicit, want)
        assert (explicit[7] > 0).any() and (explicit[4] <= backlog.cpu().numpy()).all()
        held_rb = env._t['rb'].cpu().numpy().copy()
        actions = env.goodput_ascent_actions()
        assert actions.dtype == torch.int32 and tuple(actions.shape) == (b, env.num_agents)
        _, _, _, info = env.step(actions)
        torch.cuda.synchronize()
        assert np.array_equal(info['rb'].cpu().numpy(), explicit[0]) and np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), explicit[1])
        assert np.array_equal(info['capacity_mbps'].cpu().numpy().view(np.uint32), explicit[3].view(np.uint32))
        assert np.array_equal(info['sinr_db'].cpu().numpy().view(np.uint32), explicit[2].view(np.uint32))
        if cue_actions == 'traffic':
            assert np.array_equal(explicit[0][:, :cues], held_rb[:, :cues])         # the CUE links never move
        # the max-weight recipe: weight = backlog >> k, demand uncapped
        w = (backlog >> 3).clamp(0, 1 << 20)
        got = _host(env.goodput_ascent(gu.UNCAPPED, w, None))
        want, _ = gu.goodput_by_evaluate(env, gu.UNCAPPED, w, model.bits_per_mbps_step)
        _same(got, want)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 5: refusals
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
    before = _native.goodput_launches

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            with pytest.raises(ValueError, match=text):
                env.goodput_ascent(100, None, 1000.0)
            with pytest.raises(ValueError, match=text):
                env.goodput_ascent_actions(100, None, 1000.0)
            assert env._goodput is None
            with pytest.raises(ValueError, match=text.replace('goodput_ascent', 'rb_ascent')):        # refused where rb_ascent() is
                env.rb_ascent()
        finally:
            env.close()
    refused(r'goodput_ascent\(\).*export_actions', export_actions=False)
    refused(r'goodput_ascent\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"goodput_ascent\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"goodput_ascent\(\).*'array'", {'path_loss_model': Arr})
    refused(r"goodput_ascent\(\).*'per_step'", {'path_loss_model': PerStep})
    refused(r"goodput_ascent\(\).*'channel'", {'path_loss_model': SpatialChannelPathLoss})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'goodput_ascent\(\).*float32 cannot hold', {'device_config_file': pinned})
    refused(r'goodput_ascent\(\) needs the torch path', use_torch=False)
    assert _native.goodput_launches == before


def test_a_shape_past_160_kib_and_a_class_of_65_levels_are_refused():
    from gym_d2d_amd import _native, goodput_ascent
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
    need = goodput_ascent.lds_bytes(2048, 256)
    assert need > _native.GOODPUT_MAX_LDS_BYTES
    before = _native.goodput_launches
    env = VecD2DEnv({'num_rbs': 256, 'num_cues': 512, 'num_due_pairs': 1536, 'obs_fn': SignalPlanesObsFunction}, num_envs=1)
    try:
        env.reset(seed=1)
        with pytest.raises(ValueError, match=rf'goodput_ascent\(\).*2048 links on 256 RBs need {need} bytes, more than 163840'):
            env.goodput_ascent(100, None, 1000.0)
    finally:
        env.close()
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3, 'due_max_tx_power_dBm': 64}, num_envs=2)
    try:
        env.reset(seed=1)
        assert env.num_pwr_actions['due'] == 65
        with pytest.raises(ValueError, match=r'goodput_ascent\(\).*at most 64 levels \(D2D_GOODPUT_MAX_LEVELS\), got 65'):
            env.goodput_ascent(100, None, 1000.0)
    finally:
        env.close()
    assert _native.goodput_launches == before


# ------------------------------------------------------------------------------------------ 6: the example
def test_example_runs_and_reports_the_four_policies():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'goodput_ascent.py'), run_name='__main__')['results']
    for policy in ('random', 'capacity_ascent', 'goodput_ascent', 'max_weight'):
        assert res[policy]['delivered_mbps'].shape == (64,) and res[policy]['expired_bits'].shape == (64,)
        assert np.isfinite(res[policy]['delivered_mbps']).all() and (res[policy]['delivered_mbps'] > 0).all()
    # the queue-aware search delivers more than random actions do
    assert res['goodput_ascent']['delivered_mbps'].mean() > res['random']['delivered_mbps'].mean()

"""What-if evaluation on a path-loss table on the GPU (VecD2DEnv.evaluate_table / evaluate_table_actions, csrc/d2d_evaltab.hip).

1. Direct launches on drawn tables (table_evaluate_util.CASES) with every output between guard bands, against
   evaluate_util.evaluate_ref on 'pl' at the project's bar 1e-5 (|d| <= 1e-5 max(|ref|, 1)) on sinr_db (dB) and capacity_mbps (Mbps);
   links whose reference sinr_db lies within 1e-4 dB of their sensitivity are left out of the capacity comparison, at most 1 % of a
   case (asserted on the reference alone in test_table_evaluate_cpu.py).  The total against the documented order restated on the host,
   planes=() and a second launch, all bit for bit.
2. The domain flag: raised for exactly the candidates that read a NaN / -inf entry; +inf is a gain of 0.
3. Bit for bit against the step on the 'channel', 'per_step' and 'array' routes.  4. The env is untouched.  5. table= on a native env.

Every test prints what it measured.  Measured on an MI355X: sinr_db rel_err 7.2e-8 - 1.2e-6, capacity_mbps 1.3e-7 - 2.4e-7 over the
eight direct cases; on the native env evaluate_table() 6.0e-7 / 8.9e-7 (ple 2 / 3.5) where evaluate() has 6.0e-7 / 1.9e-6."""
import runpy
from pathlib import Path

import numpy as np
import pytest

import evaluate_util as evu
import table_evaluate_util as teu
from guard_util import Guarded, bits
from oracle import d2d_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parent.parent


def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_inputs = {}


def _device_inputs(c):
    """The candidate-independent device tensors of a case, uploaded once per case."""
    key = id(c['table'])
    if key not in _inputs:
        _inputs[key] = [torch.as_tensor(np.ascontiguousarray(c[name]), device='cuda') for name in ('tx', 'rx', 'cols', 'cap_cols')]
    return _inputs[key]


def _launch(c, rb=None, pwr=None, table=None, sinr=True, cap=True):
    """One d2d_evaluate_table launch with every output between guard bands.  Returns (sinr_db, capacity_mbps, total_mbps, domain) as
    host arrays, None for a plane not asked for."""
    from gym_d2d_amd import _native
    rb, pwr = c['rb'] if rb is None else rb, c['pwr'] if pwr is None else pwr
    table = c['table'] if table is None else table
    b, k, n = rb.shape
    assert table.shape == (b, c['rows'], n) and rb.shape == pwr.shape
    tab = torch.as_tensor(np.array(table), device='cuda')
    rb_t, pwr_t = (torch.as_tensor(np.array(a, dtype=np.int32), device='cuda') for a in (rb, pwr))
    g_s, g_c = (Guarded((b, k, n), torch.float32) if on else None for on in (sinr, cap))
    g_t, g_d = Guarded((b, k), torch.float32), Guarded((b, k), torch.int32)
    launches = _native.evaltab_launches
    _native.evaluate_table(tab.data_ptr(), _native.EVALTAB_F64 if table.dtype == np.float64 else _native.EVALTAB_F32, c['rows'],
                           rb_t.data_ptr(), pwr_t.data_ptr(), *(t.data_ptr() for t in _device_inputs(c)), b, k, c['d'], n, c['r'],
                           g_s.array.data_ptr() if sinr else 0, g_c.array.data_ptr() if cap else 0, g_t.array.data_ptr(),
                           g_d.array.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.evaltab_launches == launches + 1
    for g in (g_s, g_c, g_t, g_d):
        assert g is None or g.intact()
    return tuple(None if g is None else g.array.cpu().numpy() for g in (g_s, g_c, g_t, g_d))


def _same(a, m):
    return all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(a, m))


# ------------------------------------------------------------------------------------------ 1: direct launches
@pytest.mark.parametrize('case', teu.CASES)
def test_direct_launch_against_the_float64_reference(case):
    n, r, k, b, dtype, extra = case
    c = teu.make_case(*case)
    ref_sinr, ref_cap, ref_total, decided = teu.case_ref(*case)
    sinr, cap, total, domain = _launch(c)
    assert np.isfinite(sinr).all() and np.isfinite(cap).all() and np.isfinite(total).all()
    assert (domain == 0).all()
    e_s, e_c = evu.rel_err(sinr, ref_sinr), evu.rel_err(cap[decided], ref_cap[decided])
    left_out = float((~decided).mean())
    print(f'{n} links, {r} RBs, K = {k}, B = {b}, {dtype} [{n + extra} rows]: sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e}; '
          f'{left_out:.2%} left out at the threshold; LDS {teu.lds_bytes(n, r)} B')
    assert left_out <= teu.THRESHOLD_CAP
    assert e_s <= teu.BAR
    assert e_c <= teu.BAR
    assert (cap > 0).any()
    # the total: the double sum of the returned float capacities in the documented order, rounded once
    assert np.array_equal(_f32_bits(total), _f32_bits(teu.totals_in_order(cap, c['rb'], r)))
    # two calls give the same words; null planes leave the totals, the flags and the other plane as they are
    assert _same(_launch(c), (sinr, cap, total, domain))
    assert _same(_launch(c, sinr=False, cap=False), (None, None, total, domain))
    assert _same(_launch(c, sinr=False), (None, cap, total, domain))
    assert _same(_launch(c, cap=False), (sinr, None, total, domain))


def test_a_candidate_does_not_depend_on_its_neighbours_or_on_the_layout_of_the_table():
    """Every candidate of a 17-candidate launch equals, bit for bit, a K = 1 launch of that candidate alone; the same entries as
    float64 [B, N, N] and in the live layout [B, N+1, N] give the same words."""
    case = (50, 6, 17, 1, 'float32', 0)
    c = teu.make_case(*case)
    first = _launch(c)
    for q in range(c['k']):
        alone = _launch(c, c['rb'][:, q:q + 1], c['pwr'][:, q:q + 1])
        assert _same(alone, tuple(a[:, q:q + 1] for a in first)), q
    wide = np.full((c['b'], c['n'] + 1, c['n']), -np.inf)                # the row no launch reads: it would raise the flag
    wide[:, :c['n']] = c['table']
    assert _same(_launch(dict(c, rows=c['n'] + 1), table=wide), first)
    assert len({_f32_bits(first[2][:, q]).tobytes() for q in range(c['k'])}) > 2


# ------------------------------------------------------------------------------------------ 2: the domain flag
def _pairs_by_readers(rb, r, e):
    """readers[j, i]: the candidates of env e whose evaluation reads entry [j, i], j != i (the two links share an RB)."""
    on = (rb[e] >= 0) & (rb[e] < r)
    return (rb[e][:, :, None] == rb[e][:, None, :]) & on[:, :, None] & on[:, None, :]          # [k, j, i]


def test_the_domain_flag_is_raised_for_exactly_the_candidates_that_read_a_bad_entry():
    case = (50, 6, 9, 5, 'float64', 1)
    n, r, k, b, _, _ = case
    c = teu.make_case(*case)
    base = _launch(c)
    off = ~np.eye(n, dtype=bool)
    bad, marks = c['table'].copy(), []
    # env 1: a NaN in an entry exactly one candidate reads; env 3: a -inf likewise; env 2: a NaN in an entry no candidate reads;
    # env 4: a +inf in an interferer entry exactly one candidate reads
    for e, value, readers in ((1, np.nan, 1), (3, -np.inf, 1), (2, np.nan, 0), (4, np.inf, 1)):
        reads = _pairs_by_readers(c['rb'], r, e)
        count = reads.sum(axis=0)
        j, i = np.argwhere((count == readers) & off)[0]
        q = int(np.flatnonzero(reads[:, j, i])[0]) if readers else None
        bad[e, j, i] = value
        marks.append((e, q, int(j), int(i), value))
    got = _launch(c, table=bad)
    want = np.zeros((b, k), dtype=np.int32)
    for e, q, j, i, value in marks:
        if q is not None and not value > -np.inf:
            want[e, q] = 1
    print('flagged candidates (env, candidate):', np.argwhere(got[3] != 0).tolist())
    assert np.array_equal(got[3], want) and want.sum() == 2
    # every other candidate's words are unchanged; the +inf candidate's too, but for the one receiver
    (e4, q4, j4, i4, _) = marks[3]
    touched = want.astype(bool)
    touched[e4, q4] = True
    for a, m in zip(got[:3], base[:3]):
        assert np.array_equal(bits(a[~touched]), bits(m[~touched]))
    keep = np.arange(n) != i4
    assert np.array_equal(bits(got[0][e4, q4, keep]), bits(base[0][e4, q4, keep]))
    # +inf: the gain is 0 and the SINR is the one without that interferer - the float64 reference on the same table, and bit for bit
    # the launch in which the interferer is on no RB (acc + 0.0 is acc)
    assert got[3][e4, q4] == 0 and np.isfinite(got[0][e4, q4]).all()
    ref_sinr, _, _, _ = teu.reference(c, pl=bad[:, :n].astype(np.float64))
    assert abs(got[0][e4, q4, i4] - ref_sinr[e4, q4, i4]) <= teu.BAR * max(abs(ref_sinr[e4, q4, i4]), 1.0)
    assert got[0][e4, q4, i4] >= base[0][e4, q4, i4]
    rb = c['rb'].copy()
    rb[e4, q4, j4] = -1
    without = _launch(c, rb=rb)
    assert _f32_bits(without[0][e4, q4, i4]) == _f32_bits(got[0][e4, q4, i4])


# ------------------------------------------------------------------------------------------ 3: bit for bit against the step
def _channel_model(**kw):
    from gym_d2d_amd.path_loss import LogDistancePathLoss, SpatialChannelPathLoss
    return type('Channel', (SpatialChannelPathLoss,), dict(median=LogDistancePathLoss, median_kwargs={'ple': 3.5}, **kw))


def _env(b, cues, pairs, rbs, model, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    cfg = {'num_rbs': rbs, 'num_cues': cues, 'num_due_pairs': pairs, 'seed': 4321}
    if model is not None:
        cfg['path_loss_model'] = model
    return VecD2DEnv(cfg, num_envs=b, **kw)


def _actions(env, rng, k=None):
    highs = env._initial_action_highs()
    shape = (env.num_envs,) if k is None else (env.num_envs, k)
    a = np.stack([rng.integers(0, h, shape) for h in highs], -1).astype(np.int32)
    return torch.as_tensor(a, device='cuda')


def _eq(a, m):
    return a.shape == m.shape and bool(torch.equal(a.contiguous().view(torch.int32), m.contiguous().view(torch.int32)))


def _current_planes_are_the_steps(env, table=None):
    v = env._view()
    res = env.evaluate_table(v.rb[:, None].contiguous(), v.pwr[:, None].contiguous(), table=table)
    assert set(res) == {'total_mbps', 'domain', 'sinr_db', 'capacity_mbps'}
    assert res['domain'].dtype == torch.int32 and tuple(res['domain'].shape) == tuple(res['total_mbps'].shape) == (env.num_envs, 1)
    assert _eq(res['sinr_db'][:, 0], v.sinr_db) and _eq(res['capacity_mbps'][:, 0], v.capacity_mbps)
    assert int(res['domain'].abs().sum()) == 0


@pytest.mark.parametrize('dtype', ['float64', 'float32'])
@pytest.mark.parametrize('fading', ['rayleigh', None])
@pytest.mark.parametrize('shape', [(3, 4, 6, 4), (2, 20, 45, 6)])
def test_the_planes_are_the_steps_on_the_channel_route(shape, fading, dtype):
    env = _env(*shape, _channel_model(fading=fading, table_dtype=dtype, num_sinusoids=8))
    try:
        rng = np.random.default_rng(5)
        env.reset(seed=11)
        assert env.simulator.path_loss_table.route == 'channel' and str(env.simulator.path_loss_table.live.dtype) == 'torch.' + dtype
        _current_planes_are_the_steps(env)
        for _ in range(3):
            a = _actions(env, rng)
            if fading is None:
                pred = {name: t.clone() for name, t in env.evaluate_table_actions(a[:, None].contiguous()).items()}
            _, _, _, info = env.step(a)
            if fading is None:                         # nothing moves, nothing is drawn: the table is the next step's
                assert _eq(pred['sinr_db'][:, 0], info['sinr_db']) and _eq(pred['capacity_mbps'][:, 0], info['capacity_mbps'])
                assert int(pred['domain'].sum()) == 0
            _current_planes_are_the_steps(env)
        _current_planes_are_the_steps(env, table=env.simulator.path_loss_table.live)
        assert float(env._view().capacity_mbps.sum()) > 0 and env.status_flags() == 0
    finally:
        env.close()


def test_the_planes_are_the_steps_on_the_per_step_route():
    model = runpy.run_path(str(ROOT / 'examples' / 'per_step_path_loss.py'), run_name='per_step_path_loss')['ShadowedCostHata']
    env = _env(3, 4, 6, 4, model)
    try:
        rng = np.random.default_rng(6)
        env.reset(seed=3)
        assert env.simulator.path_loss_table.route == 'per_step'
        _current_planes_are_the_steps(env)
        for _ in range(2):
            env.step(_actions(env, rng))
            _current_planes_are_the_steps(env)
        _current_planes_are_the_steps(env, table=env.simulator.path_loss_table.live)
    finally:
        env.close()


def test_the_array_route_is_served_when_compute_returns_the_snr_row_and_refused_by_name_when_not():
    from gym_d2d_amd.path_loss import ArrayPathLoss

    class Plain(ArrayPathLoss):
        def compute(self, view):
            return 20 * view.xp.log10(view.distance()) + 40.0

    class WithSnrRow(Plain):
        def compute(self, view):
            pl = Plain.compute(self, view)
            return pl, view.xp.diagonal(pl, dim1=1, dim2=2) + 1.5

    env = _env(3, 4, 6, 4, WithSnrRow)
    try:
        rng = np.random.default_rng(12)
        env.reset(seed=5)
        table = env.simulator.path_loss_table
        assert table.route == 'array' and tuple(table.live.shape) == (3, 11, 10)
        _current_planes_are_the_steps(env)
        a = _actions(env, rng)
        pred = {name: t.clone() for name, t in env.evaluate_table_actions(a[:, None].contiguous()).items()}
        _, _, _, info = env.step(a)                    # evaluated once per reset: the table is the next step's
        assert _eq(pred['sinr_db'][:, 0], info['sinr_db']) and _eq(pred['capacity_mbps'][:, 0], info['capacity_mbps'])
        _current_planes_are_the_steps(env)
    finally:
        env.close()
    env = _env(3, 4, 6, 4, Plain)
    try:
        env.reset(seed=5)
        assert env.simulator.path_loss_table.route == 'array' and env.simulator.path_loss_table.live is None
        z = torch.zeros((3, 1, 10), dtype=torch.int32, device='cuda')
        with pytest.raises(ValueError, match=r"evaluate_table\(\).*'array'.*pass table="):
            env.evaluate_table(z, z.clone())
        flat = torch.full((3, 10, 10), 90.0, device='cuda')
        assert tuple(env.evaluate_table(z, z.clone(), table=flat)['sinr_db'].shape) == (3, 1, 10)
    finally:
        env.close()


def test_links_on_fixed_actions_keep_their_planes_and_need_them_exported():
    model = _channel_model(fading=None, num_sinusoids=8)
    env = _env(3, 4, 6, 4, model, cue_actions='traffic')
    try:
        rng = np.random.default_rng(7)
        env.reset(seed=2)
        assert env.num_agents == 6 and env.num_links == 10
        a = _actions(env, rng)
        pred = {name: t.clone() for name, t in env.evaluate_table_actions(a[:, None].contiguous()).items()}
        _, _, _, info = env.step(a)
        # the four CUE links have no column: they keep the rb / power the decoded planes hold, as the step does
        assert tuple(pred['sinr_db'].shape) == (3, 1, 10)
        assert _eq(pred['sinr_db'][:, 0], info['sinr_db']) and _eq(pred['capacity_mbps'][:, 0], info['capacity_mbps'])
    finally:
        env.close()
    env = _env(3, 4, 6, 4, model, cue_actions='traffic', export_actions=False)
    try:
        env.reset(seed=2)
        with pytest.raises(ValueError, match=r'evaluate_table_actions\(\).*export_actions=True'):
            env.evaluate_table_actions(torch.zeros((3, 1, 6), dtype=torch.int32, device='cuda'))
        # the planes form reads nothing the env did not export
        z = torch.zeros((3, 2, 10), dtype=torch.int32, device='cuda')
        assert tuple(env.evaluate_table(z, z.clone())['total_mbps'].shape) == (3, 2)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 4: the env is untouched
def test_a_call_leaves_the_env_as_it_was():
    from gym_d2d_amd import _native
    env = _env(3, 4, 6, 4, _channel_model(fading='rayleigh', num_sinusoids=8))
    try:
        rng = np.random.default_rng(8)
        env.reset(seed=4)
        env.step(_actions(env, rng))
        live = env.simulator.path_loss_table.live
        names = [k for k in ('rb', 'pwr', 'pos_x', 'pos_y', 'reward', 'sinr_db', 'snr_db', 'rate_bps', 'capacity_mbps', 'env_flags')
                 if env._t.get(k) is not None]
        torch.cuda.synchronize()
        before = {k: env._t[k].clone() for k in names}
        table, steps, flags, fills, launches = live.clone(), env.num_steps, env.status_flags(), _native.channel_launches, _native.evaltab_launches
        env.evaluate_table_actions(_actions(env, rng, k=9))
        rb = torch.as_tensor(rng.integers(-1, 5, (3, 17, 10)).astype(np.int32), device='cuda')
        env.evaluate_table(rb, torch.full_like(rb, 10), planes=())
        torch.cuda.synchronize()
        assert _native.evaltab_launches == launches + 2 and _native.channel_launches == fills
        assert env.num_steps == steps and env.status_flags() == flags
        assert env.simulator.path_loss_table.live is live and np.array_equal(bits(live), bits(table))
        for k in names:
            assert np.array_equal(bits(env._t[k]), bits(before[k])), k
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ 5: table= on a native env, the refusals
def _law_table(env):
    """The native law as a float64 table, in torch on the device: a_tx[tx_j] + a_rx[rx_i] + 10 exponent[tx_j] log10 d(tx_j, rx_i)."""
    sim = env.simulator
    law = {k: torch.as_tensor(np.asarray(v, dtype=np.float64), device='cuda') for k, v in sim.path_loss_table.law.items()
           if k in ('a_tx_db', 'a_rx_db', 'exponent')}
    tx, rx = (torch.as_tensor(np.asarray(j, dtype=np.int64), device='cuda') for j in (sim.link_tx, sim.link_rx))
    p = env.link_positions().to(torch.float64)
    d = torch.sqrt((p[:, :, None, 0] - p[:, None, :, 2]) ** 2 + (p[:, :, None, 1] - p[:, None, :, 3]) ** 2)           # [b, j, i]
    return (law['a_tx_db'][tx][None, :, None] + law['a_rx_db'][rx][None, None, :]
            + 10.0 * law['exponent'][tx][None, :, None] * torch.log10(d)).contiguous()


@pytest.mark.parametrize('ple', [2.0, 3.5])
def test_a_supplied_table_serves_a_native_env_and_agrees_with_evaluate(ple):
    from gym_d2d_amd.path_loss import LogDistancePathLoss
    model = type('Ld', (LogDistancePathLoss,), {'__init__': lambda self, f: LogDistancePathLoss.__init__(self, f, ple=ple)})
    b, cues, pairs, r, k = 3, 5, 20, 7, 9
    env = _env(b, cues, pairs, r, model)
    try:
        rng = np.random.default_rng(9)
        env.reset(seed=6)
        n = env.num_links
        assert env.simulator.path_loss_table.route == 'native'
        table = _law_table(env)
        rb = rng.integers(0, r, (b, k, n)).astype(np.int32)
        rb[rng.random(rb.shape) < 0.1] = -1
        pwr = rng.integers(evu.P_LOW, 21, (b, k, n)).astype(np.int32)
        rb_t, pwr_t = torch.as_tensor(rb, device='cuda'), torch.as_tensor(pwr, device='cuda')
        got = {name: t.cpu().numpy() for name, t in env.evaluate_table(rb_t, pwr_t, table=table).items()}
        nat = {name: t.cpu().numpy() for name, t in env.evaluate(rb_t, pwr_t).items()}
        sim = env.simulator
        ocols = orc.device_columns(*orc.device_configs(cues, pairs)[1:])
        ref_sinr, ref_cap, _ = evu.evaluate_ref(np.zeros((b, 1 + cues + 2 * pairs, 2)), sim.link_tx, sim.link_rx, rb, pwr,
                                                {'ocols': ocols, 'pl': table.cpu().numpy()}, r)
        decided = np.abs(ref_sinr - ocols.sens_dbm[np.asarray(sim.link_rx)][None, None, :]) > evu.THRESHOLD_DB
        assert float((~decided).mean()) <= evu.THRESHOLD_CAP and (got['domain'] == 0).all()
        for name, res in (('evaluate_table', got), ('evaluate', nat)):
            e_s, e_c = evu.rel_err(res['sinr_db'], ref_sinr), evu.rel_err(res['capacity_mbps'][decided], ref_cap[decided])
            print(f'ple {ple}: {name}() sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e}')
            assert e_s <= evu.BAR and e_c <= evu.BAR
        # float32 entries and the [B, N+1, N] layout are taken too; what is no such tensor is refused by name
        wide = torch.full((b, n + 1, n), float('nan'), dtype=torch.float32, device='cuda')
        wide[:, :n] = table
        # (the bar plus what the format costs: the signal's and the interferers' entries, below 256 dB, each within half an ulp 2^-17 dB)
        assert evu.rel_err(env.evaluate_table(rb_t, pwr_t, table=wide)['sinr_db'].cpu().numpy(), ref_sinr) <= evu.BAR + 2.0 ** -16
        for bad in (table.cpu(), table[:, :, :-1], table.transpose(1, 2), table.to(torch.float16), table[:, :-1].contiguous(), table[0]):
            with pytest.raises(ValueError, match='table must be'):
                env.evaluate_table(rb_t, pwr_t, table=bad)
        with pytest.raises(ValueError, match=r"evaluate_table\(\).*'native'.*pass table="):
            env.evaluate_table(rb_t, pwr_t)
        with pytest.raises(ValueError, match=r"evaluate_table\(\).*'native'.*pass table="):
            env.evaluate_table_actions(_actions(env, rng, k=2))
    finally:
        env.close()


def test_out_is_honoured_bad_arguments_are_refused_by_name_and_evaluate_keeps_refusing_the_route():
    import json
    env = _env(3, 4, 6, 4, _channel_model(fading=None, num_sinusoids=8))
    try:
        env.reset(seed=2)
        b, n, k = 3, 10, 3
        rng = np.random.default_rng(8)
        rb = torch.as_tensor(rng.integers(0, 4, (b, k, n)).astype(np.int32), device='cuda')
        pwr = torch.as_tensor(rng.integers(0, 20, (b, k, n)).astype(np.int32), device='cuda')
        own = {name: v.clone() for name, v in env.evaluate_table(rb, pwr).items()}
        out = {'total_mbps': torch.empty((b, k), device='cuda'), 'domain': torch.empty((b, k), dtype=torch.int32, device='cuda'),
               'sinr_db': torch.empty((b, k, n), device='cuda')}
        got = env.evaluate_table(rb, pwr, planes=('sinr_db',), out=out)
        assert set(got) == set(out) and all(got[name] is out[name] for name in out)
        assert all(_eq(out[name], own[name]) for name in out)
        for bad_rb, bad_pwr, text in ((rb.long(), pwr, 'rb must be'), (rb[:, :, :-1].contiguous(), pwr, 'rb must be'),
                                      (rb.transpose(0, 1), pwr, 'rb must be'), (rb[:, 0], pwr, 'rb must be'), (rb.cpu(), pwr, 'rb must be'),
                                      (rb, pwr.float(), 'power_dbm must be'), (rb, pwr[:, :2].contiguous(), 'one shape'),
                                      (rb[:, :0].contiguous(), pwr[:, :0].contiguous(), 'rb must be')):
            with pytest.raises(ValueError, match=text):
                env.evaluate_table(bad_rb, bad_pwr)
        for bad in (out['total_mbps'], {'total_mbps': out['total_mbps']}, dict(out, sinr_db=out['sinr_db'].double()),
                    dict(out, domain=out['domain'].float()), dict(out, capacity_mbps=torch.empty((b, k, n), device='cuda')),
                    dict(out, total_mbps=out['total_mbps'][:, :2]), dict(out, sinr_db=out['sinr_db'].cpu())):
            with pytest.raises(ValueError, match=r'evaluate_table\(\): out must be'):
                env.evaluate_table(rb, pwr, planes=('sinr_db',), out=bad)
        with pytest.raises(ValueError, match='planes must be'):
            env.evaluate_table(rb, pwr, planes=('snr_db',))
        with pytest.raises(ValueError, match='actions must be'):
            env.evaluate_table_actions(torch.zeros((b, k, n + 1), dtype=torch.int32, device='cuda'))
        with pytest.raises(ValueError, match='actions must be'):
            env.evaluate_table_actions(torch.zeros((b, k, n), device='cuda'))
        # evaluate() keeps refusing the route, in its golden words
        golden = json.loads((ROOT / 'tests' / 'golden' / 'pair_kernel_messages.json').read_text())
        with pytest.raises(ValueError) as info:
            env.evaluate(rb, pwr)
        assert str(info.value) == golden['evaluate.refusal/channel']
    finally:
        env.close()


def test_the_example_delivers_what_it_predicted():
    res = runpy.run_path(str(ROOT / 'examples' / 'channel_candidate_search.py'), run_name='__main__')['results']
    print(res)
    # the planes are the step's bit for bit; the two totals are float32 sums of them in different orders (16 terms)
    assert res['max_rel_gap'] <= 16 * 2.0 ** -24
    assert res['predicted_mbps'] > res['mean_candidate_mbps'] > 0

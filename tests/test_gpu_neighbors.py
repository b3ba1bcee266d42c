"""The neighbour graph on the GPU (VecD2DEnv.coupling / neighbors, NeighborObsFunction, csrc/d2d_graph.hip) against the oracle.

The yardstick: ref[b, i, j] = eirp_off_db[tx_j] - orc.pair_path_loss_db(...)[b, j, i] on the float32 positions read back from the
env, and a NumPy stable descending sort of each row with the diagonal removed (neighbors_util); the bar is the project's 1e-5 on dB
quantities (golden_util.rel_err).  Index order: [b, i, j], receiver link i first.  The cases are rb_sensing_util.CASES."""
import json
import runpy
from pathlib import Path

import numpy as np
import pytest

import neighbors_util as nbu
from golden_util import load_case, rel_err
from oracle import d2d_oracle as orc
from rb_sensing_util import CASES, _models, _state
from sim_util import env_config_for, oracle_spec, random_layout

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parent.parent
BAR = 1e-5
_cache = {}


def _ks(n):
    return sorted({1, 8, min(n - 1, 64)})


def _build(name):
    """An env stepped once on a random_layout, its coupling matrix and neighbour lists, the step's planes and the oracle's matrix."""
    if name in _cache:
        return _cache[name]
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.traffic_model import DownlinkTrafficModel
    rng = np.random.default_rng(sum(map(ord, name)))
    if CASES[name] is None:
        case = load_case('case07_device_config')
        b0, cue_actions = 2, 'agent'
        cfg = env_config_for(case)
        cues, dues, r = case.meta['num_cues'], case.meta['num_due_pairs'], case.meta['num_rbs']
        spec = oracle_spec(case)
        cols = orc.device_columns(case.cfgs, case.is_bs)
    else:
        b0, cues, dues, r, model, cue_actions, down = CASES[name]
        cls, spec = _models()[model]
        cfg = {'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'path_loss_model': cls}
        if down:
            cfg['traffic_model'] = DownlinkTrafficModel
        cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    env = VecD2DEnv(cfg, num_envs=b0, cue_actions=cue_actions)
    env.reset(seed=3)
    if CASES[name] is not None:              # (case07 pins devices: the layout its reset drew around them stays)
        env.simulator.set_positions(random_layout(rng, b0, cues, dues))
    p = env.num_pwr_actions
    highs = ([r * p[env._cue_kind]] * cues if cue_actions == 'agent' else []) + [r * p['due']] * dues
    actions = torch.as_tensor(rng.integers(0, highs, (b0, len(highs))).astype(np.int32), device=env.device)
    _, _, _, info = env.step(actions)
    n = cues + dues
    coupling = env.coupling().cpu().numpy()
    lists = {k: tuple(t.cpu().numpy() for t in env.neighbors(k)) for k in _ks(n)}
    pos, rb, pwr = _state(env)
    tx, rx = env.simulator.link_tx, env.simulator.link_rx
    out = dict(env=env, coupling=coupling, lists=lists, pos=pos, rb=rb, pwr=pwr, tx=tx, rx=rx, cols=cols, spec=spec, r=r, n=n,
               step_sinr=info['sinr_db'].cpu().numpy(), ref=nbu.coupling_ref(pos, tx, rx, cols, spec))
    assert env.status_flags() == 0
    _cache[name] = out
    return out


@pytest.fixture(scope='module', autouse=True)
def _close_envs():
    yield
    for c in _cache.values():
        c['env'].close()
    _cache.clear()


@pytest.mark.parametrize('name', list(CASES))
def test_coupling_against_the_oracle(name):
    c = _build(name)
    assert c['coupling'].shape == c['ref'].shape and c['coupling'].dtype == np.float32 and np.isfinite(c['ref']).all()
    e = rel_err(c['coupling'], c['ref'])
    print(f'{name}: coupling() vs the oracle rel_err {e:.3e} over {c["ref"].size} entries')
    assert e <= BAR


@pytest.mark.parametrize('name', list(CASES))
def test_neighbor_values_against_the_oracle_s_sorted_rows(name):
    c = _build(name)
    for k, (idx, cdb) in c['lists'].items():
        assert idx.shape == cdb.shape == (c['ref'].shape[0], c['n'], k) and idx.dtype == np.int32 and cdb.dtype == np.float32
        _, vals, _ = nbu.ranked(c['ref'], k)
        e = rel_err(cdb, vals)
        print(f'{name} k={k}: neighbors() values vs the oracle\'s m-th largest rel_err {e:.3e} over {vals.size} entries')
        assert e <= BAR
        # and they are the dense matrix's own entries, bit for bit
        assert np.array_equal(np.take_along_axis(c['coupling'], idx.astype(np.int64), axis=2).view(np.uint32), cdb.view(np.uint32))


@pytest.mark.parametrize('name', list(CASES))
def test_neighbor_indices_against_the_oracle_s_stable_sort(name):
    c = _build(name)
    for k, (idx, _) in c['lists'].items():
        nbu.check_sets(idx, c['n'])
        left_out, ties = nbu.check_indices(idx, c['ref'], k)
        print(f'{name} k={k}: indices equal on every comparable entry; {left_out:.2%} left out as near ties, {ties:.1%} of the gaps exact ties')
        if 'down' in name and k > 1:
            assert ties > 0.2                                        # the ascending-j rule is exercised


@pytest.mark.parametrize('name', list(CASES))
def test_coupling_rebuilds_the_step_and_the_sensed_interference(name):
    """GPU against GPU: sum over j != i with rb_j == rb_i of lin(pwr_j + coupling[b, i, j]) is the step's interference."""
    c = _build(name)
    env, cols = c['env'], c['cols']
    b, n = c['rb'].shape
    lin = 10.0 ** ((c['pwr'][:, None, :] + c['coupling'].astype(np.float64)) / 10.0)             # [b, i, j] mW
    lin[:, np.arange(n), np.arange(n)] = 0.0
    onehot = (c['rb'][:, :, None] == np.arange(c['r'])[None, None, :]).astype(np.float64)        # [b, j, r]
    per_rb = np.einsum('bij,bjr->bir', lin, onehot)
    own = np.take_along_axis(per_rb, c['rb'][:, :, None], axis=2)[:, :, 0]
    diag = c['coupling'][:, np.arange(n), np.arange(n)].astype(np.float64)
    sig = c['pwr'] + diag + np.asarray(cols.rx_off_db)[c['rx']][None, :]
    sinr = sig - 10.0 * np.log10(own + 10.0 ** (np.asarray(cols.noise_dbm)[c['rx']][None, :] / 10.0))
    e = rel_err(sinr, c['step_sinr'])
    print(f'{name}: sinr_db rebuilt from coupling() vs the step rel_err {e:.3e}')
    assert e <= BAR
    sensed = env.sense('interference_mw').cpu().numpy()
    empty = per_rb == 0.0
    assert (sensed[empty] == 0.0).all() and (sensed[~empty] > 0.0).all()
    e2 = rel_err(10 * np.log10(sensed[~empty].astype(np.float64)), 10 * np.log10(per_rb[~empty]))
    print(f'{name}: per-RB sums of coupling() vs sense(interference_mw) rel_err {e2:.3e} in dB')
    assert e2 <= BAR


def _obs_env(autoreset, b=12, cues=9, dues=14, r=6, k=None):
    from gym_d2d_amd.envs import NeighborObsFunction, VecD2DEnv
    fn = NeighborObsFunction
    if k is not None:
        fn = type(f'Neighbor{k}', (NeighborObsFunction,), {'k': k})
    return VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'obs_fn': fn}, num_envs=b, autoreset=autoreset)


def _check_obs(env, obs, info, k):
    """The observation against the oracle-side gather of the step's planes through the checked indices; own block bit for bit."""
    n = env.num_links
    pos, rb, pwr = _state(env)
    cols = orc.device_columns(*orc.device_configs(env.num_cues, env.num_due_pairs)[1:])
    ref = nbu.coupling_ref(pos, env.simulator.link_tx, env.simulator.link_rx, cols, orc.PathLossSpec())
    idx, cdb = (t.cpu().numpy() for t in env._neighbors)
    nbu.check_sets(idx, n)
    nbu.check_indices(idx, ref, k)
    got = obs.cpu().numpy()
    assert got.shape == (env.num_envs, n, 4 * (k + 1)) and got.dtype == np.float32
    sinr, snr = info['sinr_db'].cpu().numpy(), info['snr_db'].cpu().numpy()
    assert np.array_equal(info['rb'].cpu().numpy(), rb) and np.array_equal(info['tx_pwr_dbm'].cpu().numpy(), pwr)
    want = nbu.gather_obs(idx.astype(np.int64), np.take_along_axis(ref, idx.astype(np.int64), axis=2), rb, pwr, sinr, snr)
    e = rel_err(got, want)
    assert e <= BAR, e
    g4, w4 = got.reshape(env.num_envs, n, k + 1, 4), want.reshape(env.num_envs, n, k + 1, 4)
    assert np.array_equal(g4[:, :, 1:, 1:], w4[:, :, 1:, 1:].astype(np.float32))                 # gathered planes: exact
    own = np.stack([rb.astype(np.float32), pwr.astype(np.float32), sinr, snr], axis=-1)
    assert np.array_equal(g4[:, :, 0].view(np.uint32), own.view(np.uint32))                       # own block: info bit for bit
    assert np.array_equal(g4[:, :, 1:, 0].view(np.uint32), cdb.view(np.uint32))
    return e


@pytest.mark.parametrize('k', [None, 3])
def test_neighbor_obs_function_is_the_gather_of_the_step_s_planes(k):
    env = _obs_env(False, k=k)
    k = k or 8
    try:
        assert env.observation_space.shape == (4 * (k + 1),)
        obs = env.reset(seed=7)
        rng = np.random.default_rng(1)
        for step in range(3):
            a = torch.as_tensor(rng.integers(0, 6 * 21, (env.num_envs, env.num_links)).astype(np.int32), device=env.device)
            obs, _, _, info = env.step(a)
            e = _check_obs(env, obs, info, k)
            print(f'k={k} step {step}: observation vs the oracle-side gather rel_err {e:.3e}')
        assert env.status_flags() == 0
    finally:
        env.close()


def test_autoreset_reselects_exactly_the_envs_that_were_reset():
    """Three episodes of staggered envs: after every step the cached lists equal a fresh neighbors(k) bit for bit, an env that was
    reset got new rows, and the others kept theirs - shown by a poisoned row that survives until its env's reset."""
    env = _obs_env(True)
    k, b = 8, env.num_envs
    try:
        env.reset(seed=11, elapsed=np.arange(b) % 10)
        rng = np.random.default_rng(4)
        shape = (b, env.num_links, k)
        fresh = (torch.empty(shape, dtype=torch.int32, device=env.device), torch.empty(shape, dtype=torch.float32, device=env.device))
        poison, poisoned, resets = -12345, set(), np.zeros(b, int)
        for step in range(36):
            idx_t, cdb_t = env._neighbors
            victim = int(rng.integers(0, b))
            idx_t[victim, 0, :] = poison
            poisoned.add(victim)
            a = torch.as_tensor(rng.integers(0, 6 * 21, (b, env.num_links)).astype(np.int32), device=env.device)
            before = env._t['pos_x'].clone()
            obs, _, _, info = env.step(a)
            was_reset = info['reset'].cpu().numpy()
            moved = (env._t['pos_x'] != before).any(dim=1).cpu().numpy()
            assert np.array_equal(moved, was_reset)
            resets += was_reset
            assert env._neighbors[0] is idx_t                        # the env's own tensors, rewritten in place
            cached = idx_t.cpu().numpy()
            for e in list(poisoned):
                if was_reset[e]:
                    poisoned.discard(e)
                else:
                    assert (cached[e, 0] == poison).all()            # env_mask honoured: the row was not touched
            env.neighbors(k, out=fresh)
            want_idx, want_cdb = fresh[0].cpu().numpy(), fresh[1].cpu().numpy()
            clean = np.ones(b, bool); clean[list(poisoned)] = False
            assert np.array_equal(cached[clean], want_idx[clean])
            assert np.array_equal(cached[~clean][:, 1:], want_idx[~clean][:, 1:])
            assert np.array_equal(cdb_t.cpu().numpy().view(np.uint32), want_cdb.view(np.uint32))
            for e in list(poisoned):                                 # heal, so that the observation below is checkable
                idx_t[e, 0, :] = fresh[0][e, 0, :]
            poisoned.clear()
            if step % 8 == 7:
                _check_obs(env, env._observe(env._view()), info, k)      # the gather once more, through the healed rows
        assert (resets >= 3).all()
    finally:
        env.close()


def test_user_obs_function_sees_the_lists_and_others_launch_nothing():
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import RbSensingObsFunction, VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import ArrayObsFunction, LinearObsFunction, OwnLinkObsFunction, SignalPlanesObsFunction
    from gym_d2d_amd.spaces import Box
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Strongest(ArrayObsFunction):
        native_mode = _native.OBS_NONE
        needs_neighbors = 2

        def get_obs_space(self, env_config):
            return Box(low=-np.inf, high=np.inf, shape=(2,))

        def compute(self, view):
            assert view.neighbor_idx.dtype == torch.int32
            return view.neighbor_coupling_db

    def launches(obs_fn, steps=3, **kw):
        before = dict(_native.graph_launches)
        env = VecD2DEnv(dict(small, obs_fn=obs_fn), num_envs=4, **kw)
        try:
            obs = env.reset(seed=1)
            for _ in range(steps):
                env.step(env.action_buffer().clone())
            assert (env._graph is None) == (not getattr(env.obs_fn, 'needs_neighbors', 0))
            if obs_fn is Strongest:
                idx, cdb = env.neighbors(2, out=(torch.empty((4, 6, 2), dtype=torch.int32, device=env.device),
                                                 torch.empty((4, 6, 2), dtype=torch.float32, device=env.device)))
                assert tuple(obs.shape) == (4, 6, 2) and torch.equal(obs, cdb) and torch.equal(env._neighbors[0], idx)
        finally:
            env.close()
        return {w: _native.graph_launches[w] - before[w] for w in before}
    for fn in (LinearObsFunction, OwnLinkObsFunction, SignalPlanesObsFunction, RbSensingObsFunction):
        assert launches(fn) == {'coupling': 0, 'neighbors': 0, 'neighbor_obs': 0}
        assert launches(fn, autoreset=True) == {'coupling': 0, 'neighbors': 0, 'neighbor_obs': 0}
    got = launches(Strongest)
    assert got == {'coupling': 0, 'neighbors': 2, 'neighbor_obs': 0}, got       # reset() and the explicit neighbors(2, out=...)


def test_selection_runs_at_reset_and_the_gather_every_step():
    from gym_d2d_amd import _native
    env = _obs_env(False, k=5)
    try:
        before = dict(_native.graph_launches)
        env.reset(seed=2)
        for _ in range(3):
            env.step(env.action_buffer().clone())
        env.reset()
        got = {w: _native.graph_launches[w] - before[w] for w in before}
        assert got == {'coupling': 0, 'neighbors': 2, 'neighbor_obs': 5}, got
    finally:
        env.close()


def test_two_calls_are_bit_identical_and_out_is_validated_inside_guard_words():
    """mid_ld35_agent has N = 160 links (no multiple of 64); k = 7 is no multiple of 4."""
    c = _build('mid_ld35_agent')
    env, n = c['env'], c['n']
    b = c['ref'].shape[0]
    assert n % 64 != 0
    assert np.array_equal(env.coupling().cpu().numpy().view(np.uint32), c['coupling'].view(np.uint32))
    assert env.coupling() is env.coupling()                              # the env's one block, reused
    for k, (idx, cdb) in c['lists'].items():
        i2, c2 = env.neighbors(k)
        assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(c2.cpu().numpy().view(np.uint32), cdb.view(np.uint32))
        assert env.neighbors(k)[0] is i2
    guard, pad, k = 0x5AFEC0DE, 64, 7

    def arena(words, dtype):
        a = torch.full((words + 2 * pad,), guard, dtype=torch.int32, device=env.device)
        return a, a[pad:pad + words].view(dtype)
    a_c, out_c = arena(b * n * n, torch.float32)
    assert env.coupling(out=out_c.view(b, n, n)).data_ptr() == out_c.data_ptr()
    a_i, out_i = arena(b * n * k, torch.int32)
    a_v, out_v = arena(b * n * k, torch.float32)
    got = env.neighbors(k, out=(out_i.view(b, n, k), out_v.view(b, n, k)))
    assert got[0].data_ptr() == out_i.data_ptr() and got[1].data_ptr() == out_v.data_ptr()
    # the gather through the raw entry point, into an arena of its own
    from gym_d2d_amd import _native
    a_o, out_o = arena(b * n * 4 * (k + 1), torch.float32)
    t = env._t
    _native.graph_neighbor_obs(out_i.data_ptr(), out_v.data_ptr(), t['rb'].data_ptr(), t['pwr'].data_ptr(), t['sinr_db'].data_ptr(),
                               t['snr_db'].data_ptr(), b, n, k, out_o.data_ptr(), torch.cuda.current_stream(env.device).cuda_stream)
    torch.cuda.synchronize()
    for a in (a_c, a_i, a_v, a_o):
        host = a.cpu().numpy()
        assert (host[:pad] == guard).all() and (host[-pad:] == guard).all()
        assert (host[pad:-pad] != guard).all()                           # and every word inside was written
    assert np.array_equal(out_c.cpu().numpy().view(np.uint32), c['coupling'].reshape(-1).view(np.uint32))
    idx7 = out_i.cpu().numpy().reshape(b, n, k)
    nbu.check_indices(idx7, c['ref'], k)
    assert np.array_equal(idx7, c['lists'][8][0][:, :, :7])              # a shorter list is a prefix of a longer one
    want = nbu.gather_obs(idx7.astype(np.int64), out_v.cpu().numpy().reshape(b, n, k).astype(np.float64), c['rb'], c['pwr'],
                          c['step_sinr'], t['snr_db'].cpu().numpy())
    assert np.array_equal(out_o.cpu().numpy().reshape(b, n, -1), want.astype(np.float32))
    # an unaligned base (4 bytes past a 16-byte boundary) takes the dword stores: same bits, same bounds
    a_u = torch.full((b * n * n + 2 * pad + 1,), guard, dtype=torch.int32, device=env.device)
    out_u = a_u[pad + 1:pad + 1 + b * n * n].view(torch.float32).view(b, n, n)
    assert out_u.data_ptr() % 16 == 4
    env.coupling(out=out_u)
    host = a_u.cpu().numpy()
    assert (host[:pad + 1] == guard).all() and (host[-pad:] == guard).all()
    assert np.array_equal(host[pad + 1:-pad].view(np.uint32), c['coupling'].reshape(-1).view(np.uint32))
    # out= validation
    with pytest.raises(ValueError, match='out must be'):
        env.coupling(out=torch.empty((b, n, n + 1), device=env.device))
    with pytest.raises(ValueError, match='out must be'):
        env.coupling(out=torch.empty((b, n, n), dtype=torch.float64, device=env.device))
    with pytest.raises(ValueError, match='out must be'):
        env.coupling(out=torch.empty((b, n, 2 * n), device=env.device)[:, :, ::2])
    with pytest.raises(ValueError, match='out must be a pair'):
        env.neighbors(k, out=out_i.view(b, n, k))
    with pytest.raises(ValueError, match='int32'):
        env.neighbors(k, out=(out_v.view(b, n, k), out_v.view(b, n, k)))
    with pytest.raises(ValueError, match='out must be'):
        env.neighbors(k, out=(out_i.view(b, n, k), torch.empty((b, n, k + 1), device=env.device)))
    for bad in (0, n, 65, 2.0, True):
        with pytest.raises(ValueError, match='k must be an int in 1'):
            env.neighbors(bad)


def test_an_index_out_of_range_reads_nothing():
    from gym_d2d_amd import _native
    dev = torch.device('cuda', 0)
    b, n, k = 2, 5, 3
    idx = torch.tensor(np.random.default_rng(0).integers(0, n, (b, n, k)).astype(np.int32), device=dev)
    idx[0, 1, 2] = n; idx[1, 4, 0] = -1; idx[1, 0, 1] = 2 ** 31 - 1
    cdb = torch.arange(b * n * k, dtype=torch.float32, device=dev).view(b, n, k)
    rb = torch.arange(b * n, dtype=torch.int32, device=dev).view(b, n)
    pwr, sinr, snr = rb + 100, rb.float() + 0.5, rb.float() + 0.25
    out = torch.zeros((b, n, k + 1, 4), dtype=torch.float32, device=dev)
    _native.graph_neighbor_obs(idx.data_ptr(), cdb.data_ptr(), rb.data_ptr(), pwr.data_ptr(), sinr.data_ptr(), snr.data_ptr(), b, n, k,
                               out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.zeros((b, n, k), bool); bad[0, 1, 2] = bad[1, 4, 0] = bad[1, 0, 1] = True
    assert np.isnan(got[:, :, 1:, 1:][bad]).all() and np.isfinite(got[:, :, 1:, 1:][~bad]).all()
    assert np.array_equal(got[:, :, 1:, 0], cdb.cpu().numpy())
    ok_idx = np.where(bad, 0, idx.cpu().numpy())
    assert np.array_equal(got[:, :, 1:, 3][~bad], (sinr.cpu().numpy()[np.arange(b)[:, None, None], ok_idx])[~bad])


def test_unsupported_envs_are_refused_by_name(tmp_path):
    from gym_d2d_amd.envs import NeighborObsFunction, VecD2DEnv
    from gym_d2d_amd.path_loss import ArrayPathLoss, PathLoss, ShadowingPathLoss
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Foo(PathLoss):
        def __call__(self, tx, rx):
            return 20 * np.log10(tx.position.distance(rx.position)) + 40.0

    class Arr(ArrayPathLoss):
        def compute(self, view):
            return 20 * view.xp.log10(view.distance()) + 40.0

    class PerStep(Arr):
        per_step = True

    class TooMany(NeighborObsFunction):
        k = 6                                                            # N - 1 = 5

    class Two(NeighborObsFunction):
        k = 2

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            for call in (env.coupling, lambda: env.neighbors(2)):
                with pytest.raises(ValueError, match=text):
                    call()
        finally:
            env.close()
        with pytest.raises(ValueError, match=text):                      # at construction when the obs function asks
            VecD2DEnv(dict(small, obs_fn=Two, **(cfg or {})), num_envs=2, **kw)
    refused('export_actions', export_actions=False)
    refused('ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused("'link_table'", {'path_loss_model': Foo})
    refused("'array'", {'path_loss_model': Arr})
    refused("'per_step'", {'path_loss_model': PerStep})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused('float32 cannot hold', {'device_config_file': pinned})
    with pytest.raises(ValueError, match='k must be an int in 1'):
        VecD2DEnv(dict(small, obs_fn=TooMany), num_envs=2)
    with pytest.raises(ValueError, match='k must be an int in 1'):
        VecD2DEnv(dict(small, obs_fn=type('Zero', (NeighborObsFunction,), {'k': -1})), num_envs=2)
    env = VecD2DEnv(dict(small, path_loss_model=Foo), num_envs=1)        # one env: the per-object route of a single env
    try:
        env.reset(seed=1)
        with pytest.raises(ValueError, match="'device_table'"):
            env.neighbors(1)
    finally:
        env.close()


def test_numpy_path_matches_the_torch_path():
    from gym_d2d_amd.envs import NeighborObsFunction, VecD2DEnv
    cfg = {'num_rbs': 6, 'num_cues': 5, 'num_due_pairs': 7, 'obs_fn': NeighborObsFunction}
    a = VecD2DEnv(dict(cfg), num_envs=4, use_torch=True)
    b = VecD2DEnv(dict(cfg), num_envs=4, use_torch=False)
    try:
        oa, ob = a.reset(seed=4), b.reset(seed=4)
        assert isinstance(ob, np.ndarray) and ob.shape == (4, 12, 36)
        assert np.array_equal(oa.cpu().numpy().view(np.uint32), ob.view(np.uint32))
        ca, cb = a.coupling().cpu().numpy(), b.coupling()
        assert isinstance(cb, np.ndarray) and np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
        (ia, va), (ib, vb) = a.neighbors(3), b.neighbors(3)
        assert np.array_equal(ia.cpu().numpy(), ib) and np.array_equal(va.cpu().numpy().view(np.uint32), vb.view(np.uint32))
        out = (np.empty((4, 12, 3), np.int32), np.empty((4, 12, 3), np.float32))
        got = b.neighbors(3, out=out)
        assert got[0] is out[0] and got[1] is out[1] and np.array_equal(out[0], ib)
        with pytest.raises(ValueError, match='out must be'):
            b.coupling(out=np.empty((4, 12, 12), np.float64))
        acts = a.action_buffer().clone()
        oa, _, _, _ = a.step(acts)
        ob, _, _, _ = b.step(acts.cpu().numpy())
        assert np.array_equal(oa.cpu().numpy().view(np.uint32), ob.view(np.uint32))
    finally:
        a.close(); b.close()


def test_full_size_once():
    """4096 envs x 512 links, k = 8: idx in range and free of duplicates and of i itself everywhere, one env's rows against the oracle,
    the observation's own block against info everywhere, the device healthy afterwards; where 6 GiB are free also the 4.3 GB dense
    matrix, whose gather through idx is the lists' values bit for bit."""
    b, cues, dues, r, k = 4096, 256, 256, 256, 8
    env = _obs_env(False, b=b, cues=cues, dues=dues, r=r)
    try:
        n = cues + dues
        env.reset(seed=5)
        obs, _, _, info = env.step(env.action_buffer().clone())
        idx, cdb = env.neighbors(k)
        torch.cuda.synchronize()
        assert tuple(idx.shape) == (b, n, k) and int(idx.min()) >= 0 and int(idx.max()) < n
        s = idx.sort(dim=2).values
        assert bool((s[:, :, 1:] != s[:, :, :-1]).all())
        assert bool((idx != torch.arange(n, device=idx.device, dtype=torch.int32)[None, :, None]).all())
        assert bool(torch.isfinite(cdb).all()) and bool((cdb[:, :, 1:] <= cdb[:, :, :-1]).all())
        assert tuple(obs.shape) == (b, n, 36)
        o4 = obs.view(b, n, k + 1, 4)
        own = torch.stack([info['rb'].float(), info['tx_pwr_dbm'].float(), info['sinr_db'], info['snr_db']], dim=-1)
        assert torch.equal(o4[:, :, 0], own) and torch.equal(o4[:, :, 1:, 0], cdb)
        assert torch.equal(o4[:, :, 1:, 3], torch.gather(info['sinr_db'], 1, idx.long().view(b, n * k)).view(b, n, k))
        pick = 2717
        pos, _, _ = _state(env)
        cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
        ref = nbu.coupling_ref(pos[pick:pick + 1], env.simulator.link_tx, env.simulator.link_rx, cols, orc.PathLossSpec())
        left_out, _ = nbu.check_indices(idx[pick:pick + 1].cpu().numpy(), ref, k)
        e = rel_err(cdb[pick:pick + 1].cpu().numpy(), nbu.ranked(ref, k)[1])
        print(f'full size: env {pick} values vs the oracle rel_err {e:.3e}, {left_out:.2%} of its index entries left out')
        assert e <= BAR
        free, _ = torch.cuda.mem_get_info()
        if free >= 6 << 30:
            c = env.coupling()
            assert torch.equal(torch.gather(c, 2, idx.long()), cdb)
            e = rel_err(c[pick:pick + 1].cpu().numpy(), ref)
            print(f'full size: coupling() of env {pick} vs the oracle rel_err {e:.3e}; gather through idx equals the lists bit for bit')
            assert e <= BAR
        else:
            print(f'full size: {free >> 20} MiB free, the dense matrix was not built')
        torch.cuda.synchronize()
        assert env.status_flags() == 0
    finally:
        env.close()


def test_neighbor_obs_example_runs(capsys):
    res = runpy.run_path(str(ROOT / 'examples' / 'neighbor_obs.py'), run_name='__main__')
    out = capsys.readouterr().out
    print(out)
    assert res['obs_shape'][-1] == 4 * (res['k'] + 1) and 'strongest' in out

"""Difference rewards on the GPU (VecD2DEnv.marginal_capacity, DifferenceRewardFunction, csrc/d2d_marginal.hip) against the oracle.

The yardstick is the oracle's own step on the B0 * N envs in which one link sits on an RB of its own (marginal_util.leave_one_out),
which test_marginal_cpu.py ties to the reference at 1e-9; the bar is the project's 1e-5 (golden_util.rel_err: |d| <= 1e-5 max(|ref|,
1), Mbps) on BOTH planes.  Every entry is compared: the layouts come from sim_util.random_layout, which never places two interacting
devices on one point, and the cases are small enough that no link - and no victim on its RB, with or without the link - has an SINR
within twice the bar of its receiver's sensitivity threshold, where a capacity flips between 0 and its whole value and no bar-limited
comparison can call it (read_side_util.leave_one_out_direct's `decided`; asserted on the float64 reference of every case here, and for
the states that need no GPU to rebuild in test_marginal_cpu.py).

Measured on an MI355X (every test prints its rel_err): harm 3.5e-8 - 1.9e-7 and difference 8.9e-8 - 3.5e-7 over the nine cases,
1.8e-7 / 6.4e-7 at full size, 2.5 - 4.8e-7 against the simulator's own second step (CHANGELOG.md)."""
import json
import runpy
from pathlib import Path

import numpy as np
import pytest

import marginal_util as mu
import rb_sensing_util as rbs
import read_side_util as rsu
from golden_util import load_case, rel_err
from oracle import d2d_oracle as orc
from rb_sensing_util import _models, _state
from sim_util import env_config_for, oracle_spec, random_layout

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parent.parent
BAR = 1e-5


# rb_sensing_util.CASES - name: (B0, cues, due pairs, RBs, model, cue_actions, downlink traffic model) - and one_rb
CASES = dict(rbs.CASES, one_rb=(2, 20, 30, 1, 'ld2', 'agent', False))         # N^2 pairs, cancellation, the long sums
_cache = {}


def _build(name):
    """An env stepped once on a random_layout, its two planes, the step's capacity and the oracle's side - computed once per case."""
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
    diff, harm = (t.cpu().numpy() for t in env.marginal_capacity())
    pos, rb, pwr = _state(env)
    tx, rx = env.simulator.link_tx, env.simulator.link_rx
    ref_diff, ref_harm, ref_cap, _ = mu.leave_one_out(pos, tx, rx, rb, pwr, cols, spec, r)
    decided = rsu.leave_one_out_direct(dict(b=rb.shape[0], n=rb.shape[1], r=r, pos=pos, tx=tx, rx=rx, rb=rb, pwr=pwr, ocols=cols),
                                       pl=orc.pair_path_loss_db(spec, pos, np.asarray(tx), np.asarray(rx), cols))[3]
    out = dict(env=env, diff=diff, harm=harm, cap=info['capacity_mbps'].cpu().numpy(), pos=pos, rb=rb, pwr=pwr, tx=tx, rx=rx,
               cols=cols, spec=spec, r=r, ref_diff=ref_diff, ref_harm=ref_harm, ref_cap=ref_cap, decided=decided)
    assert env.status_flags() == 0
    _cache[name] = out
    return out


@pytest.fixture(scope='module', autouse=True)
def _close_envs():
    yield
    for c in _cache.values():
        c['env'].close()
    _cache.clear()


def _alone(rb, r):
    """[B, N] bool: the link is the only one on its RB (or on no RB at all)."""
    same = rb[:, :, None] == rb[:, None, :]
    return (same.sum(axis=2) == 1) | (rb < 0) | (rb >= r)


@pytest.mark.parametrize('name', list(CASES))
def test_both_planes_against_the_oracle(name):
    c = _build(name)
    assert c['harm'].shape == c['diff'].shape == c['ref_harm'].shape and c['harm'].dtype == c['diff'].dtype == np.float32
    assert np.isfinite(c['ref_harm']).all() and np.isfinite(c['harm']).all() and np.isfinite(c['diff']).all()
    e_h, e_d, e_c = rel_err(c['harm'], c['ref_harm']), rel_err(c['diff'], c['ref_diff']), rel_err(c['cap'], c['ref_cap'])
    print(f'{name}: harm rel_err {e_h:.3e}, difference rel_err {e_d:.3e} (the step capacity itself: {e_c:.3e}) over '
          f'{c["harm"].size} links; harm up to {c["ref_harm"].max():.3f} Mbps, negative difference for {(c["ref_diff"] < 0).mean():.1%}')
    assert c['decided'].all()        # on the float64 reference: no link within the bar of a sensitivity threshold, so every entry counts
    assert e_h <= BAR
    assert e_d <= BAR
    assert (c['harm'] >= 0.0).all()
    if name == 'one_rb':
        assert (c['ref_harm'] > 0).all()
    if name.startswith('empty'):
        assert _alone(c['rb'], c['r']).mean() > 0.3


@pytest.mark.parametrize('name', list(CASES))
def test_identities_hold_bit_for_bit(name):
    c = _build(name)
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(c['diff']), bits(c['cap'] - c['harm']))             # capacity: the step's plane
    alone = _alone(c['rb'], c['r'])
    print(f'{name}: {alone.mean():.1%} of the links alone on their RB')
    assert (c['harm'][alone] == 0.0).all() and not np.signbit(c['harm'][alone]).any()
    assert np.array_equal(bits(c['diff'][alone]), bits(c['cap'][alone]))


def test_two_calls_are_bit_identical_and_out_is_honoured_inside_guard_words():
    c = _build('mid_ld35_agent')
    env = c['env']
    b, n = c['harm'].shape
    d2, h2 = env.marginal_capacity()
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), c['diff'].view(np.uint32))
    assert np.array_equal(h2.cpu().numpy().view(np.uint32), c['harm'].view(np.uint32))
    d3, h3 = env.marginal_capacity()
    assert d3 is d2 and h3 is h2                                         # the env's one pair, reused
    guard, pad, words = 0x5AFEC0DE, 64, b * n
    arena = torch.full((2 * words + 3 * pad,), guard, dtype=torch.int32, device=env.device)
    od = arena[pad:pad + words].view(torch.float32).view(b, n)
    oh = arena[2 * pad + words:2 * pad + 2 * words].view(torch.float32).view(b, n)
    got = env.marginal_capacity(out=(od, oh))
    assert got[0] is od and got[1] is oh
    host = arena.cpu().numpy()
    assert (host[:pad] == guard).all() and (host[pad + words:2 * pad + words] == guard).all() and (host[2 * pad + 2 * words:] == guard).all()
    assert np.array_equal(host[pad:pad + words].view(np.uint32), c['diff'].reshape(-1).view(np.uint32))
    assert np.array_equal(host[2 * pad + words:2 * pad + 2 * words].view(np.uint32), c['harm'].reshape(-1).view(np.uint32))
    for bad in ((od, od), (od,), od, (od, torch.empty((b, n + 1), device=env.device)), (od, oh.double())):
        with pytest.raises(ValueError, match='out must be'):
            env.marginal_capacity(out=bad)


@pytest.mark.parametrize('n_rbs', [1, 5, 36])
def test_rb_values_out_of_range_are_on_no_rb_and_write_nothing_out_of_bounds(n_rbs):
    """Through the raw entry point: links whose rb is outside [0, R) harm nobody and nobody harms them - harm == 0.0, difference ==
    their capacity alone, the same bits a launch gives in which each of them has a real RB of its own - and the words around both
    outputs stay as they were."""
    from gym_d2d_amd import _native
    from gym_d2d_amd.marginal import fold_capacity_columns
    from gym_d2d_amd.sensing import fold_columns
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(n_rbs)
    b, cues, dues = 3, 7, 30
    n, d = cues + dues, 1 + cues + 2 * dues
    pos = random_layout(rng, b, cues, dues)
    tx = np.array(list(range(1, 1 + cues)) + [1 + cues + 2 * k for k in range(dues)], dtype=np.int32)
    rx = np.array([0] * cues + [2 + cues + 2 * k for k in range(dues)], dtype=np.int32)
    rb = rng.integers(0, n_rbs, (b, n)).astype(np.int32)
    bad = rng.random((b, n)) < 0.3
    rb[bad] = rng.choice([-1, -7, n_rbs, n_rbs + 1, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    pwr = rng.integers(0, 20, (b, n)).astype(np.int32)
    ocols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    law = {'a_tx_db': np.full(d, orc.pl_constant_db(2.1, 2.0)), 'a_rx_db': np.zeros(d), 'exponent': np.full(d, 2.0)}
    budget = {'eirp_off_db': ocols.eirp_off_db, 'rx_off_db': ocols.rx_off_db, 'noise_dbm': ocols.noise_dbm, 'bw_hz': ocols.bw_hz,
              'sens_dbm': ocols.sens_dbm}
    cols, kind, k = fold_columns(budget, law, tx)
    cap_cols = fold_capacity_columns(budget)
    guard, pad, words = 0x5AFEC0DE, 64, b * n
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(rb_plane, r):
        t = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (pos[..., 0].astype(np.float32), pos[..., 1].astype(np.float32),
                                                                              rb_plane, pwr, tx, rx, cols, cap_cols)]
        arena = torch.full((2 * words + 3 * pad,), guard, dtype=torch.int32, device=dev)
        _native.marginal_capacity(*(x.data_ptr() for x in t), kind, k, b, d, n, r, arena.data_ptr() + 4 * pad,
                                  arena.data_ptr() + 4 * (2 * pad + words), stream)
        torch.cuda.synchronize()                                        # raises if the device faulted
        host = arena.cpu().numpy()
        assert (host[:pad] == guard).all() and (host[pad + words:2 * pad + words] == guard).all() and (host[2 * pad + 2 * words:] == guard).all()
        return (host[pad:pad + words].view(np.float32).reshape(b, n), host[2 * pad + words:2 * pad + 2 * words].view(np.float32).reshape(b, n))
    harm, diff = run(rb, n_rbs)
    ref_diff, ref_harm, ref_cap, _ = mu.leave_one_out(pos, tx, rx, rb, pwr, ocols, orc.PathLossSpec(), n_rbs)
    assert (harm[bad] == 0.0).all()
    assert rel_err(diff[bad], ref_cap[bad]) <= BAR
    assert rel_err(harm, ref_harm) <= BAR and rel_err(diff, ref_diff) <= BAR
    own = rb.copy()
    own[bad] = np.broadcast_to(n_rbs + np.arange(n, dtype=np.int32), rb.shape)[bad]     # a real RB of its own for each of them
    harm2, diff2 = run(own, n_rbs + n)
    assert np.array_equal(harm.view(np.uint32), harm2.view(np.uint32)) and np.array_equal(diff.view(np.uint32), diff2.view(np.uint32))


def test_against_the_simulator_itself_with_the_link_parked_on_an_unused_rb():
    """No oracle: the definition executed on the GPU.  One link per env moves to an RB nobody uses, the env is stepped again, and what
    the OTHER links' capacities gained is that link's harm."""
    from gym_d2d_amd.envs import VecD2DEnv
    b, cues, dues, r = 8, 10, 22, 6
    n, spare = cues + dues, r - 1
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b)
    try:
        rng = np.random.default_rng(17)
        env.reset(seed=4)
        levels = np.array([env.num_pwr_actions['cue']] * cues + [env.num_pwr_actions['due']] * dues)
        rb = rng.integers(0, spare, (b, n)); lvl = rng.integers(0, levels, (b, n))
        _, _, _, info = env.step(torch.as_tensor((rb * levels + lvl).astype(np.int32), device=env.device))
        cap = info['capacity_mbps'].cpu().numpy().astype(np.float64)
        diff, harm = (t.cpu().numpy() for t in env.marginal_capacity())
        assert np.array_equal(info['rb'].cpu().numpy(), rb)
        worst = 0.0
        for trial in range(3):                                           # 3 x 8 links
            pick = rng.integers(0, n, b)
            rb2 = rb.copy(); rb2[np.arange(b), pick] = spare
            _, _, _, info2 = env.step(torch.as_tensor((rb2 * levels + lvl).astype(np.int32), device=env.device))
            cap2 = info2['capacity_mbps'].cpu().numpy().astype(np.float64)
            others = np.ones((b, n), bool); others[np.arange(b), pick] = False
            ref_harm = ((cap2 - cap) * others).sum(axis=1)               # G without link i - (G - cap_i), over the others
            got_h, got_d = harm[np.arange(b), pick], diff[np.arange(b), pick]
            ref_d = cap[np.arange(b), pick] - ref_harm
            e_h, e_d = rel_err(got_h, ref_harm), rel_err(got_d, ref_d)
            print(f'trial {trial}: links {pick.tolist()} parked on RB {spare}: harm rel_err {e_h:.3e}, difference rel_err {e_d:.3e}, '
                  f'harm up to {ref_harm.max():.3f} Mbps')
            worst = max(worst, e_h, e_d)
            assert e_h <= BAR and e_d <= BAR
        assert env.status_flags() == 0
    finally:
        env.close()


def test_full_size_once():
    """4096 envs x 512 links x 256 RBs: the identities on all 2.1 M links, harm >= -1e-5 everywhere, and the oracle yardstick on
    every link of 8 envs (first, last, six drawn)."""
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import SignalPlanesObsFunction
    b, cues, dues, r = 4096, 256, 256, 256
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'obs_fn': SignalPlanesObsFunction}, num_envs=b)
    try:
        rng = np.random.default_rng(11)
        env.reset(seed=5)             # the device-side sampler's layout (reset() raises on a zero distance); random actions
        _, _, _, info = env.step(env.action_buffer().clone())
        diff, harm = env.marginal_capacity()
        cap, rb = info['capacity_mbps'], info['rb'].long()
        assert tuple(diff.shape) == tuple(harm.shape) == (b, n) and bool(torch.isfinite(diff).all()) and bool(torch.isfinite(harm).all())
        assert torch.equal(diff, cap - harm)
        counts = torch.zeros((b, r), dtype=torch.int64, device=env.device).scatter_add_(1, rb, torch.ones_like(rb))
        alone = counts.gather(1, rb) == 1
        assert bool((harm[alone] == 0.0).all()) and torch.equal(diff[alone], cap[alone])
        low = float(harm.min())
        print(f'full size: identities hold on {diff.numel()} links, {float(alone.float().mean()):.1%} alone on their RB; min harm {low:.3e}, '
              f'max harm {float(harm.max()):.3f} Mbps; negative difference for {float((diff < 0).float().mean()):.1%}')
        assert low >= -1e-5
        picks = np.concatenate([[0], np.sort(rng.choice(np.arange(1, b - 1), 6, replace=False)), [b - 1]])
        pos, rb_h, pwr = _state(env)
        cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
        tx, rx = env.simulator.link_tx, env.simulator.link_rx
        ref_diff, ref_harm, _, _ = mu.leave_one_out(pos[picks], tx, rx, rb_h[picks], pwr[picks], cols, orc.PathLossSpec(), r)
        sel = torch.as_tensor(picks, device=env.device)
        e_h, e_d = rel_err(harm[sel].cpu().numpy(), ref_harm), rel_err(diff[sel].cpu().numpy(), ref_diff)
        print(f'full size: envs {picks.tolist()} vs the oracle: harm rel_err {e_h:.3e}, difference rel_err {e_d:.3e}')
        assert e_h <= BAR and e_d <= BAR
        assert env.status_flags() == 0
    finally:
        env.close()


@pytest.mark.parametrize('autoreset', [False, True])
def test_difference_reward_function_through_step(autoreset):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import DifferenceRewardFunction, VecD2DEnv
    b, cues, dues, r = 16, 6, 10, 4
    cfg = {'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'reward_fn': DifferenceRewardFunction}
    env = VecD2DEnv(cfg, num_envs=b, autoreset=autoreset)
    try:
        kw = {'elapsed': np.arange(b) % 10} if autoreset else {}
        before = _native.marginal_launches
        env.reset(seed=9, **kw)
        assert _native.marginal_launches == before                      # the reset returns no reward: nothing to launch
        rng = np.random.default_rng(2)
        resets, negative = 0, 0
        by_hand = tuple(torch.empty((b, cues + dues), device=env.device) for _ in range(2))
        for step in range(12):
            a = torch.as_tensor(rng.integers(0, r * 21, (b, cues + dues)).astype(np.int32), device=env.device)
            _, rewards, _, info = env.step(a)
            assert _native.marginal_launches == before + step + 1       # one launch per step
            rewards = rewards.clone()
            assert tuple(rewards.shape) == (b, cues + dues) and rewards.dtype == torch.float32
            diff, harm = env.marginal_capacity(out=by_hand)
            before += 1
            assert torch.equal(diff, info['capacity_mbps'] - harm)
            if autoreset:
                was_reset = info['reset']
                assert bool((rewards[was_reset] == 0.0).all())           # the existing rule: a reset env's reward is 0
                assert torch.equal(rewards[~was_reset], diff[~was_reset])
                resets += int(was_reset.sum())
            else:
                assert torch.equal(rewards, diff)
            negative += int((diff < 0).sum())
        assert negative > 0 and (not autoreset or resets >= b)
    finally:
        env.close()
    with pytest.raises(ValueError, match='reward_per_env'):
        VecD2DEnv(dict(cfg), num_envs=2, reward_per_env=True)


def test_user_reward_and_obs_functions_with_needs_marginal_see_both_planes():
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import ArrayObsFunction
    from gym_d2d_amd.spaces import Box
    seen = {}

    class HarmOnly:
        needs_marginal = True

        def compute(self, view):
            seen['reward'] = (view.difference_mbps, view.harm_mbps)
            return -view.harm_mbps

    class MarginalObs(ArrayObsFunction):
        native_mode = _native.OBS_NONE
        needs_marginal = True

        def get_obs_space(self, env_config):
            return Box(low=-np.inf, high=np.inf, shape=(2,))

        def compute(self, view):
            return torch.stack([view.difference_mbps, view.harm_mbps], dim=2)
    env = VecD2DEnv({'num_rbs': 3, 'num_cues': 4, 'num_due_pairs': 4, 'obs_fn': MarginalObs, 'reward_fn': HarmOnly}, num_envs=5)
    try:
        before = _native.marginal_launches
        obs = env.reset(seed=2)
        assert _native.marginal_launches == before + 1                  # the obs function asks at reset too
        assert tuple(obs.shape) == (5, 8, 2)
        cached = env._view()
        assert not hasattr(cached, 'difference_mbps') and not hasattr(cached, 'harm_mbps')     # the cached view is untouched
        obs, rewards, _, info = env.step(env.action_buffer().clone())
        assert _native.marginal_launches == before + 2                  # ONE launch serves both functions
        obs, rewards = obs.clone(), rewards.clone()
        diff, harm = env.marginal_capacity()
        assert torch.equal(obs[:, :, 0], diff) and torch.equal(obs[:, :, 1], harm) and torch.equal(rewards, -harm)
        assert seen['reward'][0] is diff and seen['reward'][1] is harm
        assert bool((harm > 0).any())
    finally:
        env.close()


def test_existing_reward_and_obs_functions_launch_no_marginal_kernel():
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import DifferenceRewardFunction, VecD2DEnv
    from gym_d2d_amd.envs.obs_fn import LinearObsFunction, OwnLinkObsFunction, SignalPlanesObsFunction
    from gym_d2d_amd.envs.reward_fn import CueSinrShannonRewardFunction, ShannonRewardFunction, SystemCapacityRewardFunction
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    def launches(**kw):
        cfg = {k: kw.pop(k) for k in ('obs_fn', 'reward_fn') if k in kw}
        before = _native.marginal_launches
        env = VecD2DEnv(dict(small, **cfg), num_envs=4, **kw)
        try:
            env.reset(seed=1)
            for _ in range(3):
                env.step(env.action_buffer().clone())
            assert (env._marginal is None) == (cfg.get('reward_fn') is not DifferenceRewardFunction)
        finally:
            env.close()
        return _native.marginal_launches - before
    for fn in (LinearObsFunction, OwnLinkObsFunction, SignalPlanesObsFunction):
        assert launches(obs_fn=fn) == 0
        assert launches(obs_fn=fn, autoreset=True) == 0
    for fn in (SystemCapacityRewardFunction, ShannonRewardFunction, CueSinrShannonRewardFunction):
        assert launches(reward_fn=fn) == 0
        assert launches(reward_fn=fn, autoreset=True) == 0
    assert launches(reward_fn=DifferenceRewardFunction) == 3            # three steps; the reset returns no reward
    assert launches(reward_fn=DifferenceRewardFunction, autoreset=True) == 3


def test_numpy_path_matches_the_torch_path():
    from gym_d2d_amd.envs import VecD2DEnv
    cfg = {'num_rbs': 3, 'num_cues': 5, 'num_due_pairs': 7}
    a = VecD2DEnv(dict(cfg), num_envs=4, use_torch=True)
    b = VecD2DEnv(dict(cfg), num_envs=4, use_torch=False)
    try:
        a.reset(seed=4); b.reset(seed=4)
        da, ha = (t.cpu().numpy() for t in a.marginal_capacity())
        db, hb = b.marginal_capacity()
        assert isinstance(db, np.ndarray) and db.shape == hb.shape == (4, 12) and db.dtype == np.float32
        assert np.array_equal(da.view(np.uint32), db.view(np.uint32)) and np.array_equal(ha.view(np.uint32), hb.view(np.uint32))
        assert (ha > 0).any()
        out = (np.empty((4, 12), dtype=np.float32), np.empty((4, 12), dtype=np.float32))
        got = b.marginal_capacity(out=out)
        assert got[0] is out[0] and got[1] is out[1]
        assert np.array_equal(out[0].view(np.uint32), da.view(np.uint32)) and np.array_equal(out[1].view(np.uint32), ha.view(np.uint32))
        with pytest.raises(ValueError, match='out must be'):
            b.marginal_capacity(out=(out[0], out[0]))
    finally:
        a.close(); b.close()


def test_unsupported_routes_are_refused_by_name(tmp_path):
    from gym_d2d_amd.envs import DifferenceRewardFunction, VecD2DEnv
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

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            with pytest.raises(ValueError, match=text):
                env.marginal_capacity()
        finally:
            env.close()
    refused('marginal_capacity.*export_actions', export_actions=False)
    refused('marginal_capacity.*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused("marginal_capacity.*'link_table'", {'path_loss_model': Foo})
    refused("'array'", {'path_loss_model': Arr})
    refused("'per_step'", {'path_loss_model': PerStep})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused('float32 cannot hold', {'device_config_file': pinned})
    with pytest.raises(ValueError, match='export_actions'):              # at construction, not inside the first step
        VecD2DEnv(dict(small, reward_fn=DifferenceRewardFunction), num_envs=2, export_actions=False)


def test_difference_reward_example_checks_itself(capsys):
    res = runpy.run_path(str(ROOT / 'examples' / 'difference_reward.py'), run_name='__main__')
    out = capsys.readouterr().out
    print(out)
    assert res['self_check_error'] <= 1e-4 and 'self-check' in out and 'MISMATCH' not in out
    assert 0.0 < res['negative_share'] < 1.0
    assert 'capacity' in out and 'harm' in out and 'difference' in out

"""CPU-only tests of the env front-ends' HOST logic (key parsing, action decode, link typing, plugin lowering,
traffic-model actions, error types) with the C-ABI handle replaced by a recording stub.  The stub computes nothing:
numbers are checked by the -m gpu tests; here only what the host hands to the boundary is."""
import json
import math
import random
from unittest.mock import ANY

import numpy as np
import pytest

from gym_d2d_amd import _native
from gym_d2d_amd.path_loss import ArrayPathLoss, PathLoss


class RecordingHandle:
    """Stands in for _native.Handle: remembers every call, returns zeros for downloads."""
    instances = []

    def __init__(self, **kw):
        self.kw = kw
        self.num_envs = kw['num_envs']
        self.num_devices = 1 + kw['num_cues'] + 2 * kw['num_due_pairs']
        self.max_links = kw.get('max_links') or (kw['num_cues'] + kw['num_due_pairs'])
        self.num_links = 0
        self.num_fixed = 0
        self.env_offset = 0
        self.calls = []
        self.uploads = {}
        RecordingHandle.instances.append(self)

    def _rec(self, name, *args):
        self.calls.append((name, args))

    def set_device_table(self, *cols): self._rec('device_table', *[np.asarray(c) for c in cols])
    def set_path_loss_power_law(self, a, b, e): self._rec('power_law', np.asarray(a), np.asarray(b), np.asarray(e))
    def set_path_loss_shadowing(self, a, b, e, d0, chi, seed): self._rec('shadowing', d0, chi, seed)
    def set_path_loss_table(self, t): self._rec('table', np.asarray(t))
    def set_path_loss_link_table(self, t): self._rec('link_table', np.asarray(t))
    def set_reward(self, rid, param=0.0): self._rec('reward', rid, param)
    def set_obs_mode(self, m): self._rec('obs_mode', m)
    def set_export_actions(self, on): self._rec('export_actions', on)
    def set_stream(self, p): self._rec('stream', p)
    def synchronize(self): self._rec('synchronize')

    def set_env_offset(self, k):
        self.env_offset = int(k)
        self._rec('env_offset', k)
    def reset_positions(self, seed, episode=0, mask=None, xy=None): self._rec('reset', seed, episode, mask, xy)
    def set_positions(self, x, y, env_begin=0): self._rec('positions', np.asarray(x), np.asarray(y))
    def status_flags(self): return 0
    def close(self): self._rec('close')

    def set_links(self, tx, rx, ty):
        self.num_links = len(tx)
        self._rec('links', list(tx), list(rx), list(ty))

    def upload(self, which, array, offset_bytes=0):
        self.uploads[which] = np.array(array)

    def step(self, ptr=0): self._rec('step', ptr)
    def step_rb_pwr(self, a=0, b=0): self._rec('step_rb_pwr')
    def positions_changed(self): self._rec('positions_changed')

    def set_fixed_actions(self, idx, rb, pwr):
        self.num_fixed = len(idx)
        self._rec('fixed_actions', list(idx), list(rb), list(pwr))

    def step_host(self, rb, pwr):
        """d2d_step_host: (rb, pwr) in, every result in one block out - zeros here, with rb/pwr echoed."""
        self.uploads[_native.BUF_RB] = np.array(rb); self.uploads[_native.BUF_PWR] = np.array(pwr)
        self._rec('step_host')
        b, n = self.num_envs, self.num_links
        res = {k: np.zeros((b, n), np.float32) for k in ('sinr_db', 'snr_db', 'rate_bps', 'capacity', 'reward')}
        res.update(rb=np.array(rb, np.int32), pwr=np.array(pwr, np.int32), obs_table=np.zeros((b, n, 6), np.float32),
                   env_flags=np.zeros(b, np.int32), obs=np.zeros((b, n, 6 * n), np.float32))
        return res

    def download(self, which, env_begin=0, env_count=None):
        b, n, d = (env_count or self.num_envs), self.num_links, self.num_devices
        shape = {_native.BUF_POS_X: (b, d), _native.BUF_POS_Y: (b, d), _native.BUF_OBS_TABLE: (b, n, 6),
                 _native.BUF_OBS: (b, n, 6 * n), _native.BUF_ENV_FLAGS: (b,)}.get(which, (b, n))
        dtype = np.int32 if which in (_native.BUF_RB, _native.BUF_PWR) else np.float32
        if which in self.uploads and self.uploads[which].shape == shape:
            return self.uploads[which].astype(dtype)
        return np.zeros(shape, dtype=dtype)

    def last(self, name):
        return [args for n, args in self.calls if n == name][-1]


@pytest.fixture
def stub(monkeypatch):
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    return RecordingHandle


def test_env_construction_lowers_config_to_tables(stub):
    from gym_d2d_amd.envs import D2DEnv
    env = D2DEnv({'num_rbs': 6, 'num_cues': 3, 'num_due_pairs': 2})
    h = stub.instances[-1]
    assert h.kw['pwr_levels_due'] == 21 and h.kw['pwr_levels_cue'] == 24 and h.kw['pwr_levels_mbs'] == 47
    assert h.kw['max_links'] == 2 * 3 + 2                   # every uplink, downlink and sidelink at once
    eirp, rxo, noise, sens, bw = h.last('device_table')
    assert list(eirp) == [15.5] + [-6.0] * 7 and list(rxo) == [17.5] + [-3.0] * 7      # SURVEY 8(a) closed form
    assert list(noise) == [-118.4] + [-104.5] * 7 and list(bw) == [180000.0] * 8
    a_tx, a_rx, ple = h.last('power_law')
    assert a_tx[0] == pytest.approx(38.892169116561746) and (a_rx == 0).all() and (ple == 2.0).all()
    assert h.last('obs_mode') == (_native.OBS_LINEAR,) and h.last('reward') == (_native.REWARD_SYSTEM_CAPACITY, 0.0)
    assert env.action_space['due'].n == 6 * 21 and env.action_space['cue'].n == 6 * 24 and env.action_space['mbs'].n == 6 * 47
    assert env.observation_space.shape == (6 * 5,)
    assert env.num_steps == 0 and env.actions is None and env.state is None


def test_step_parses_keys_types_links_and_decodes(stub):
    from gym_d2d_amd.envs import D2DEnv
    from gym_d2d_amd.link_type import LinkType
    env = D2DEnv({'num_rbs': 6, 'num_cues': 3, 'num_due_pairs': 2})
    h = stub.instances[-1]
    raw = {'due02:due03': 5 * 21 + 20, 'cue01:mbs': 2 * 24 + 23, 'mbs:cue00': np.int64(4 * 47 + 46),
           'due00:due01': np.array([[3], [7]])}
    obs, rewards, done, info = env.step(raw)
    # agent order = dict order; device indices follow devices.py:20-25 (mbs, cues, due tx/rx interleaved)
    assert h.last('links') == ([6, 2, 0, 4], [7, 0, 1, 5], [3, 1, 2, 3])
    assert h.uploads[_native.BUF_RB].tolist() == [[5, 2, 4, 3]] and h.uploads[_native.BUF_PWR].tolist() == [[20, 23, 46, 7]]
    assert [a.link_type for a in env.actions.values()] == [LinkType.SIDELINK, LinkType.UPLINK, LinkType.DOWNLINK, LinkType.SIDELINK]
    assert list(obs) == list(raw) == list(rewards) == list(info) and obs['cue01:mbs'].shape == (24,)
    assert info['mbs:cue00']['rb'] == 4 and info['mbs:cue00']['tx_pwr_dbm'] == 46 and isinstance(info['mbs:cue00']['rb'], int)
    assert done == {'__all__': False} and env.num_steps == 1
    for _ in range(9):
        _, _, done, _ = env.step(raw)
    assert done == {'__all__': True}                       # EPISODE_LENGTH = 10 (d2d_env.py:16,68)
    n_link_uploads = sum(1 for n, _ in h.calls if n == 'links')
    assert n_link_uploads == 1                             # same link set: the table is not re-sent
    env.step({'cue01:mbs': 3})
    assert h.last('links') == ([2], [0], [1])


def test_step_error_types_match_reference(stub):
    from gym_d2d_amd.envs import D2DEnv
    env = D2DEnv({'num_cues': 2, 'num_due_pairs': 1})
    with pytest.raises(ZeroDivisionError):
        env.step({})                                       # reward_fn.py:42
    with pytest.raises(TypeError):
        env.step({'cue00': 1})                             # d2d_env.py:76-77: key must split into exactly two ids
    with pytest.raises(TypeError):
        env.step({'a:b:c': 1})
    with pytest.raises(KeyError):
        env.step({'cue00:ghost': 1})                       # devices.py:28
    with pytest.raises(ValueError, match='Unable to decode action type'):
        env.step({'cue00:mbs': '7'})                       # d2d_env.py:100
    with pytest.raises(ValueError, match='Unable to decode action type'):
        env.step({'cue00:mbs': np.array([1, 2])})          # ndarray must have ndim == 2
    with pytest.raises(TypeError):
        D2DEnv({'num_cue': 2})                             # unknown config key (dataclass)
    with pytest.raises(ValueError):
        D2DEnv({'num_envs': 4})                            # batches go through VecD2DEnv


def test_reset_draws_positions_then_steps_with_all_links(stub):
    from gym_d2d_amd.envs import D2DEnv
    env = D2DEnv({'num_cues': 2, 'num_due_pairs': 2, 'cell_radius_m': 100.0, 'd2d_radius_m': 5.0})
    h = stub.instances[-1]
    obs = env.reset()
    assert list(obs) == ['cue00:mbs', 'cue01:mbs', 'due00:due01', 'due02:due03']       # d2d_env.py:54-60
    x, y = h.last('positions')
    assert x.shape == (1, 7) and x.dtype == np.float64 and x[0, 0] == 0 and y[0, 0] == 0      # the reference's precision (position.py:7-12)
    assert (np.hypot(x, y) <= 100.0 + 1e-3).all()
    assert np.hypot(x[0, 3] - x[0, 4], y[0, 3] - y[0, 4]) <= 5.0 + 1e-3
    devs = list(env.simulator.devices.values())
    assert [d.position.x for d in devs] == [float(v) for v in x[0]]        # objects hold what the GPU is given (hi + lo pairs)
    assert any(float(np.float32(v)) != v for v in x[0, 1:])                # ... and that is NOT rounded to float32
    rb, pw = h.uploads[_native.BUF_RB][0], h.uploads[_native.BUF_PWR][0]
    assert (rb >= 0).all() and (rb < 25).all() and (pw[:2] <= 23).all() and (pw[2:] <= 20).all()


def test_plugin_lowering_choices(stub):
    from gym_d2d_amd.envs import D2DEnv
    from gym_d2d_amd.envs.obs_fn import LinearObsFunction, ObsFunction
    from gym_d2d_amd.envs.reward_fn import CueSinrShannonRewardFunction, RewardFunction, ShannonRewardFunction
    from gym_d2d_amd.path_loss import AreaType, CostHataPathLoss, PathLoss, ShadowingPathLoss
    from gym_d2d_amd.spaces import Box

    D2DEnv({'reward_fn': ShannonRewardFunction})
    assert stub.instances[-1].last('reward') == (_native.REWARD_SHANNON, -70.0)

    class Cue3(CueSinrShannonRewardFunction):
        def __init__(self):
            super().__init__(sinr_threshold_dB=3.0)
    D2DEnv({'reward_fn': Cue3})
    assert stub.instances[-1].last('reward') == (_native.REWARD_CUE_SINR_SHANNON, 3.0)

    class PyReward(RewardFunction):
        def __call__(self, actions, state):
            return {':'.join(k): 0.0 for k in actions}
    D2DEnv({'reward_fn': PyReward})
    assert stub.instances[-1].last('reward') == (_native.REWARD_NONE, 0.0)

    class PyObs(ObsFunction):
        def get_obs_space(self, cfg):
            return Box(-1, 1, shape=(1,))

        def get_state(self, actions, state, devices):
            return {}
    D2DEnv({'obs_fn': PyObs})
    assert stub.instances[-1].last('obs_mode') == (_native.OBS_TABLE,)

    class OverriddenLinear(LinearObsFunction):
        def get_state(self, actions, state, devices):
            return {}
    D2DEnv({'obs_fn': OverriddenLinear})
    assert stub.instances[-1].last('obs_mode') == (_native.OBS_TABLE,)       # overridden -> Python, not the kernel

    D2DEnv({'path_loss_model': CostHataPathLoss})
    a_tx, a_rx, expo = stub.instances[-1].last('power_law')
    assert expo[0] != expo[1] and a_rx[0] != a_rx[1]                            # per-device heights: BS 23 m vs UE 1.5 m

    D2DEnv({'path_loss_model': ShadowingPathLoss, 'seed': 11})
    assert stub.instances[-1].last('shadowing') == (100.0, 2.7, 11)

    class Custom(PathLoss):
        def __call__(self, tx, rx):
            return 100.0
    env = D2DEnv({'path_loss_model': Custom, 'num_cues': 1, 'num_due_pairs': 1})
    assert not any(n in ('power_law', 'shadowing') for n, _ in stub.instances[-1].calls)
    env.reset()
    table, = stub.instances[-1].last('table')
    # only (transmitter of a link) x (receiver of a link) pairs are evaluated: cue00 -> mbs, due00 -> due01 and their cross terms
    assert table.shape == (4, 4) and table.dtype == np.float64 and np.isnan(table[0, 0])
    assert table[1, 0] == 100.0 and table[2, 3] == 100.0 and table[1, 3] == 100.0 and table[2, 0] == 100.0
    assert np.isnan(table[0, 1]) and np.isnan(table[3, 2])                     # the BS / a DUE receiver never transmit here
    # a changed link list (downlink mbs -> cue00) adds the pairs it needs, keeps the rest
    calls = []
    orig = Custom.__call__
    Custom.__call__ = lambda self, tx, rx: (calls.append((tx.id, rx.id)), 100.0)[1]
    env.step({'mbs:cue00': 3, 'due00:due01': 5})
    Custom.__call__ = orig
    table, = stub.instances[-1].last('table')
    assert table[0, 1] == 100.0 and table[0, 3] == 100.0 and table[2, 1] == 100.0 and table[1, 0] == 100.0


def test_save_device_config_format(stub, tmp_path):
    from gym_d2d_amd.envs import D2DEnv
    env = D2DEnv({'num_cues': 1, 'num_due_pairs': 1})
    env.reset()
    path = tmp_path / 'cfg.json'
    env.save_device_config(path)
    data = json.loads(path.read_text())
    assert list(data) == ['mbs', 'cue00', 'due00', 'due01']
    assert data['mbs']['position'] == [0, 0] and data['cue00']['config']['max_tx_power_dBm'] == 23
    assert data['due01']['config']['body_loss_dB'] == 3.0 and len(data['due00']['position']) == 2


def test_vec_env_host_side(stub):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2, 'seed': 5}, num_envs=6, cue_actions='traffic',
                    use_torch=False, first_env=12)
    h = stub.instances[-1]
    assert h.kw['max_links'] == 5 and h.last('env_offset') == (12,)
    assert h.last('links') == ([1, 2, 3, 4, 6], [0, 0, 0, 5, 7], [1, 1, 1, 3, 3])
    env.reset()
    assert h.last('reset')[:2] == (5, 0)
    env.reset()
    assert h.last('reset')[:2] == (5, 1)                   # next episode, same seed
    due = np.arange(12, dtype=np.int32).reshape(6, 2)
    obs, rew, dones, info = env.step(due)
    # CUE links from UplinkTrafficModel: rb = i mod R at the CUE's max power (traffic_model.py:15-22), handed over ONCE
    # as fixed (rb, pwr) of links 0..2 - the per-step action array carries the DUE columns only
    assert h.last('fixed_actions') == ([0, 1, 2], [0, 1, 2], [23, 23, 23])
    assert sum(1 for n, _ in h.calls if n == 'fixed_actions') == 1
    assert h.uploads[_native.BUF_ACTIONS].shape == (6, 2) and (h.uploads[_native.BUF_ACTIONS] == due).all()
    assert obs.shape == (6, 5, 30) and rew.shape == (6, 5) and dones.shape == (6,) and not dones.any()
    with pytest.raises(ValueError, match=r'\[6,2\]'):
        env.step(np.zeros((6, 5), dtype=np.int32))
    # DownlinkTrafficModel: the CUE links become mbs -> cueXX with the base station's power alphabet (47 levels)
    from gym_d2d_amd.traffic_model import DownlinkTrafficModel
    down = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2, 'traffic_model': DownlinkTrafficModel},
                     num_envs=2, cue_actions='traffic', use_torch=False)
    hd = stub.instances[-1]
    assert hd.last('links') == ([0, 0, 0, 4, 6], [1, 2, 3, 5, 7], [2, 2, 2, 3, 3])
    down.reset(seed=1)
    assert hd.last('fixed_actions') == ([0, 1, 2], [0, 1, 2], [23, 23, 23]) and hd.uploads[_native.BUF_ACTIONS].shape == (2, 2)
    # reset()'s random actions are keyed by global env index: a shard reproduces its slice of the unsharded batch
    whole = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=8, use_torch=False)
    whole.reset(seed=7)
    part = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=3, use_torch=False, first_env=5)
    part.reset(seed=7)
    a_whole, a_part = stub.instances[-2].uploads[_native.BUF_ACTIONS], stub.instances[-1].uploads[_native.BUF_ACTIONS]
    assert a_whole.shape == (8, 5) and (a_whole[5:8] == a_part).all()
    assert (a_whole[:, :3] < 4 * 24).all() and (a_whole[:, 3:] < 4 * 21).all() and len(np.unique(a_whole)) > 10
    with pytest.raises(ValueError):
        VecD2DEnv({}, num_envs=2, cue_actions='nope', use_torch=False)
    from gym_d2d_amd.envs.obs_fn import ObsFunction

    class DictObs(ObsFunction):
        def get_obs_space(self, cfg): return None
        def get_state(self, a, s, d): return {}
    with pytest.raises(TypeError):
        VecD2DEnv({'obs_fn': DictObs}, num_envs=2, use_torch=False)


# ---------------------------------------------------------------------------------------------- path-loss table routes
# What a Python PathLoss the kernels cannot evaluate hands to the handle, call by call, on every route that needs no GPU.

class _Plugin(PathLoss):
    """Deterministic and position-dependent; refuses a zero distance (math.log10(0)), as the reference's models do."""
    def __call__(self, tx, rx):
        return 30.0 + 31.0 * math.log10(tx.position.distance(rx.position)) - 0.5 * tx.tx_antenna_gain_dBi


class _ArrayPlugin(ArrayPathLoss):
    def compute(self, view):
        return 30.0 + 31.0 * view.xp.log10(view.distance()) - 0.5 * view.tx_column(lambda t: t.tx_antenna_gain_dBi)


class _ArrayPluginPerObject(PathLoss):
    """_ArrayPlugin's own per-object call, as a plain PathLoss."""
    def __call__(self, tx, rx):
        return _ArrayPlugin(self.carrier_freq_GHz)(tx, rx)


class _Gauss(PathLoss):
    def __call__(self, tx, rx):
        return 80.0 + random.gauss(0.0, 4.0)


class _GaussArray(ArrayPathLoss):
    def compute(self, view):
        return 80.0 + np.random.standard_normal(tuple(view.tx_x.shape) + (view.tx_x.shape[-1],))


_UPLINKS = [('cue00', 'mbs'), ('cue01', 'mbs'), ('due00', 'due01')]          # devices: mbs 0, cue00 1, cue01 2, due00 3, due01 4
_MIXED = [('mbs', 'cue00'), ('cue00', 'mbs'), ('due00', 'due01')]            # a downlink: mbs transmits, cue00 receives


def _sim(model, num_envs=1):
    from gym_d2d_amd.simulator import Simulator
    sim = Simulator({'num_rbs': 4, 'num_cues': 2, 'num_due_pairs': 1, 'num_envs': num_envs, 'path_loss_model': model})
    return sim, RecordingHandle.instances[-1]


def _pl(gains, xy, i, j):
    """_Plugin's value for device i -> device j at xy [D, 2], NaN where it refuses."""
    d = ((float(xy[i][0]) - float(xy[j][0])) ** 2 + (float(xy[i][1]) - float(xy[j][1])) ** 2) ** 0.5
    return 30.0 + 31.0 * math.log10(d) - 0.5 * gains[i] if d > 0 else np.nan


def _device_table(gains, xy, txs, rxs):
    out = np.full((len(gains), len(gains)), np.nan)
    for i in txs:
        for j in rxs:
            if i != j:
                out[i, j] = _pl(gains, xy, i, j)
    return out


def _link_table(gains, xy, tx, rx):
    return np.array([[[_pl(gains, xy[b], t, r) if t != r else np.nan for r in rx] for t in tx] for b in range(len(xy))])


def _assert_log(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, args), (_, expected) in zip(got, want):
        if expected is ANY:
            continue
        assert len(args) == len(expected), name
        for a, e in zip(args, expected):
            if isinstance(e, np.ndarray):
                a = np.asarray(a)
                assert a.dtype == e.dtype and a.shape == e.shape and np.array_equal(a, e, equal_nan=True), (name, a, e)
            else:
                assert a == e, name


def test_path_loss_device_table_route_is_incremental_over_link_changes(stub):
    """One env: a [D, D] table of the pairs the links read, topped up when a new link list reads more, evaluated afresh when the
    positions change; prepare_step() hands nothing over."""
    sim, h = _sim(_Plugin)
    gains = [d.tx_antenna_gain_dBi for d in sim.devices.values()]
    rng = np.random.default_rng(3)
    xy = rng.uniform(-300.0, 300.0, (1, 5, 2))
    xy32 = rng.uniform(-300.0, 300.0, (1, 5, 2)).astype(np.float32)
    sim.set_links(_UPLINKS)                          # no positions yet: nothing evaluated
    sim.set_positions(xy)
    sim.prepare_step()
    sim.set_links(_MIXED)                            # adds mbs -> cue00 and the pairs it crosses
    sim.set_links(_UPLINKS)                          # every pair it reads is there already
    sim.prepare_step()
    sim.set_positions(xy32)                          # new positions: only the current list's pairs
    _assert_log(h.calls, [
        ('device_table', ANY),
        ('links', ([1, 2, 3], [0, 0, 4], [1, 1, 3])),
        ('positions', (xy[..., 0], xy[..., 1])),
        ('table', (_device_table(gains, xy[0], {1, 2, 3}, {0, 4}),)),
        ('links', ([0, 1, 3], [1, 0, 4], [2, 1, 3])),
        ('table', (_device_table(gains, xy[0], {0, 1, 2, 3}, {0, 1, 4}),)),
        ('links', ([1, 2, 3], [0, 0, 4], [1, 1, 3])),
        ('positions', (xy32[..., 0], xy32[..., 1])),
        ('table', (_device_table(gains, xy32[0], {1, 2, 3}, {0, 4}),)),
    ])


def _drive_batch(sim, h):
    """reset_device, float32 and float64 set_positions, a link-list change, an empty link list and back; returns the positions
    each link table should come from."""
    rng = np.random.default_rng(5)
    dev = rng.uniform(-300.0, 300.0, (3, 5, 2)).astype(np.float32)
    dev[1, 4] = dev[1, 3]                            # env 1: due01 on top of due00 - the model refuses that pair
    h.uploads[_native.BUF_POS_X], h.uploads[_native.BUF_POS_Y] = dev[..., 0].copy(), dev[..., 1].copy()
    p32 = rng.uniform(-300.0, 300.0, (3, 5, 2)).astype(np.float32)
    p64 = rng.uniform(-300.0, 300.0, (3, 5, 2))
    p32b = rng.uniform(-300.0, 300.0, (3, 5, 2)).astype(np.float32)
    sim.set_links(_UPLINKS)                          # no positions yet: nothing evaluated
    sim.reset_device(7)
    sim.prepare_step()
    sim.set_positions(p32)
    sim.set_positions(p64)
    sim.set_links(_MIXED)
    sim.set_links([])                                # no links, no pairs
    sim.set_positions(p32b)
    sim.set_links(_UPLINKS)
    sim.prepare_step()
    return dev, p32, p64, p32b


def test_path_loss_link_table_route_follows_positions_and_links(stub):
    """A batch with a per-object model: [B, N, N] by (tx link, rx link) of the current list, evaluated again on every position
    or link change, from the positions as given (float64 kept) or, after a device-side reset, as the handle holds them."""
    sim, h = _sim(_Plugin, num_envs=3)
    gains = [d.tx_antenna_gain_dBi for d in sim.devices.values()]
    dev, p32, p64, p32b = _drive_batch(sim, h)
    up, mixed = ([1, 2, 3], [0, 0, 4]), ([0, 1, 3], [1, 0, 4])
    _assert_log(h.calls, [
        ('device_table', ANY),
        ('links', (*up, [1, 1, 3])),
        ('reset', (7, 0, None, None)),
        ('link_table', (_link_table(gains, dev, *up),)),
        ('positions', (p32[..., 0], p32[..., 1])),
        ('link_table', (_link_table(gains, p32, *up),)),
        ('positions', (p64[..., 0], p64[..., 1])),
        ('link_table', (_link_table(gains, p64, *up),)),
        ('links', (*mixed, [2, 1, 3])),
        ('link_table', (_link_table(gains, p64, *mixed),)),
        ('links', ([], [], [])),
        ('positions', (p32b[..., 0], p32b[..., 1])),
        ('links', (*up, [1, 1, 3])),
        ('link_table', (_link_table(gains, p32b, *up),)),
    ])
    assert np.isnan(_link_table(gains, dev, *up)[1, 2, 2])          # the refused pair stays NaN in the table handed over


@pytest.fixture
def no_gpu(monkeypatch):
    """torch without a GPU, whichever machine runs the suite."""
    try:
        import torch
    except ImportError:         # pragma: no cover - torch is part of the platform
        return
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


def test_array_path_loss_without_a_gpu_takes_the_link_table_route(stub, no_gpu):
    """A once-per-reset ArrayPathLoss on a batch, with no GPU for compute(view): the link-table route through its own per-object
    call, the same calls as that per-object model makes."""
    logs = []
    with np.errstate(divide='ignore'):
        for model in (_ArrayPlugin, _ArrayPluginPerObject):
            sim, h = _sim(model, num_envs=3)
            _drive_batch(sim, h)
            logs.append(h.calls)
    assert [n for n, _ in logs[0]].count('link_table') == 5
    _assert_log(logs[0], logs[1])


def test_stochastic_per_object_model_warns_once(stub, no_gpu):
    """A per-object PathLoss that draws per call is frozen into its table: one UserWarning per simulator, on either table route.
    An ArrayPathLoss is not asked (its stochastic form is per_step)."""
    import warnings
    for model, num_envs, expected in ((_Gauss, 1, 1), (_Gauss, 3, 1), (_Plugin, 3, 0), (_GaussArray, 1, 0), (_GaussArray, 3, 0)):
        with warnings.catch_warnings(record=True) as got:
            warnings.simplefilter('always')
            sim, h = _sim(model, num_envs=num_envs)
            if num_envs == 1:
                sim.set_links(_UPLINKS)
                sim.set_positions(np.random.default_rng(1).uniform(-300.0, 300.0, (1, 5, 2)))
                sim.set_links(_MIXED)
                sim.set_positions(np.random.default_rng(2).uniform(-300.0, 300.0, (1, 5, 2)))
            else:
                _drive_batch(sim, h)
        frozen = [w for w in got if issubclass(w.category, UserWarning) and 'frozen' in str(w.message)]
        assert len(frozen) == expected, (model.__name__, num_envs, [str(w.message) for w in got])

"""Packet traffic on the GPU (VecD2DEnv(traffic=PacketTraffic(...)), csrc/d2d_queue.hip) against the integer restatement of the model
(tests/queue_util.py) and against itself: sharded, autoreset, with mobility.

Every comparison is bit for bit, on all eight planes and on the ring: the model is integers but mean_delay_steps, which both sides
form as one double division rounded once.  The restatement is given the GPU's own capacity_mbps plane, so the step's arithmetic does
not enter.  What each direct-launch case exercises (expiry, overflow, partial service, a queue that empties, an OFF to ON switch) is
counted by the restatement on the CPU and asserted, so a case that exercises nothing fails.

Printed by the test on an MI355X: see CHANGELOG.md."""
import numpy as np
import pytest

import queue_util as qu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SEED = 33
EPISODE = 10
NAMES = qu.PLANES + ('ring',)


def _traffic(**kw):
    from gym_d2d_amd.queues import PacketTraffic
    return PacketTraffic(**kw)


def _env(cfg, b, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    return VecD2DEnv(dict(cfg), num_envs=b, **kw)


def _np(t):
    return t.detach().contiguous().cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)


def _same_bits(a, b, what):
    a, b = _np(a), _np(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


def _env_planes(env):
    """Copies of the env's planes and ring, as NumPy."""
    torch.cuda.synchronize()
    q = env.queues()
    return {name: _np(getattr(q, name)).copy() for name in NAMES}


def _assert_planes(got, ref, what, rows=slice(None)):
    want = ref.planes()
    for name in NAMES:
        w = want[name][:, rows] if name == 'ring' else want[name][rows]
        _same_bits(got[name], w, f'{what}: {name}')


def _actions(env, rng):
    highs = env._initial_action_highs()
    a = np.stack([rng.integers(0, h, env.num_envs) for h in highs], axis=1).astype(np.int32)
    return torch.as_tensor(a, device=env.device)


# ------------------------------------------------------------------------------------------ 1: direct launches
PKT, DT, FIRST_ENV, STEPS = 1000, 1e-3, 4096, 40
MODEL = dict(packets_per_step=(2.0, 0.7), packet_bits=PKT, buffer_bits=5 * PKT + 7, dt_s=DT, p_on_to_off=0.2, p_off_to_on=0.3)


def _synthetic_capacity(rng, b, n):
    """float32 [B, N] Mbps.  By link index mod 7: 0, NaN, -1, 1e-30 (no service: these queues fill, overflow and expire), +inf now
    and then (the queue empties), a whole number of packets (the budget lands on a packet boundary), anything (partial packets)."""
    cap = (rng.random((b, n)) * 3.0).astype(np.float32)
    col = np.arange(n) % 7
    for c, v in enumerate((0.0, np.nan, -1.0, 1e-30)):
        cap[:, col == c] = np.float32(v)
    burst = (col == 4)[None, :] & (rng.random((b, n)) < 0.3)
    cap[burst] = np.inf
    whole = rng.integers(0, 4, (b, n)).astype(np.float32) * np.float32(PKT / (1e6 * DT))
    cap[:, col == 5] = whole[:, col == 5]
    return cap


@pytest.mark.parametrize('d', [1, 3, 8, 32])
@pytest.mark.parametrize('b,cues,pairs', [(3, 3, 4), (5, 3, 4), (3, 70, 61), (5, 70, 61)])
def test_direct_launches_equal_the_restatement_bit_for_bit(b, cues, pairs, d):
    from gym_d2d_amd import _native
    from gym_d2d_amd.queues import PLANES
    assert PLANES == qu.PLANES
    n = cues + pairs
    model = _traffic(deadline_steps=d, seed=77, **MODEL)
    ref = qu.Restatement(b, cues, pairs, deadline_steps=d, seed=77, first_env=FIRST_ENV, **MODEL)
    assert qu.budget_bits(np.float32(PKT / (1e6 * DT)), 1e6 * DT) == PKT            # the boundary value is one whole packet
    dev = torch.device('cuda', 0)
    planes = {}
    for name in PLANES:                                                              # garbage: t = 0 has to clear all of it
        dtype = torch.float32 if name == 'mean_delay_steps' else torch.uint8 if name == 'on' else torch.int32
        planes[name] = torch.full((b, n), 77, dtype=dtype, device=dev)
    ring = torch.full((d, b, n), 12345, dtype=torch.int32, device=dev)
    cap_dev = torch.zeros((b, n), dtype=torch.float32, device=dev)
    tables, switches = model.thresholds(), model.switch_thresholds()

    def launch(step, episode):
        _native.queue_step(cap_dev.data_ptr(), ring.data_ptr(), *(planes[name].data_ptr() for name in PLANES), tables, b, cues, pairs, d,
                           model.packet_bits, model.buffer_bits, model.bits_per_mbps_step, *switches, FIRST_ENV, model.stream_seed(0),
                           step=step, episode=episode, stream_ptr=torch.cuda.current_stream().cuda_stream)

    def got():
        torch.cuda.synchronize()
        return dict({name: _np(planes[name]) for name in PLANES}, ring=_np(ring))
    rng = np.random.default_rng(1000 * b + 10 * n + d)
    episode = 2
    ref.start(episode)
    launch(0, episode)
    _assert_planes(got(), ref, f'D={d} t=0')
    for t in range(1, STEPS + 1):
        cap = _synthetic_capacity(rng, b, n)
        cap_dev.copy_(torch.as_tensor(cap))
        launch(t, episode)
        ref.step(cap)
        _assert_planes(got(), ref, f'D={d} t={t}')
    print(f'direct B={b} N={n} D={d} steps={STEPS}: events {ref.events}, oldest served age {ref.max_served_age}')
    assert all(v > 0 for v in ref.events.values()), ref.events
    assert ref.max_served_age <= d - 1
    ref.start(episode + 1)                                                           # a second episode clears what the first left
    launch(0, episode + 1)
    _assert_planes(got(), ref, f'D={d} next episode t=0')


# ------------------------------------------------------------------------------------------ 2: through VecD2DEnv
def _expected_obs(view_planes, ref, buffer_bits, d):
    p = ref.planes()
    fill = (p['backlog_bits'].astype(np.float64) / float(max(buffer_bits, 1))).astype(np.float32)
    age = (p['hol_age_steps'].astype(np.float64) / float(d)).astype(np.float32)
    return np.stack([view_planes['sinr_db'], view_planes['snr_db'], view_planes['capacity_mbps'], fill, age, p['on'].astype(np.float32)],
                    axis=-1)


def _expected_reward(ref, penalty, bits_per_mbps_step):
    p = ref.planes()
    lost = p['expired_bits'].astype(np.float64) + p['overflow_bits'].astype(np.float64)
    return ((p['served_bits'].astype(np.float64) - float(penalty) * lost) / bits_per_mbps_step).astype(np.float32)


def test_env_planes_info_obs_and_reward_equal_the_restatement():
    from gym_d2d_amd.envs import GoodputRewardFunction, QueueObsFunction
    b, cues, pairs, first_env = 5, 70, 61, 11
    kw = dict(packets_per_step=(3.0, 1.5), packet_bits=12000, deadline_steps=4, buffer_bits=6 * 12000 + 100, dt_s=1e-3, p_on_to_off=0.15,
              p_off_to_on=0.4)
    model = _traffic(**kw)
    cfg = {'num_rbs': 16, 'num_cues': cues, 'num_due_pairs': pairs, 'obs_fn': QueueObsFunction, 'reward_fn': GoodputRewardFunction}
    env = _env(cfg, b, first_env=first_env, traffic=model)
    ref = qu.Restatement(b, cues, pairs, seed=qu.stream_seed(SEED), first_env=first_env, **kw)
    rng = np.random.default_rng(8)
    assert env.reward_fn.drop_penalty == 1.0

    def signal_planes():
        v = env._view()
        return {k: _np(getattr(v, k)) for k in ('sinr_db', 'snr_db', 'capacity_mbps')}
    for episode in range(2):
        obs = env.reset(seed=SEED) if episode == 0 else env.reset()
        ref.start(episode)
        _assert_planes(_env_planes(env), ref, f'episode {episode} reset')
        _same_bits(obs, _expected_obs(signal_planes(), ref, model.buffer_bits, model.deadline_steps), f'episode {episode} reset obs')
        assert tuple(obs.shape) == (b, cues + pairs, 6)
        for t in range(1, EPISODE + 1):
            obs, rewards, dones, info = env.step(_actions(env, rng))
            sig = signal_planes()
            ref.step(sig['capacity_mbps'])
            what = f'episode {episode} step {t}'
            _assert_planes(_env_planes(env), ref, what)
            want = ref.planes()
            for name in ('served_bits', 'backlog_bits', 'expired_bits', 'overflow_bits'):
                _same_bits(info[name], want[name], f'{what}: info[{name}]')
                assert info[name] is getattr(env.queues(), name) is getattr(env._view(), name)
            _same_bits(obs, _expected_obs(sig, ref, model.buffer_bits, model.deadline_steps), f'{what}: QueueObsFunction')
            _same_bits(rewards, _expected_reward(ref, 1.0, model.bits_per_mbps_step), f'{what}: GoodputRewardFunction')
            assert bool(dones.all()) == (t == EPISODE)
    print(f'env B={b} N={cues + pairs} D={model.deadline_steps}, two episodes: events {ref.events}')
    assert env._view().traffic is model and env.status_flags() == 0
    env.close()


# ------------------------------------------------------------------------------------------ 3: sharding and autoreset
SMALL = {'num_rbs': 6, 'num_cues': 6, 'num_due_pairs': 7, 'seed': 7}
SMALL_MODEL = dict(packets_per_step=(2.5, 1.0), packet_bits=8000, deadline_steps=3, buffer_bits=4 * 8000, p_on_to_off=0.2, p_off_to_on=0.5)


def test_two_shards_equal_the_whole_batch():
    b, half = 6, 3
    rng = np.random.default_rng(3)
    acts = [rng.integers(0, 6 * 21, (b, 13)).astype(np.int32) for _ in range(EPISODE)]      # (below every column's action range)

    def run(n, first_env, rows):
        env = _env(SMALL, n, first_env=first_env, traffic=_traffic(**SMALL_MODEL))
        env.reset(seed=SEED)
        out = [_env_planes(env)]
        for a in acts:
            env.step(torch.as_tensor(a[rows], device=env.device))
            out.append(_env_planes(env))
        env.close()
        return out
    whole = run(b, 0, slice(None))
    assert sum(int(p['served_bits'].sum()) for p in whole) > 0 and sum(int(p['overflow_bits'].sum()) for p in whole) > 0
    for k in range(2):
        rows = slice(k * half, (k + 1) * half)
        for t, (w, s) in enumerate(zip(whole, run(half, k * half, rows))):
            for name in NAMES:
                _same_bits(s[name], w[name][:, rows] if name == 'ring' else w[name][rows], f'shard {k} step {t}: {name}')


@pytest.mark.parametrize('moving', [False, True], ids=['still', 'mobility'])
def test_autoreset_with_staggered_episodes_equals_one_lockstep_env_each(moving):
    from gym_d2d_amd.mobility import GaussMarkovMobility
    b, steps, first = 6, 24, 40
    extra = lambda: dict(mobility=GaussMarkovMobility(speed_std_mps=8.0, memory=0.7)) if moving else {}
    env = _env(SMALL, b, autoreset=True, first_env=first, traffic=_traffic(**SMALL_MODEL), **extra())
    env.reset(seed=SEED, elapsed=np.arange(b) % EPISODE)
    start = _env_planes(env)
    rng = np.random.default_rng(4)
    acts, outs, resets = [], [], []
    for t in range(1, steps + 1):
        if t == 15:
            env.request_reset(np.arange(b) % 2 == 0)
        a = _actions(env, rng)
        _, _, _, info = env.step(a)
        outs.append(dict(_env_planes(env), capacity_mbps=_np(info['capacity_mbps']).copy()))
        resets.append(_np(info['reset']).copy()); acts.append(a)
    env.close()
    resets = np.array(resets)
    assert resets.sum() >= 2 * b                                  # every env crosses two episode boundaries
    for e in range(b):
        one = _env(SMALL, 1, first_env=first + e, traffic=_traffic(**SMALL_MODEL), **extra())
        one.reset(seed=SEED)
        want = _env_planes(one)
        for name in NAMES:
            _same_bits(start[name][:, e:e + 1] if name == 'ring' else start[name][e:e + 1], want[name], f'env {e} reset: {name}')
        for t in range(steps):
            if resets[t, e]:
                one.reset()
                for name in NAMES:                               # reset inside the step: zero planes, a cleared ring
                    if name != 'on':
                        g = outs[t][name]
                        assert not (g[:, e] if name == 'ring' else g[e]).any(), (e, t, name)
            else:
                one.step(acts[t][e:e + 1].contiguous())
            want = dict(_env_planes(one), capacity_mbps=_np(one._view().capacity_mbps))
            for name in NAMES + ('capacity_mbps',):
                g = outs[t][name]
                _same_bits(g[:, e:e + 1] if name == 'ring' else g[e:e + 1], want[name], f'env {e} step {t + 1}: {name}')
        one.close()
    assert sum(int(o['served_bits'].sum()) for o in outs) > 0 and sum(int(o['expired_bits'].sum()) for o in outs) > 0


# ------------------------------------------------------------------------------------------ 4: an env without traffic=
def test_an_env_without_traffic_returns_what_one_with_it_returns():
    from gym_d2d_amd import _native
    b = 4
    plain = _env(SMALL, b, first_env=5)
    before = _native.queue_launches
    obs0 = plain.reset(seed=SEED).clone()
    a = torch.zeros((b, 13), dtype=torch.int32, device=plain.device)
    plain.step(a)
    assert _native.queue_launches == before and plain._queues is None
    queued = _env(SMALL, b, first_env=5, traffic=_traffic(**SMALL_MODEL))
    obs1 = queued.reset(seed=SEED)
    assert _native.queue_launches == before + 1
    _same_bits(obs1, obs0, 'reset obs')
    plain.reset(seed=SEED)
    for step in range(2):
        for name in ('pos_x', 'pos_y', 'sinr_db', 'snr_db', 'capacity_mbps', 'rate_bps', 'rb', 'pwr', 'table', 'reward'):
            _same_bits(queued._t[name], plain._t[name], f'step {step}: {name}')
        o0, r0, _, i0 = plain.step(a)
        o1, r1, _, i1 = queued.step(a)
        _same_bits(o1, o0, f'step {step + 1}: obs'); _same_bits(r1, r0, f'step {step + 1}: reward')
        assert set(i1) - set(i0) == {'served_bits', 'backlog_bits', 'expired_bits', 'overflow_bits'}
    plain.close(); queued.close()

"""Packet traffic, the part that needs no GPU: libd2d_queue.so's header and exports, what its entry point refuses, the queue kernel's
resources, the model object's range checks and threshold tables, the integer restatement's own invariants (tests/queue_util.py, the
yardstick of test_gpu_queue.py), the refusals, and that an env without a model never touches the library."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import queue_util as qu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_queue.hip'
HEADER = ROOT / 'include' / 'd2d_queue.h'


# ---------------------------------------------------------------------------------------------- header and library
def test_queue_header_is_valid_c_and_cpp():
    for compiler, std in (('gcc', '-std=c99'), ('g++', '-std=c++17')):
        if shutil.which(compiler) is None:
            pytest.skip(f'{compiler} missing')
        r = subprocess.run([compiler, std, '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-x', 'c' if compiler == 'gcc' else 'c++',
                            str(HEADER)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_queue_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    lib = _native.load_queue_library()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', HEADER.read_text(), flags=re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / 'libd2d_queue.so')], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}
    assert exported == declared == {'d2d_queue_step', 'd2d_queue_last_error'}
    assert set(_native.QUEUE_SIGNATURES) == declared
    decl = re.search(r'int d2d_queue_step\((.*?)\);', HEADER.read_text(), flags=re.S).group(1)
    assert len(_native.QUEUE_SIGNATURES['d2d_queue_step'][1]) == len(decl.split(',')) == 30
    for name in declared:
        assert getattr(lib, name).restype is not None
    text = HEADER.read_text()
    assert int(re.search(r'#define D2D_QUEUE_MAX_DEADLINE (\d+)', text).group(1)) == _native.QUEUE_MAX_DEADLINE == 32
    assert int(re.search(r'#define D2D_QUEUE_TABLE (\d+)', text).group(1)) == _native.QUEUE_TABLE == qu.TABLE == 64
    assert 'SLOT-MAJOR' in text and 'still transmits' in text


def test_step_library_still_exports_its_43():
    from gym_d2d_amd import _native
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / 'libd2d_hip.so')], capture_output=True, text=True, check=True).stdout
    assert len({ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}) == 43 == len(_native.SIGNATURES)


def test_queue_library_is_registered_in_the_build(tmp_path):
    from gym_d2d_amd import build
    assert build.LIBRARIES['queue'] == ['d2d_queue.hip'] and HEADER in build.HEADERS and build.lib_path('queue') == LIB_DIR / 'libd2d_queue.so'
    names = {p.name for p in build.HEADERS} | set(build.LIBRARIES['queue'])
    assert {'d2d_queue.hip', 'd2d_queue.h'} <= names
    # compiled and linked (the build iterates LIBRARIES and nothing else), in the digest, in the up-to-date test
    assert SOURCE in build.digest_files() and HEADER in build.digest_files()
    digest = build.source_digest()
    for stem in build.LIBRARIES:
        if stem != 'probe':
            build.lib_path(stem, tmp_path).touch()
    (tmp_path / 'libd2d_hip.sha256').write_text(digest)
    assert build.up_to_date(digest, tmp_path) and not build.up_to_date('0' * 64, tmp_path)
    build.lib_path('queue', tmp_path).unlink()
    assert not build.up_to_date(digest, tmp_path)


def test_queue_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    tables = np.stack([qu.poisson_table(1.0), qu.poisson_table(2.0)])
    ok = dict(ptr=8, ring=8, tables=tables, n_envs=2, n_cues=3, n_due_pairs=4, d=8, packet_bits=12000, buffer_bits=120000, bps=1000.0,
              first_env=0, clock={})

    def call(**kw):
        a = dict(ok, **kw)
        p = a['ptr']
        _native.queue_step(p, a['ring'], p, p, p, p, p, p, p, p, a['tables'], a['n_envs'], a['n_cues'], a['n_due_pairs'], a['d'],
                           a['packet_bits'], a['buffer_bits'], a['bps'], 0, qu.U32, qu.U32, a['first_env'], 1, **a['clock'])
    falling = tables.copy()
    falling[1, 5] = falling[1, 4] - 1
    before = _native.queue_launches
    for kw, text in ((dict(d=0), 'deadline_steps'), (dict(d=33), 'deadline_steps'), (dict(d=-1), 'deadline_steps'),
                     (dict(n_envs=-1), 'n_envs'), (dict(n_cues=-1), 'n_cues'), (dict(n_due_pairs=-1), 'n_due_pairs'),
                     (dict(first_env=(1 << 32) - 1), 'first_env'),
                     (dict(packet_bits=0), 'packet_bits'), (dict(packet_bits=1 << 25), 'packet_bits'),
                     (dict(buffer_bits=1 << 31), 'buffer_bits'), (dict(buffer_bits=-1), 'buffer_bits'),
                     (dict(bps=0.0), 'bits_per_mbps_step'), (dict(bps=float('nan')), 'bits_per_mbps_step'),
                     (dict(bps=float('inf')), 'bits_per_mbps_step'), (dict(tables=falling), 'must not decrease'),
                     (dict(ptr=0), 'null device pointer'), (dict(ring=0), 'null device pointer'),
                     (dict(clock=dict(reset_ptr=8)), 'per-env clock'),
                     (dict(clock=dict(reset_ptr=8, elapsed_ptr=8, episode_ptr=8)), 'per-env clock')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    with pytest.raises(ValueError, match='thresholds'):
        call(tables=tables[:, :32])
    assert _native.queue_launches == before
    call(n_envs=0)                                                   # nothing to do: no launch behind it, no error
    call(n_cues=0, n_due_pairs=0)
    call(n_envs=0, packet_bits=(1 << 25) - 1, buffer_bits=(1 << 31) - 1)     # 64 * packet_bits = 2^31 - 64: the largest allowed


@pytest.fixture(scope='module')
def queue_kernel(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_queue')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'queue.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    kernels = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        if not name or 'queue_step_kernel' not in name.group(1):
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        kernels[name.group(1)] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                        'private_segment_fixed_size', 'group_segment_fixed_size')}
    return kernels, asm


def test_queue_kernel_uses_no_scratch_spills_nothing_and_has_no_atomics(queue_kernel):
    """One kernel serves the lockstep and the per-env clock, every D.  LDS: the two 64-entry tables, 512 bytes."""
    kernels, asm = queue_kernel
    assert len(kernels) == 1
    for name, k in kernels.items():
        print(name, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == 512, k
        assert k['vgpr_count'] <= 64, k                              # 64 is where occupancy would drop below 8 waves per SIMD
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    src = SOURCE.read_text().split('#include', 1)[1]
    assert 'atomic' not in src and 'asm' not in src                   # plain C++ only


# ---------------------------------------------------------------------------------------------- the model object
def test_model_range_checks():
    from gym_d2d_amd.queues import SEED_MIX, PacketTraffic
    from gym_d2d_amd.mobility import SEED_MIX as MOBILITY_MIX
    from gym_d2d_amd.path_loss import FADING_SEED_MIX, SHADOW_SEED_MIX
    m = PacketTraffic()
    assert (m.packets_per_step, m.packet_bits, m.deadline_steps, m.buffer_bits, m.dt_s, m.p_on_to_off, m.p_off_to_on, m.seed) == \
        ((1.0, 1.0), 12000, 8, 64 * 12000, 1e-3, 0.0, 1.0, None)
    assert m.bits_per_mbps_step == 1e6 * 1e-3
    for kw in (dict(packets_per_step=-0.1), dict(packets_per_step=16.5), dict(packets_per_step=(1.0, 17.0)),
               dict(packets_per_step=(1.0, 2.0, 3.0)), dict(packets_per_step=float('nan')), dict(packets_per_step='1'),
               dict(packet_bits=0), dict(packet_bits=1 << 25), dict(packet_bits=1.5), dict(deadline_steps=0), dict(deadline_steps=33),
               dict(deadline_steps=2.0), dict(buffer_bits=-1), dict(buffer_bits=1 << 31), dict(buffer_bits=1e6), dict(dt_s=0),
               dict(dt_s=float('inf')), dict(p_on_to_off=-0.1), dict(p_on_to_off=1.1), dict(p_off_to_on=2), dict(p_off_to_on=float('nan')),
               dict(seed=-1), dict(seed=1.5)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            PacketTraffic(**kw)
    m = PacketTraffic(packets_per_step=(0.5, 3.0), p_on_to_off=0.25, p_off_to_on=0.5, packet_bits=(1 << 25) - 1, buffer_bits=(1 << 31) - 1)
    assert m.packets_per_step == (0.5, 3.0) and m.on_share == 0.5 / 0.75
    assert m.switch_thresholds() == (qu.threshold(0.25), qu.threshold(0.5), qu.threshold(qu.on_share(0.25, 0.5))) == (1 << 30, 1 << 31, 2863311530)
    assert PacketTraffic().switch_thresholds() == (0, qu.U32, qu.U32) and PacketTraffic(p_off_to_on=0.0).on_share == 1.0
    assert SEED_MIX == qu.SEED_MIX and len({SEED_MIX, MOBILITY_MIX, FADING_SEED_MIX, SHADOW_SEED_MIX}) == 4
    assert m.stream_seed(9) == qu.stream_seed(9) == 9 ^ SEED_MIX and PacketTraffic(seed=4).stream_seed(9) == 4


@pytest.mark.parametrize('lam', [0.0, 0.01, 1.0, 7.5, 16.0])
def test_thresholds_equal_the_restatement_s_tables_entry_for_entry(lam):
    from gym_d2d_amd.queues import PacketTraffic
    tab = PacketTraffic(packets_per_step=(lam, 16.0 - lam)).thresholds()
    assert tab.dtype == np.uint32 and tab.shape == (2, 64)
    for row, rate in zip(tab, (lam, 16.0 - lam)):
        want = qu.poisson_table(rate)
        assert np.array_equal(row, want)
        assert (np.diff(want.astype(np.int64)) >= 0).all()
        assert want[0] == min(qu.U32, math.floor(math.exp(-rate) * 2.0 ** 32))
        # the tail beyond the table: what the last entry leaves of 2^32 (rounding of the float64 sum included) is a few words
        assert int(qu.U32) - int(want[-1]) <= 16, (rate, want[-1])


# ---------------------------------------------------------------------------------------------- the restatement on its own
def _capacities(rng, shape, scale_mbps):
    """float32 [B, N] with the awkward values strewn in."""
    cap = (rng.random(shape) * scale_mbps).astype(np.float32)
    special = np.array([0.0, np.nan, -1.0, np.inf, 1e-30], dtype=np.float32)
    mask = rng.random(shape) < 0.15
    cap[mask] = rng.choice(special, size=int(mask.sum()))
    return cap


@pytest.mark.parametrize('kw', [dict(deadline_steps=1, packets_per_step=(2.0, 0.5)), dict(deadline_steps=3, packets_per_step=(3.0, 1.0)),
                                dict(deadline_steps=8, packets_per_step=(1.5, 4.0), p_on_to_off=0.2, p_off_to_on=0.3),
                                dict(deadline_steps=32, packets_per_step=(6.0, 2.0), buffer_bits=15 * 1000 + 7)])
def test_restatement_conserves_bits_on_every_step(kw):
    b, cues, pairs, pkt = 6, 9, 11, 1000
    kw = dict(dict(packet_bits=pkt, buffer_bits=4 * pkt, dt_s=1e-3), **kw)
    scale = 0.3 if kw['deadline_steps'] == 32 else 4.0                # Mbps: at D = 32 a cohort has to wait 32 steps to expire
    r = qu.Restatement(b, cues, pairs, seed=qu.stream_seed(3), first_env=17, **kw)
    rng = np.random.default_rng(5)
    d = kw['deadline_steps']
    for t in range(1, 81):
        before = r.backlog_bits.copy()
        cap = _capacities(rng, (b, cues + pairs), scale)
        r.step(cap)
        assert np.array_equal(r.arrived_bits, r.admitted_bits + r.overflow_bits), t
        assert np.array_equal(r.backlog_bits, before + r.admitted_bits - r.served_bits - r.expired_bits), t
        assert (r.backlog_bits <= r.buffer_bits).all() and (r.backlog_bits >= 0).all(), t
        assert np.array_equal(r.backlog_bits, r.ring.sum(axis=0)) and (r.ring >= 0).all(), t
        assert (r.arrived_bits % pkt == 0).all() and (r.overflow_bits % pkt == 0).all(), t
        assert (r.served_bits <= qu.budget_bits(cap, r.bits_per_mbps_step)).all(), t
        assert ((r.hol_age_steps >= 0) & (r.hol_age_steps <= d - 1)).all() and (r.hol_age_steps[r.backlog_bits == 0] == 0).all(), t
        assert (r.mean_delay_steps >= 0).all() and (r.mean_delay_steps <= d - 1).all() and (r.mean_delay_steps[r.served_bits == 0] == 0).all()
        assert (r.arrived_bits[r.on == 0] == 0).all(), t
    print(kw, r.events, 'oldest served age', r.max_served_age)
    assert r.max_served_age <= d - 1                                 # nothing older than D - 1 steps is ever served
    assert r.events['expiry'] > 0 and r.events['overflow'] > 0 and r.events['partial'] > 0 and r.events['emptied'] > 0
    assert (r.events['switched_on'] > 0) == ('p_on_to_off' in kw)


def test_restatement_budget_rule():
    cap = np.array([0.0, np.nan, -1.0, np.inf, 1e-30, 12.0, 0.0125, 3.0000002, -np.inf, 3e6], dtype=np.float32)
    want = [0, 0, 0, 2 ** 31 - 1, 0, 12000, 12, math.floor(float(np.float32(3.0000002)) * 1000.0), 0, 2 ** 31 - 1]
    assert qu.budget_bits(cap, 1e6 * 1e-3).tolist() == want


def test_restatement_draws_do_not_depend_on_the_batch_split():
    kw = dict(packets_per_step=(2.0, 3.0), packet_bits=500, deadline_steps=4, buffer_bits=6000, p_on_to_off=0.3, p_off_to_on=0.4, seed=99)
    whole = qu.Restatement(8, 3, 4, first_env=5, **kw)
    part = qu.Restatement(4, 3, 4, first_env=9, **kw)
    rng = np.random.default_rng(1)
    assert np.array_equal(whole.on[4:], part.on)
    for _ in range(12):
        cap = (rng.random((8, 7)) * 3).astype(np.float32)
        whole.step(cap); part.step(cap[4:])
        for name, got in part.planes().items():
            want = whole.planes()[name]
            assert np.array_equal(got, want[:, 4:] if name == 'ring' else want[4:]), name
    a = qu.words(99, 5, 2, 3, 8, 9)
    assert not np.array_equal(a, qu.words(99, 5, 3, 3, 8, 9)) and not np.array_equal(a, qu.words(99, 5, 2, 4, 8, 9))
    assert not np.array_equal(a, qu.words(98, 5, 2, 3, 8, 9))


def test_restatement_arrival_mean_and_on_share_follow_the_model():
    """About 1e5 draws.  A link's state is a stationary two-state chain with lag-one correlation rho = 1 - p_on_to_off - p_off_to_on;
    over T steps the variance of its time average is at most pi (1 - pi) / T * (1 + rho) / (1 - rho).  Arrivals are a Poisson count
    masked by the state: Var(sum) <= L T lambda pi + lambda^2 Var(sum of on).  Five standard errors, both from the model."""
    p_off, p_on, lam = 0.1, 0.3, 2.5
    b, n, steps = 25, 100, 40
    pi = qu.on_share(p_off, p_on)
    r = qu.Restatement(b, n, 0, packets_per_step=(lam, 0.0), packet_bits=100, deadline_steps=1, buffer_bits=2 ** 31 - 1, p_on_to_off=p_off,
                       p_off_to_on=p_on, seed=12345)
    on0 = r.on.mean()
    se0 = math.sqrt(pi * (1 - pi) / (b * n))
    assert abs(on0 - pi) <= 5 * se0, (on0, pi, se0)
    on_sum = arrivals = 0
    cap = np.full((b, n), np.inf, dtype=np.float32)
    for _ in range(steps):
        r.step(cap)
        on_sum += int(r.on.sum()); arrivals += int(r.arrived_bits.sum()) // 100
    draws = b * n * steps
    rho = 1.0 - p_off - p_on
    var_on = draws * pi * (1 - pi) * (1 + rho) / (1 - rho)             # of the sum over links and steps
    se_on = math.sqrt(var_on) / draws
    se_arr = math.sqrt(draws * lam * pi + lam * lam * var_on) / draws
    print(f'{draws} draws: ON share {on_sum / draws:.5f} (model {pi:.5f}, se {se_on:.5f}); arrivals per draw {arrivals / draws:.5f} '
          f'(model {lam * pi:.5f}, se {se_arr:.5f})')
    assert abs(on_sum / draws - pi) <= 5 * se_on
    assert abs(arrivals / draws - lam * pi) <= 5 * se_arr
    assert r.events['overflow'] == 0 and r.events['expiry'] == 0


# ---------------------------------------------------------------------------------------------- the env
@pytest.fixture
def stub(monkeypatch):
    from gym_d2d_amd import _native
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    return RecordingHandle


def test_every_refusal_raises_at_construction_with_its_text(stub):
    from gym_d2d_amd.envs import GoodputRewardFunction, QueueObsFunction, VecD2DEnv
    from gym_d2d_amd.queues import PacketTraffic
    cfg = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}
    with pytest.raises(ValueError, match='traffic= needs the torch path'):
        VecD2DEnv(dict(cfg), num_envs=2, use_torch=False, traffic=PacketTraffic())
    with pytest.raises(TypeError, match='PacketTraffic'):
        VecD2DEnv(dict(cfg), num_envs=2, use_torch=False, traffic={'packets_per_step': 1.0})
    with pytest.raises(ValueError, match='QueueObsFunction needs traffic='):
        VecD2DEnv(dict(cfg, obs_fn=QueueObsFunction), num_envs=2, use_torch=False)
    with pytest.raises(ValueError, match='GoodputRewardFunction needs traffic='):
        VecD2DEnv(dict(cfg, reward_fn=GoodputRewardFunction), num_envs=2, use_torch=False)
    assert QueueObsFunction().get_obs_space(None).shape == (6,)
    with pytest.raises(RuntimeError, match='VecD2DEnv'):
        GoodputRewardFunction()({}, {})


def test_an_env_without_a_model_never_opens_the_library(stub, monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv

    def opened():
        raise AssertionError('libd2d_queue.so was opened by an env without a traffic model')
    monkeypatch.setattr(_native, 'load_queue_library', opened)
    before = _native.queue_launches
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=3, use_torch=False)
    env.reset(seed=1)
    for _ in range(3):
        _, _, _, info = env.step(np.zeros((3, 5), dtype=np.int32))
    assert env._queues is None and 'backlog_bits' not in env._t and 'traffic' not in env._t
    assert set(info) == {'rb', 'tx_pwr_dbm', 'snr_db', 'sinr_db', 'rate_bps', 'capacity_mbps'}
    with pytest.raises(ValueError, match='traffic='):
        env.queues()
    env.close()
    assert _native.queue_launches == before

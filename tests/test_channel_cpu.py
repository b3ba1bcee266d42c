"""SpatialChannelPathLoss, the part that needs no GPU: libd2d_channel.so's header and exports, the fill kernels' resources, the
statistics of the float64 restatement (tests/channel_util.py, the yardstick of test_gpu_channel.py), the conditions under which the
restatement can judge the large direct launches (tests/channel_large_util.py, the cases of test_gpu_channel_large.py), the model's
range checks, every refusal by its text, and that an env without the model never touches the library."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import channel_large_util as clu
import channel_util as cu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_channel.hip'
HEADER = ROOT / 'include' / 'd2d_channel.h'
CFG = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}


# ---------------------------------------------------------------------------------------------- the library
def test_channel_header_is_valid_c_and_cpp():
    for compiler, std in (('gcc', '-std=c99'), ('g++', '-std=c++17')):
        if shutil.which(compiler) is None:
            pytest.skip(f'{compiler} missing')
        r = subprocess.run([compiler, std, '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-x', 'c' if compiler == 'gcc' else 'c++',
                            str(HEADER)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_channel_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    lib = _native.load_channel_library()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', HEADER.read_text(), flags=re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / 'libd2d_channel.so')], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}
    assert exported == declared == {'d2d_channel_fill', 'd2d_channel_last_error'}
    assert set(_native.CHANNEL_SIGNATURES) == declared
    decl = re.search(r'int d2d_channel_fill\((.*?)\);', HEADER.read_text(), flags=re.S).group(1)
    assert len(_native.CHANNEL_SIGNATURES['d2d_channel_fill'][1]) == len(decl.split(',')) == 29
    for name in declared:
        assert getattr(lib, name).restype is not None


def test_step_library_still_exports_its_43():
    from gym_d2d_amd import _native
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / 'libd2d_hip.so')], capture_output=True, text=True, check=True).stdout
    assert len({ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}) == 43 == len(_native.SIGNATURES)


def test_channel_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(ptr=16, n_envs=2, n_dev=8, n_links=5, first_env=0, m=16, amp=2.0, scale=0.01, fading=1, mu=0.9, s=0.3, scratch=16,
              table=16, dtype=1, clock={})

    def call(**kw):
        a = dict(ok, **kw)
        _native.channel_fill(*([a['ptr']] * 7), a['n_envs'], a['n_dev'], a['n_links'], a['first_env'], a['m'], a['amp'], a['scale'],
                             a['fading'], a['mu'], a['s'], 1, 2, a['scratch'], a['table'], a['dtype'], **a['clock'])
    before = _native.channel_launches
    for kw, text in ((dict(n_envs=-1), 'n_envs'), (dict(n_links=0), 'n_links'), (dict(n_links=2049), 'n_links'),
                     (dict(n_dev=65536), 'n_dev'), (dict(first_env=(1 << 32) - 1), 'first_env'), (dict(m=12), 'num_sinusoids'),
                     (dict(fading=3), 'fading'), (dict(dtype=2), 'table_dtype'), (dict(scale=0.0), 'wave_scale'), (dict(amp=float('nan')), 'shadow_amp_db'),
                     (dict(fading=2, s=0.0), 'rician_s'), (dict(ptr=0), 'null device pointer'), (dict(table=0), 'null device pointer'),
                     (dict(scratch=0), 'phase_scratch'), (dict(table=8), '16-byte aligned'),
                     (dict(clock=dict(reset_ptr=16)), 'per-env clock')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.channel_launches == before
    call(n_envs=0)                                                   # nothing to do: no launch behind it, no error
    call(n_envs=0, m=0, scratch=0)                                   # no shadowing: no work space needed


@pytest.fixture(scope='module')
def fill_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_channel')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'channel.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    kernels = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        if not name or 'channel_' not in name.group(1):
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        kernels[name.group(1)] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                        'private_segment_fixed_size', 'group_segment_fixed_size')}
    return kernels, asm


def test_fill_kernels_use_no_scratch_spill_nothing_and_no_atomics(fill_kernels):
    """3 phase kernels (M_s = 8, 16, 32) and 24 fill kernels (M_s = 0, 8, 16, 32 x no fading, Rayleigh, Rician x float32, float64
    entries).  On the build this was written on the largest is the M_s = 32 Rician fill: 127 VGPRs, 9.3 KB of LDS."""
    kernels, asm = fill_kernels
    assert len(kernels) == 27
    for name, k in kernels.items():
        print(name, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (name, k)
        assert k['vgpr_count'] <= 128, (name, k)                     # 4 waves per SIMD: the LDS of the same kernel allows 16 per CU
        assert k['group_segment_fixed_size'] <= 10 * 1024, (name, k)
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'atomic' not in SOURCE.read_text().split('#include', 1)[1].replace('No atomics', '')


# ---------------------------------------------------------------------------------------------- the restatement on its own
def test_restated_shadowing_has_the_stated_variance_and_correlation():
    """4096 envs, one transmitter, receivers at displacements 0, d_c / 2 and d_c.  The bars are the estimators' own: the sample
    variance of n Gaussian-like values has the relative SE sqrt(2 / n) (11 % at 5 SE), a sample correlation (1 - rho^2) / sqrt(n)."""
    b, sigma, dc = 4096, 8.0, 20.0
    for m in (8, 16, 32):
        k_tx, k_rx, phi = cu.wave_vectors(cu.stream_seeds(123)[0], 0, 0, b, m, dc)
        p_tx = np.broadcast_to(np.array([100.0, 50.0]), (b, 1, 2))
        p_rx = np.broadcast_to(np.array([[-30.0, 200.0], [-30.0 + dc / 2, 200.0], [-30.0, 200.0 + dc]]), (b, 3, 2))
        s = cu.shadow_db(p_tx, p_rx, k_tx, k_rx, phi, sigma)[:, 0]            # [B, 3]
        var = s.var(axis=0)
        corr = np.corrcoef(s.T)[0]
        print(m, 'variance / sigma^2', var / sigma ** 2, 'correlation', corr)
        assert (np.abs(var - sigma ** 2) <= 5 * sigma ** 2 * np.sqrt(2.0 / b)).all()
        for r, got in zip((0.0, dc / 2, dc), corr):
            rho = np.exp(-r / dc)
            assert abs(got - rho) <= 5 * (1 - rho ** 2) / np.sqrt(b) + 1e-12


def test_restated_shadow_of_a_pair_that_stands_still_is_constant_within_an_episode_and_redrawn_with_it():
    k0 = cu.wave_vectors(5, 7, 0, 3, 16, 20.0)
    assert all(np.array_equal(a, b) for a, b in zip(k0, cu.wave_vectors(5, 7, 0, 3, 16, 20.0)))
    assert not np.array_equal(k0[0], cu.wave_vectors(5, 7, 1, 3, 16, 20.0)[0])
    assert np.array_equal(k0[0][1:], cu.wave_vectors(5, 8, 0, 2, 16, 20.0)[0])      # shards: keyed by the global env index
    assert np.array_equal(cu.wave_vectors(5, 7, np.array([0, 1, 0]), 3, 16, 20.0)[0][1], cu.wave_vectors(5, 7, 1, 3, 16, 20.0)[0][1])


def test_restated_rayleigh_power_has_mean_one():
    h2 = cu.fading_h2(cu.stream_seeds(9)[1], 0, 0, 1, 100, np.arange(100), np.arange(100), 'rayleigh')
    assert h2.size == 10 ** 6
    print('Rayleigh mean', h2.mean())
    assert abs(h2.mean() - 1.0) <= 5e-3                              # Exp(1): sd 1, SE 1e-3 over 1e6 draws; 5 SE


def test_restated_rician_power_has_the_stated_mean_and_variance():
    for k_db in (0.0, 6.0, 10.0):
        h2 = cu.fading_h2(cu.stream_seeds(9)[1], 0, 2, 3, 100, np.arange(100), np.arange(100), 'rician', k_db)
        n, k = h2.size, 10.0 ** (k_db / 10.0)
        mean, var = h2.mean(), h2.var()
        m4 = ((h2 - mean) ** 4).mean()
        se_mean, se_var = np.sqrt(var / n), np.sqrt((m4 - var ** 2) / n)     # from the sample's own moments
        print(k_db, 'mean', mean, 'var', var, 'wanted', (2 * k + 1) / (k + 1) ** 2, 'SE', se_mean, se_var)
        assert abs(mean - 1.0) <= 5 * se_mean
        assert abs(var - (2 * k + 1) / (k + 1) ** 2) <= 5 * se_var


def test_fading_is_keyed_by_device_pair_step_and_episode():
    a = cu.fading_h2(3, 0, 0, 1, 2, [1, 2, 1], [0, 0, 5], 'rayleigh')
    assert np.array_equal(a[:, 0], a[:, 2]) and not np.array_equal(a[:, 0], a[:, 1])       # rows 0 and 2: the same transmitter
    assert not np.array_equal(a, cu.fading_h2(3, 0, 0, 2, 2, [1, 2, 1], [0, 0, 5], 'rayleigh'))
    assert not np.array_equal(a, cu.fading_h2(3, 0, 1, 1, 2, [1, 2, 1], [0, 0, 5], 'rayleigh'))


# ---------------------------------------------------------------------------------------------- the large cases' conditions
MIN_ENTRY_DB = 5.0              # the relative measure |got - want| / |want| never divides by less than this


@pytest.mark.parametrize('name', list(clu.CASES))
def test_large_case_can_be_judged_by_the_restatement(name):
    """The left-out share is within the cap, every kept entry is finite (but the one case h makes -inf) and at least MIN_ENTRY_DB
    from 0 dB.  Printed per case: the share left out and the smallest kept |entry|."""
    c = clu.build_case(name)
    want, h2 = clu.restated(name)
    n = c['n']
    assert want.shape == (c['b'], n + 1, n)
    keep = np.ones(want.shape, dtype=bool)
    if h2 is not None:
        keep[:, :n] = h2 >= cu.DEEP_FADE
        keep[:, n] = h2[:, np.arange(n), np.arange(n)] >= cu.DEEP_FADE
    inf = clu.infinite_entries(c)
    assert np.array_equal(np.isneginf(want), inf) and int(inf.sum()) == (1 if name == 'h' else 0)
    kept = want[keep & ~inf]
    print(f'{name}: B {c["b"]} N {n} D {c["d"]}: {1.0 - keep.mean():.2g} left out, min |entry| of the kept {np.abs(kept).min():.3g} dB')
    assert 1.0 - keep.mean() <= cu.DEEP_FADE_CAP
    assert np.isfinite(kept).all()
    assert np.abs(kept).min() >= MIN_ENTRY_DB
    assert np.array_equal(want[:, n], want[:, np.arange(n), np.arange(n)])
    assert c['n'] <= c['d'] and c['tx'].max() < c['d'] and c['rx'].max() < c['d'] and min(c['tx'].min(), c['rx'].min()) >= 0
    assert c['pos'].dtype == np.float32 and (np.hypot(c['pos'][..., 0], c['pos'][..., 1]) <= 500.0 * (1 + 1e-6)).all()


def test_large_cases_cover_what_they_claim():
    case = {k: clu.build_case(k) for k in clu.CASES}
    # the env mapping: more than one group of eight, the last one partial
    for k in ('a', 'b', 'c', 'f_rayleigh', 'f_rician', 'g', 'h'):
        assert case[k]['b'] > 8 and case[k]['b'] % 8 != 0, k
    assert (case['a']['b'], case['b']['b'], case['c']['b']) == (9, 17, 11)
    assert case['b']['first_env'] + case['b']['b'] == 2 ** 32                # the last env's counter word is 2^32 - 1
    # tile edges: 64 columns, 32 rows
    assert case['a']['n'] == 64 and case['a']['n'] % 64 == 0 and case['a']['n'] % 32 == 0
    assert case['b']['n'] == 65 and case['b']['n'] % 64 == 1 and case['b']['n'] % 32 == 1
    assert case['c']['n'] == 259 and case['c']['n'] % 64 == 3 and case['c']['n'] % 32 == 3
    assert case['d']['n'] == 1030 and case['d']['n'] % 64 == 6 and case['d']['n'] % 32 == 6
    assert case['e']['n'] == 2048 and case['e']['n'] % 64 == 0
    assert (case['e']['n'] + 1) * case['e']['n'] > 4.19e6
    assert (case['g']['n'], case['g']['m'], case['g']['fading']) == (131, 0, None)
    # device indexing
    for k in ('f_rayleigh', 'f_rician'):
        c = case[k]
        tx, rx = c['tx'], c['rx']
        assert (c['n'], c['d']) == (70, 65535) and clu.TOP_DEVICE == 65534 and clu.TOP_DEVICE in tx
        assert (tx >= 32768).sum() >= 5 and (rx >= 32768).sum() >= 5
        assert np.bitwise_or.reduce(tx) == 0xFFFF == np.bitwise_or.reduce(rx)          # every bit of both halves of u | v << 16
        assert len(set(tx[clu.SHARED_TX])) == 1 and len(tx[clu.SHARED_TX]) >= 2
        assert len(set(rx[clu.SHARED_RX])) == 1 and len(rx[clu.SHARED_RX]) >= 2
        assert not set(tx) & set(rx)                                                   # no pair at distance 0
        assert len(set(tx)) == c['n'] - len(tx[clu.SHARED_TX]) + 1 and len(set(rx)) == c['n'] - len(rx[clu.SHARED_RX]) + 1
        for col in ('a_tx', 'a_rx', 'expo'):                                           # by device: no two links read one value
            assert len(set(c[col][np.unique(tx)])) == len(set(tx)) and len(set(c[col][np.unique(rx)])) == len(set(rx))
            assert not np.array_equal(c[col][tx], c[col][:c['n']]) and not np.array_equal(c[col][tx], c[col][rx])
    for k in ('g', 'h'):
        c = case[k]
        assert c['d'] == 193 and len(set(c['a_tx'])) == len(set(c['a_rx'])) == len(set(c['expo'])) == 193
        assert (20 <= c['a_tx']).all() and (c['a_tx'] <= 60).all() and (np.abs(c['a_rx']) <= 10).all()
        assert (2 <= c['expo']).all() and (c['expo'] <= 4).all()
    # case h is case g but for one device of one env
    e, j, i = clu.COINCIDENT
    g, h = case['g'], case['h']
    moved = np.zeros(g['pos'].shape[:2], dtype=bool)
    moved[e, h['tx'][j]] = True
    assert np.array_equal(g['pos'][~moved], h['pos'][~moved]) and np.array_equal(h['pos'][e, h['tx'][j]], h['pos'][e, h['rx'][i]])
    assert e >= 8 and j != i and h['tx'][j] != h['rx'][i] and all(np.array_equal(g[k], h[k]) for k in ('tx', 'rx', 'a_tx', 'a_rx', 'expo'))
    # the per-env clock: pending and running envs in both groups of eight, elapsed >= start, episodes in [1, 1000]
    k = case['c']['clock']
    pending = k['reset'] != 0
    for group in (slice(0, 8), slice(8, 11)):
        assert pending[group].any() and (~pending[group]).any()
    assert (k['elapsed'] >= k['start']).all() and (k['start'][pending] != 0).any() and (1 <= k['episode']).all() and (k['episode'] <= 1000).all()
    episode, t = clu.env_clock(case['c'])
    assert (t[pending] == 0).all() and (t[~pending] >= 1).all() and len(set(episode)) > 8
    assert all(case[n]['clock'] is None for n in case if n != 'c')
    # the shards start inside a group of eight and end in the next
    for name, (lo, hi) in clu.SHARDS.items():
        assert 0 < lo < 8 < hi <= case[name]['b'] and lo % 8 != 0


def test_the_column_restatement_agrees_with_the_oracle_s_median_restatement():
    """table_db_columns on the log-distance columns (a_tx the path-loss constant, a_rx 0, exponent the ple) against table_db, whose
    median is the oracle's own formula: 1e-12 of the entry, scalar and per-env clocks, every fading."""
    from oracle import d2d_oracle as orc
    from sim_util import default_links, random_layout
    b, cues, pairs = 3, 3, 2
    d = 1 + cues + 2 * pairs
    pos = random_layout(np.random.default_rng(5), b, cues, pairs)
    tx, rx, _ = default_links(cues, pairs)
    _, cfgs, is_bs = orc.device_configs(cues, pairs)
    cols = orc.device_columns(cfgs, is_bs)
    shadow_seed, fading_seed = cu.stream_seeds(clu.SEED)
    for ple, fading, m, episode, t in ((2.0, 'rayleigh', 16, 3, 5), (3.5, 'rician', 8, np.array([1, 7, 2]), np.array([0, 4, 9])),
                                       (3.5, None, 32, 0, 0)):
        kw = dict(first_env=clu.FIRST_ENV, episode=episode, t=t, num_sinusoids=m, fading=fading)
        want, want_h2 = cu.table_db(pos, tx, rx, cols, orc.PathLossSpec('log_distance', 2.1, ple=ple), env_seed=clu.SEED, **kw)
        got, got_h2 = cu.table_db_columns(pos, tx, rx, np.full(d, orc.pl_constant_db(2.1, ple)), np.zeros(d), np.full(d, ple),
                                          shadow_seed=shadow_seed, fading_seed=fading_seed, chunk_elems=1, **kw)
        err = np.max(np.abs(got - want) / np.abs(want))
        print(f'ple {ple} {fading} M_s {m}: {err:.3g} of the entry')
        assert err <= 1e-12
        assert (got_h2 is None and want_h2 is None) or np.array_equal(got_h2, want_h2)


# ---------------------------------------------------------------------------------------------- the host side
def test_model_defaults_range_checks_constants_and_seeds():
    from gym_d2d_amd import mobility
    from gym_d2d_amd.path_loss import (FADING_SEED_MIX, SHADOW_SEED_MIX, CostHataPathLoss, LogDistancePathLoss, PathLoss,
                                       SpatialChannelPathLoss)
    m = SpatialChannelPathLoss(2.1)
    assert (m.shadow_std_dB, m.decorrelation_m, m.num_sinusoids, m.fading, m.rician_k_dB, m.seed) == (8.0, 20.0, 16, 'rayleigh', 6.0, None)
    assert m.table_dtype == 'float64' and SpatialChannelPathLoss(2.1, table_dtype='float32').table_dtype == 'float32'
    assert isinstance(m.median_model, LogDistancePathLoss) and isinstance(m, PathLoss)
    for kw in (dict(shadow_std_dB=-1), dict(shadow_std_dB=float('nan')), dict(decorrelation_m=0), dict(num_sinusoids=12),
               dict(num_sinusoids=True), dict(fading='nakagami'), dict(rician_k_dB=float('inf')), dict(seed=-1), dict(seed=1.5),
               dict(table_dtype='float16'), dict(median=3), dict(median=SpatialChannelPathLoss)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            SpatialChannelPathLoss(2.1, **kw)
    sub = type('Sub', (SpatialChannelPathLoss,), dict(num_sinusoids=32, fading=None, median=CostHataPathLoss))   # subclass attributes
    s = sub(2.1)
    assert (s.num_sinusoids, s.fading) == (32, None) and isinstance(s.median_model, CostHataPathLoss)
    m = SpatialChannelPathLoss(2.1, shadow_std_dB=6.0, decorrelation_m=35.0, num_sinusoids=32, fading='rician', rician_k_dB=3.0)
    assert m.constants() == cu.constants(6.0, 35.0, 32, 'rician', 3.0)
    assert SpatialChannelPathLoss(2.1, shadow_std_dB=0.0).constants()[0] == 0
    assert (SHADOW_SEED_MIX, FADING_SEED_MIX) == (cu.SHADOW_SEED_MIX, cu.FADING_SEED_MIX)
    assert len({SHADOW_SEED_MIX, FADING_SEED_MIX, mobility.SEED_MIX, 0}) == 4               # three streams and the env's own
    assert m.stream_seeds(9) == cu.stream_seeds(9) and SpatialChannelPathLoss(2.1, seed=4).stream_seeds(9) == cu.stream_seeds(9, 4)
    with pytest.raises(NotImplementedError, match='no value for one isolated'):
        m(None, None)


@pytest.fixture
def stub(monkeypatch):
    from gym_d2d_amd import _native
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    return RecordingHandle


def test_every_refusal_raises_by_name(stub):
    from gym_d2d_amd.envs import D2DEnv, VecD2DEnv
    from gym_d2d_amd.path_loss import PathLoss, ShadowingPathLoss, SpatialChannelPathLoss
    from gym_d2d_amd.simulator import Simulator

    class PerObject(PathLoss):
        def __call__(self, tx, rx):
            return 100.0
    with pytest.raises(ValueError, match='median=PerObject is not a power law in distance'):
        VecD2DEnv(dict(CFG, path_loss_model=type('A', (SpatialChannelPathLoss,), dict(median=PerObject))), num_envs=2, use_torch=False)
    with pytest.raises(ValueError, match='median=ShadowingPathLoss draws a shadowing of its own'):
        VecD2DEnv(dict(CFG, path_loss_model=type('B', (SpatialChannelPathLoss,), dict(median=ShadowingPathLoss))), num_envs=2,
                  use_torch=False)
    with pytest.raises(ValueError, match='path_loss_model=SpatialChannelPathLoss needs the torch path'):
        VecD2DEnv(dict(CFG, path_loss_model=SpatialChannelPathLoss), num_envs=2, use_torch=False)
    with pytest.raises(ValueError, match='path_loss_model=SpatialChannelPathLoss needs VecD2DEnv'):
        D2DEnv(dict(CFG, path_loss_model=SpatialChannelPathLoss))
    sim = Simulator(dict(CFG, num_envs=2, path_loss_model=SpatialChannelPathLoss))
    assert sim.path_loss_table.route == 'channel'
    sim.set_links(sim.default_link_keys())
    with pytest.raises(ValueError, match='needs an episode clock .* Simulator.step / step_arrays'):
        sim.step_arrays(np.zeros((2, 5), dtype=np.int32))
    one = Simulator(dict(CFG, path_loss_model=SpatialChannelPathLoss))
    from gym_d2d_amd.actions import Action, Actions
    acts = Actions({k: Action(k[0], k[1], one.classify(k[0])[0], 0, 0) for k in one.default_link_keys()})
    with pytest.raises(ValueError, match='needs an episode clock'):
        one.step(acts)


def test_the_routes_that_serve_moving_positions_include_the_channel():
    from types import SimpleNamespace
    from gym_d2d_amd import mobility, sensing
    from gym_d2d_amd.path_loss_table import positions_move_unserved
    sim = SimpleNamespace(path_loss_table=SimpleNamespace(route='channel', law={}), fixed_positions=lambda: (np.zeros(5, np.uint8), np.zeros((5, 2))))
    assert positions_move_unserved(sim, True) is None and mobility.refusal(sim, True) is None
    assert sensing.unserved(sim, True) == ('route', 'channel')


def test_an_env_without_the_model_never_touches_the_library(stub, monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv

    def opened():
        raise AssertionError('libd2d_channel.so was opened by an env without SpatialChannelPathLoss')
    monkeypatch.setattr(_native, 'load_channel_library', opened)
    before = _native.channel_launches
    env = VecD2DEnv(dict(CFG), num_envs=3, use_torch=False)
    env.reset(seed=1)
    for _ in range(3):
        env.step(np.zeros((3, 5), dtype=np.int32))
    assert env._channel is False and env.simulator.path_loss_table.channel is None
    with pytest.raises(ValueError, match='path_loss_db\\(\\) needs path_loss_model=SpatialChannelPathLoss'):
        env.path_loss_db()
    env.close()
    assert _native.channel_launches == before

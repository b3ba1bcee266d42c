"""Target-SINR power control, the part that needs no GPU: the library's exported set, the entry point's refusals, the kernels'
register budget, the refusal texts, the host-side action encoding, known answers of the reference restatement, and the oracle's
side of the GPU tests' ambiguity cap."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import power_control_util as pcu
from oracle import d2d_oracle as orc

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_powerctl_library_exports_exactly_its_header():
    from gym_d2d_amd import _native, build
    lib = _native.load_powerctl_library()
    header = (ROOT / 'include' / 'd2d_powerctl.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_powerctl.so') == declared == {'d2d_power_control', 'd2d_powerctl_last_error'}
    assert set(_native.POWERCTL_SIGNATURES) == declared
    assert len(_native.POWERCTL_SIGNATURES['d2d_power_control'][1]) == 24
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('POWERCTL_LAW_INV_SQUARE', 'POWERCTL_LAW_POWER', 'POWERCTL_LAW_POW_K', 'POWERCTL_MAX_RBS'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_POWERCTL_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    # the law ids are the sensing kernel's: sensing.fold_columns serves both
    assert (_native.POWERCTL_LAW_INV_SQUARE, _native.POWERCTL_LAW_POWER, _native.POWERCTL_LAW_POW_K) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K)
    # built like the other side libraries, and part of the source digest
    assert build.LIBRARIES['powerctl'] == ['d2d_powerctl.hip'] and ROOT / 'include' / 'd2d_powerctl.h' in build.HEADERS
    assert build.lib_path('powerctl') == LIB_DIR / 'libd2d_powerctl.so'


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, max_iters=4)

    def call(ptr=8, target=8, lo=8, hi=8, power=8, sinr=16, iters=24, conv=32, **kw):
        a = dict(ok, **kw)
        _native.power_control(ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'],
                              a['n_rbs'], target, lo, hi, 0, a['max_iters'], 0, power, sinr, iters, conv)
    before = _native.powerctl_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.POWERCTL_MAX_RBS + 1), 'n_rbs'), (dict(law=3), 'law'), (dict(law=-1), 'law'),
                     (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(max_iters=0), 'max_iters'), (dict(max_iters=-3), 'max_iters'),
                     (dict(ptr=0), 'null device pointer'), (dict(target=0), 'null device pointer'), (dict(lo=0), 'null device pointer'),
                     (dict(hi=0), 'null device pointer'), (dict(power=0), 'null device pointer'), (dict(sinr=0), 'null device pointer'),
                     (dict(iters=0), 'null device pointer'), (dict(conv=0), 'null device pointer'), (dict(sinr=8), 'four arrays'),
                     (dict(conv=24), 'four arrays'), (dict(n_links=2048, n_rbs=8192, law=1), '160 KiB')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.powerctl_launches == before
    call(n_envs=0)                                                      # nothing to do: accepted, and still no launch on a device
    assert _native.powerctl_launches == before


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    return SimpleNamespace(path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law={'shadowing': shadowing}),
                           fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))


def test_refusal_texts_name_the_method():
    from gym_d2d_amd import power_control
    assert power_control.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True, False, False]), np.array([[100.1, -20.3], [0, 0], [0, 0]]))
    texts = {'export_actions=True': power_control.refusal(_stub_sim(), False),
             "'link_table'": power_control.refusal(_stub_sim(route='link_table'), True),
             "'per_step'": power_control.refusal(_stub_sim(route='per_step'), True),
             'ShadowingPathLoss': power_control.refusal(_stub_sim(shadowing=True), True),
             'float32 cannot hold': power_control.refusal(pinned, True),
             'torch path': power_control.refusal(_stub_sim(), True, use_torch=False)}
    for needle, text in texts.items():
        assert needle in text and 'power_control()' in text and 'sense()' not in text and 'best_rb()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)


@pytest.fixture
def stub_handle(monkeypatch):
    from gym_d2d_amd import _native
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    opened = []
    monkeypatch.setattr(_native, 'load_powerctl_library', lambda: opened.append(1) or pytest.fail('libd2d_powerctl.so was opened'))
    return opened


def test_an_env_that_does_not_ask_never_opens_the_library(stub_handle):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._powerctl is None and env._power_levels is None and stub_handle == []
    # asking on the NumPy path is refused by name, at the call, still without the library
    with pytest.raises(ValueError, match=r'power_control\(\) needs the torch path'):
        env.power_control(3.0)
    with pytest.raises(ValueError, match=r'power_control\(\) needs the torch path'):
        env.power_control_actions({'cue': 3.0, 'due': 1.0})
    assert stub_handle == [] and env._powerctl is None
    env.close()


@pytest.mark.parametrize('due_min', [0, 5])
@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_power_control_actions_encoding_on_a_stubbed_handle(stub_handle, cue_actions, due_min):
    """6 CUEs + 4 pairs on 5 RBs: 24 CUE power levels, 21 (due_min 0) or 16 (due_min 5) DUE levels.  The solved powers are
    hand-made; power_control() is stubbed.  The decoder takes the level as the dBm (d2d_env.py:94-96 does not add due_min back),
    so the env's own bounds start at 0 whatever due_min is, and decoding the actions gives the solved powers back."""
    torch = pytest.importorskip('torch')
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.power_control import class_bounds, encode_actions
    b, cues, dues, r = 3, 6, 4, 5
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues, 'due_min_tx_power_dBm': due_min}, num_envs=b,
                    use_torch=False, cue_actions=cue_actions)
    levels = np.array([24] * cues + [21 - due_min] * dues)
    p_min, p_max = class_bounds(env.num_pwr_actions, env._cue_kind, cues, dues)
    assert np.array_equal(p_min, np.zeros(n)) and np.array_equal(p_max, levels - 1) and p_min.dtype == p_max.dtype == np.int32
    rng = np.random.default_rng(5 + due_min)
    rb = rng.integers(0, r, (b, n)); power = rng.integers(0, levels, (b, n))
    rb[1, 8] = r + 2                                                    # on no RB: repeats its (out of range) action
    power[0, 6], power[2, 9] = levels[6] - 1, 0                         # the two ends of the DUE alphabet
    env.device = torch.device('cpu')
    env._t = {'rb': torch.as_tensor(rb, dtype=torch.int32)}
    planes = (torch.as_tensor(power, dtype=torch.int32), torch.zeros((b, n)), torch.zeros(b, dtype=torch.int32),
              torch.ones(b, dtype=torch.uint8))
    seen = []
    env.power_control = lambda target, adjustable=None, max_iters=64, out=None, env_mask=None: \
        seen.append((target, adjustable, max_iters)) or planes
    first = 0 if cue_actions == 'agent' else cues
    a = env.power_control_actions(7.5, adjustable='mask', max_iters=9)
    assert seen == [(7.5, 'mask', 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, env.num_agents) == (b, n - first)
    assert np.array_equal(a.numpy(), (rb * levels + power)[:, first:])
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[first:])     # the env's own decode
    assert np.array_equal(got_rb, rb[:, first:]) and np.array_equal(got_pwr, power[:, first:])
    # the function behind it: NumPy planes alike, and a class whose lowest power is not 0
    lo = np.array([0] * cues + [due_min] * dues)
    a_np = encode_actions(rb, power + lo, lo[first:], levels[first:], first)
    assert a_np.dtype == np.int32 and np.array_equal(a_np, a.numpy())
    env.close()


@pytest.fixture(scope='module')
def powerctl_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_powerctl')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_powerctl.hip'), '-save-temps', '-o', 'powerctl.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'powerctl_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out


def test_powerctl_kernels_use_no_scratch_and_spill_nothing(powerctl_kernels):
    """law in {inverse square 0, power 1, pow-k 4}, from the resource summary alone.  The figures of the build this was written
    on: 50 VGPRs for the inverse-square kernel, 52 and 54 for the two power-law ones; LDS is dynamic (see d2d_powerctl.hip)."""
    assert set(powerctl_kernels) == {0, 1, 4}
    for key, k in powerctl_kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_in_the_powerctl_source():
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_powerctl.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code.replace('no atomics', '').replace('free of atomics', '')


# ------------------------------------------------------------------------------------------ known answers of the restatement
def _two_links(dist_own, dist_cross):
    """Two DUE pairs on a line: transmitters dist_cross apart, each receiver dist_own from its transmitter."""
    cols = orc.device_columns(*orc.device_configs(0, 2)[1:])
    pos = np.array([[[0.0, 0.0], [100.0, 0.0], [100.0 + dist_own, 0.0], [100.0 + dist_cross, 0.0], [100.0 + dist_cross + dist_own, 0.0]]])
    tx, rx = np.array([1, 3]), np.array([2, 4])
    return pos, tx, rx, cols, orc.PathLossSpec('log_distance', 2.1, ple=2.0)


def test_a_link_alone_on_its_rb_takes_the_clamped_ceiling_in_one_sweep():
    pos, tx, rx, cols, spec = _two_links(10.0, 300.0)
    zero = np.zeros((1, 2), dtype=np.int64)
    snr0 = orc.step(pos, tx, rx, np.array([[0, 1]]), zero, cols, spec)['snr_db'][0]        # at 0 dBm, nobody else on the RB
    lo, hi = np.array([0, 0]), np.array([20, 20])
    for target in (snr0[0] + 7.3, snr0[0] - 5.0, snr0[0] + 40.0):
        o = pcu.solve(pos, tx, rx, np.array([[0, 1]]), zero + 3, cols, spec, 2, np.full(2, target), lo, hi)
        want = np.clip(np.ceil(target - snr0), lo, hi)
        assert np.array_equal(o.power_dbm[0], want), (target, o.power_dbm, want)
        assert o.converged[0] and o.iters[0] == (1 if want.any() else 0)
        assert np.array_equal(o.after_one[0], want)
        met = o.sinr_db[0] >= target - 1e-9
        assert np.array_equal(met, want < hi) or (want == hi).all() and not met.any()


def test_two_links_on_one_rb_with_infeasible_targets_both_end_at_p_max():
    pos, tx, rx, cols, spec = _two_links(15.0, 25.0)                    # the cross path is about as good as the own one
    lo, hi = np.array([0, 0]), np.array([20, 20])
    o = pcu.solve(pos, tx, rx, np.array([[0, 0]]), np.zeros((1, 2), np.int64), cols, spec, 1, np.full(2, 30.0), lo, hi)
    assert np.array_equal(o.power_dbm[0], hi) and o.converged[0] and 1 <= o.iters[0] <= 21
    assert (o.sinr_db[0] < 30.0).all()
    # an iteration cap below what it takes: not converged, iters == the cap, and the vector after one sweep is kept
    capped = pcu.solve(pos, tx, rx, np.array([[0, 0]]), np.zeros((1, 2), np.int64), cols, spec, 1, np.full(2, 30.0), lo, hi, max_iters=1)
    full = pcu.solve(pos, tx, rx, np.array([[0, 0]]), np.zeros((1, 2), np.int64), cols, spec, 1, np.full(2, 30.0), lo, hi)
    assert (not capped.converged[0]) == (full.iters[0] >= 1) and capped.iters[0] == 1
    assert np.array_equal(capped.power_dbm, full.after_one)
    # a link on no RB and a link that is not adjustable keep their power; the first has no SINR
    o = pcu.solve(pos, tx, rx, np.array([[0, 5]]), np.array([[4, 9]]), cols, spec, 1, np.full(2, 200.0), lo, hi,
                  adjustable=np.array([False, True]))
    assert np.array_equal(o.power_dbm[0], [4, 9]) and np.isnan(o.sinr_db[0, 1]) and np.isfinite(o.sinr_db[0, 0]) and o.iters[0] == 0


# ------------------------------------------------------------------------------------------ the ambiguity cap of the GPU cases
@pytest.mark.parametrize('name', list(pcu.CASES))
def test_oracle_ambiguity_of_the_gpu_cases_stays_inside_the_cap(name):
    """The seeds and targets of the GPU test's oracle comparison, on the oracle alone: at most 25 % of a case's envs are ambiguous
    (power_control_util: an evaluation whose ceiling decides an update lies within W of a whole number), and the cases exercise
    what they are there for."""
    c, o = pcu.make_case(name), pcu.oracle_side(name)
    share = float(o.ambiguous.mean())
    at_max = (o.power_dbm == c.p_max[None])[o.adjustable]
    at_min = (o.power_dbm == c.p_min[None])[o.adjustable]
    print(f'{name}: {share:.2%} of {c.b} envs ambiguous (decisive rule; {np.mean(o.near < pcu.W):.2%} had any evaluation that near); '
          f'sweeps {o.iters.min()}..{o.iters.max()}, converged {o.converged.mean():.0%}; at p_max {at_max.mean():.0%}, at p_min '
          f'{at_min.mean():.0%}')
    assert o.ambiguous.shape == (c.b,) and share <= pcu.CAP and (~o.ambiguous).sum() >= 3
    assert (o.ambiguous <= (o.near < pcu.W)).all()                      # the decisive rule only ever excludes fewer envs
    assert o.converged.all() and o.iters.max() < 64
    assert not at_max.all() and not at_min.all()                        # neither trivial end
    if name != 'n1':
        assert o.iters.max() >= 2 and ((~at_max) & (~at_min)).any()     # interior powers: the ceiling decides something
    if name == pcu.ONE_RB:
        assert (o.iters > 1).any() and o.iters.max() >= 10
    if name in pcu.LARGE:
        # several sweeps, and what they change reaches the upper half of the links: powers that are raised after the first sweep
        # and end strictly between the bounds, at slots and link indices of 1024 and more where the case has them
        later = (o.power_dbm != o.after_one) & (o.power_dbm > c.p_min[None]) & (o.power_dbm < c.p_max[None])
        lo = min(1024, c.n // 2)
        print(f'{name}: {int(later.sum())} links raised after the first sweep to an interior power, {int(later[:, lo:].sum())} of them j >= {lo}')
        assert o.iters.min() >= 3 and later[:, lo:].any(axis=1).all()
    if name.endswith('no_rb'):
        assert (~o.on_rb).sum() == pcu.B and np.isnan(o.sinr_db[~o.on_rb]).all() and np.isfinite(o.sinr_db[o.on_rb]).all()
        assert np.array_equal(o.power_dbm[~o.on_rb], c.pwr[~o.on_rb])

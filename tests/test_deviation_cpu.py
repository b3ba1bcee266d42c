"""Unilateral-deviation gains, the part that needs no GPU: the library's exported set and its place in the build, the entry
points' refusals, the host class on a stub sim (every refusal before the library is opened), the identity the feature rests on and
the properties of the statement on the float64 oracle's planes (deviation_util.by_oracle), and the conditions the GPU cases are there
for, re-derived on the case states."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import deviation_util as du
from test_rb_ascent_cpu import _stub_sim

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_deviate.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_deviate.hip'
PREFIX = ['pos_x', 'pos_y', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'law', 'pow_k', 'n_envs', 'n_dev', 'n_links', 'n_rbs',
          'p_min', 'p_max', 'links', 'n_sel', 'n_levels', 'allowed', 'floor_db']
ARGS = {'d2d_deviation_gains': PREFIX + ['env_mask', 'gain_out', 'hip_stream'],
        'd2d_best_deviation': PREFIX + ['min_gain_mbps', 'env_mask', 'rb_out', 'pwr_out', 'gain_link', 'regret', 'leader', 'hip_stream']}
ORACLE_CASES = [k for k in du.CASES if du.CASES[k]['oracle'] is not None]


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_deviate_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_deviate_library()
    assert _native.side_library('deviate') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_deviate.so') == declared == {'d2d_deviation_gains', 'd2d_best_deviation', 'd2d_deviate_last_error'}
    assert set(_native.DEVIATE_SIGNATURES) == declared and _native.LATER['deviate'] is _native.DEVIATE_SIGNATURES
    # the signatures are the header's, argument for argument
    ctype = {'const float*': _native._P, 'const int32_t*': _native._P, 'const uint8_t*': _native._P, 'const uint32_t*': _native._P,
             'float*': _native._P, 'double*': _native._P, 'int32_t*': _native._P, 'void*': _native._P,
             'int32_t': _native._I, 'int64_t': _native.C.c_int64, 'double': _native.C.c_double}
    for symbol, names in ARGS.items():
        args = re.search(r'^int %s\((.*?)\);' % symbol, header, flags=re.M | re.S).group(1).replace('\n', ' ').split(',')
        assert [a.strip().split()[-1].lstrip('*') for a in args] == names
        assert [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args] == _native.DEVIATE_SIGNATURES[symbol][1]
    for symbol, (res, argtypes) in _native.DEVIATE_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_deviate_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MAX_LINKS', 'MAX_RBS', 'MAX_LEVELS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_DEVIATE_%s (\d+)' % const, header).group(1)) == getattr(_native, 'DEVIATE_' + const), const
    assert _native.DEVIATE_MAX_LDS_BYTES == 160 * 1024 and _native.DEVIATE_MAX_LEVELS == 64 and _native.DEVIATE_MAX_TABLE_BYTES == 8 << 30
    # the LATER rows are in both tables, in one order, and what was in the build keeps its place
    assert build.LATER['deviate'] == ['d2d_deviate.hip'] and list(build.LATER) == list(_native.LATER)
    assert build.COMPLETE == {**build.EVERY, **build.LATER} and list(build.COMPLETE)[:len(build.EVERY)] == list(build.EVERY)
    assert 'deviate' not in build.EVERY and list(build.LATER)[0] == 'rbascent'
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('deviate') == LIB_DIR / 'libd2d_deviate.so' == _native.side_path('deviate')
    assert 'deviate' in build.__doc__ and '4.25' in build.__doc__
    assert _native.deviate_launches >= 0 and callable(_native.deviation_gains) and callable(_native.best_deviation)


def test_a_missing_deviate_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and 'deviate' in build.later_missing(tmp_path)
    build.lib_path('deviate', tmp_path).touch()
    assert 'deviate' not in build.later_missing(tmp_path)
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_deviate\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_deviate_library()


# ------------------------------------------------------------------------------------------ the LDS formula and the entry points
def _gains(ptr=8, links=8, allowed=0, floor=0, mask=0, out=8, **kw):
    from gym_d2d_amd import _native
    a = dict(dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=4, n_rbs=3, n_sel=2, n_levels=4), **kw)
    _native.deviation_gains(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                            ptr, ptr, links, a['n_sel'], a['n_levels'], allowed, floor, mask, out)


def _best(ptr=8, links=8, allowed=0, floor=0, mask=0, min_gain=0.0, out=(16, 24, 32, 40, 48), **kw):
    from gym_d2d_amd import _native
    a = dict(dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=4, n_rbs=3, n_sel=2, n_levels=4), **kw)
    _native.best_deviation(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                           ptr, ptr, links, a['n_sel'], a['n_levels'], allowed, floor, min_gain, mask, *out)


def test_lds_bytes_are_the_headers_formula_at_the_case_shapes_and_on_both_sides_of_the_limit():
    from gym_d2d_amd import _native, deviation
    header = ' '.join(HEADER.read_text().replace(' *', ' ').split())
    assert '80 n_links + has_allowed round16(4 n_links ceil(n_rbs / 32)) + round16(4 ceil(n_links / 32) n_rbs) + 5216' in header
    shapes = [(k['cues'] + k['dues'], k['r']) for k in du.CASES.values()] + [(1, 1), (1000, 64), (1900, 1), (2048, 256)]
    for n, r in shapes:
        for allowed in (False, True):
            want = 80 * n + ((4 * n * ((r + 31) // 32) + 15) // 16 * 16 if allowed else 0) + (4 * ((n + 31) // 32) * r + 15) // 16 * 16 + 5216
            assert deviation.lds_bytes(n, r, allowed) == du.lds_bytes(n, r, allowed) == want, (n, r)
    limit = _native.DEVIATE_MAX_LDS_BYTES
    assert du.lds_bytes(1000, 64) > 64 * 1024 > du.lds_bytes(300, 8)
    before = _native.deviate_launches
    for n, r, allowed in ((1980, 1, 0), (2048, 1, 0), (1600, 400, 0), (1600, 150, 8), (256, 8192, 0)):
        need = du.lds_bytes(n, r, bool(allowed))
        assert need > limit
        for call in (_gains, _best):
            with pytest.raises(_native.NativeError, match=rf'n_links and n_rbs need {need} bytes of LDS, more than the 163840 a workgroup can have'):
                call(n_links=n, n_rbs=r, allowed=allowed, n_envs=0)
    for n, r, allowed in ((1960, 1, 0), (1600, 50, 0), (512, 1788, 0), (1, 1, 0)):
        assert du.lds_bytes(n, r, bool(allowed)) <= limit
        _gains(n_links=n, n_rbs=r, allowed=allowed, n_envs=0, n_sel=1)
        _best(n_links=n, n_rbs=r, allowed=allowed, n_envs=0, n_sel=1)
    assert _native.deviate_launches == before


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    before = _native.deviate_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=2049), r'n_links must be in \[1, 2048\]'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=8193), 'n_rbs'), (dict(n_envs=-1), 'n_envs'), (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'),
                     (dict(n_sel=0), r'n_sel must be in \[1, n_links\]'), (dict(n_sel=5), 'n_sel'), (dict(n_levels=0), r'n_levels must be in \[1, 64\]'),
                     (dict(n_levels=65), 'n_levels'), (dict(law=3), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(ptr=0), 'null device pointer'), (dict(links=0), 'null device pointer')):
        for call in (_gains, _best):
            with pytest.raises(_native.NativeError, match=text):
                call(**kw)
    with pytest.raises(_native.NativeError, match='null device pointer'):
        _gains(out=0)
    good = (16, 24, 32, 40, 48)
    for z in range(5):
        with pytest.raises(_native.NativeError, match='null device pointer'):
            _best(out=tuple(0 if i == z else v for i, v in enumerate(good)))
    with pytest.raises(_native.NativeError, match='rb_out, pwr_out, gain_link, regret and leader must be five arrays'):
        _best(out=(16, 16, 32, 40, 48))
    with pytest.raises(_native.NativeError, match='must not be the held planes'):
        _best(out=(8, 24, 32, 40, 48))
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(_native.NativeError, match='min_gain_mbps must be finite and >= 0'):
            _best(min_gain=bad)
    for kw in (dict(), dict(allowed=8, floor=8, mask=8), dict(law=2, pow_k=4), dict(law=1), dict(n_levels=64), dict(n_sel=4)):
        _gains(n_envs=0, **kw)                                          # nothing to do: accepted, and no launch on a device
        _best(n_envs=0, **kw)
    assert _native.deviate_launches == before


# ------------------------------------------------------------------------------------------ the host module on a stub sim
@pytest.fixture
def unopened(monkeypatch):
    """Every refusal below is raised before the library is opened, with deviate_launches unchanged."""
    from gym_d2d_amd import _native
    monkeypatch.setattr(_native, 'load_deviate_library', lambda: pytest.fail('libd2d_deviate.so was opened'))
    before = _native.deviate_launches
    yield
    assert _native.deviate_launches == before


def test_refusal_texts_name_deviation_gains_and_it_is_refused_where_rb_ascent_is(unopened):
    from gym_d2d_amd import deviation, rb_ascent, sensing
    assert deviation.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: deviation.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = deviation.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('deviation_gains() ') and 'rb_ascent()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():
        assert rb_ascent.refusal(*args) is not None
    assert rb_ascent.refusal(_stub_sim(), True) is None
    assert len(deviation.REFUSAL) == 5 and deviation.REFUSAL[1] == sensing.REFUSALS['best_rb'][1]
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11     # the shared table is as it was


def _kernel(torch, p_max=(23, 23, 20, 20), **kw):
    from gym_d2d_amd import deviation
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    return deviation.Deviation(_stub_sim(**kw), 4, np.zeros(4, np.int32), np.array(p_max, np.int32), agent, torch, torch.device('cpu'))


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim(unopened):
    import torch
    from gym_d2d_amd import _native, deviation, sensing
    from gym_d2d_amd.deviation import Deviation
    cpu = torch.device('cpu')
    k = _kernel(torch)
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4) and k.law == _native.DEVIATE_LAW_POW_K
    assert len(k.ptrs) == 4 and len(k.raw_launch_args(1, 2, 3, 4)) == 14
    assert k.floor(None, 2).tolist() == [-np.inf] * 4 and k.floor({'cue': 0.0, 'due': -np.inf}, 2).tolist() == [0.0, 0.0, -np.inf, -np.inf]
    assert k.words(None) is None and tuple(k.words(np.ones((4, 4), bool)).shape) == (4, 1)
    # the selection: the agent links by default; ascending, distinct, agent links only
    sel, levels, lmax = k.select(None)
    assert sel.tolist() == [1, 2, 3] and sel.dtype == torch.int32 and levels.tolist() == [24, 21, 21] and lmax == 24
    assert k.select([2, 3])[0].tolist() == [2, 3] and k.select(np.array([2, 3]))[2] == 21 and k.select((1,))[2] == 24
    assert k.select([2, 3])[0] is k.select([2, 3])[0]                   # a repeat is not uploaded again
    for bad in ([], [3, 2], [2, 2], [4], [-1], [1.0], np.array([[1]]), 'x', True, torch.tensor([1, 2])):
        with pytest.raises(ValueError, match='links must be None or ascending, distinct ints'):
            k.select(bad)
    with pytest.raises(ValueError, match=r"links on fixed actions \(cue_actions='traffic'\) .* may not be selected: \[0\]"):
        k.select([0, 2])
    # out=, min_gain, the masks: refused before any launch
    planes = dict(pos_x=torch.zeros(3, 7), pos_y=torch.zeros(3, 7), rb=torch.zeros(3, 4, dtype=torch.int32), pwr=torch.zeros(3, 4, dtype=torch.int32))
    floor = k.floor(None, 2)
    for out in (torch.zeros(3, 3, 4, 23), torch.zeros(3, 3, 4, 24, dtype=torch.float64), torch.zeros(3, 3, 96), [torch.zeros(3, 3, 4, 24)],
                torch.zeros(3, 3, 24, 4).permute(0, 1, 3, 2)):
        with pytest.raises(ValueError, match=r'out must be a contiguous float32 \[3, 3, 4, 24\] tensor'):
            k.gains(planes, None, None, floor, out, 0)
    with pytest.raises(ValueError, match=r'out must be a contiguous float32 \[3, 2, 4, 21\] tensor'):
        k.gains(planes, [2, 3], None, floor, torch.zeros(3, 3, 4, 24), 0)
    i32, f64 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s, dtype=torch.float64))
    good = (i32(3, 4), i32(3, 4), f64(3, 4), f64(3), i32(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4)] * 3 + [(3,)] * 2 and [o.dtype for o in k.outputs(None)] == [o.dtype for o in good]
    for out in (good[:4], (*good[:2], torch.zeros(3, 4), *good[3:]), (good[0], good[0], *good[2:]), good[0]):
        with pytest.raises(ValueError, match=r'out must be \(rb, power_dbm, gain_mbps, regret_mbps, leader\)'):
            k.best(planes, None, None, floor, 0.0, out, 0)
    for bad in (-1, -0.5, float('nan'), float('inf'), True, '1', None):
        with pytest.raises(ValueError, match='min_gain_mbps must be a finite number >= 0'):
            k.best(planes, None, None, floor, bad, None, 0)
    for call in (lambda **kw: k.gains(planes, None, kw.get('allowed'), floor, None, 0, kw.get('env_mask')),
                 lambda **kw: k.best(planes, None, kw.get('allowed'), floor, 0.0, None, 0, kw.get('env_mask'))):
        with pytest.raises(ValueError, match=r'allowed must be bool \[4, 4\]'):
            call(allowed=np.ones((4, 5), bool))
        with pytest.raises(ValueError, match='env_mask must be'):
            call(env_mask=np.ones(4, bool))
    with pytest.raises(ValueError, match='floor_sinr_db must be'):
        k.floor(np.zeros(3), 2)
    # the shapes and classes the object refuses when it is made
    agent = np.array([False, True, True, True])
    with pytest.raises(ValueError, match=r'deviation_gains\(\) serves at most 8192 RBs'):
        _kernel(torch, num_rbs=8193)
    with pytest.raises(ValueError, match='the agent mask does not match the env'):
        Deviation(_stub_sim(), 4, np.zeros(4, np.int32), np.ones(4, np.int32), agent[:3], torch, cpu)
    for lo, hi in ((np.ones(4), np.zeros(4)), (np.zeros(4), np.array([1, 1, 4096, 1])), (np.array([0, 0, -4096, 0]), np.ones(4))):
        with pytest.raises(ValueError, match='the power bounds do not match the env'):
            Deviation(_stub_sim(), 4, lo.astype(np.int32), hi.astype(np.int32), agent, torch, cpu)
    with pytest.raises(ValueError, match=r'deviation_gains\(\) serves at most 64 power levels per link \(D2D_DEVIATE_MAX_LEVELS\), got 65'):
        _kernel(torch, p_max=(23, 23, 64, 20))
    assert _kernel(torch, p_max=(64, 23, 63, 20)).select(None)[2] == 64          # 64 levels; link 0 is never selected

    def wide(n, r, b=3):
        return SimpleNamespace(**{**vars(_stub_sim(num_rbs=r)), 'num_envs': b, 'link_tx': np.ones(n, dtype=np.int64),
                                  'link_rx': np.zeros(n, dtype=np.int64)})
    ones = lambda n: (np.zeros(n, np.int32), np.ones(n, np.int32), np.ones(n, bool))
    with pytest.raises(ValueError, match=rf'deviation_gains\(\) .*1600 links on 400 RBs need {du.lds_bytes(1600, 400)} bytes, more than 163840'):
        Deviation(wide(1600, 400), 1600, *ones(1600), torch, cpu)
    big = Deviation(wide(1600, 100), 1600, *ones(1600), torch, cpu)
    with pytest.raises(ValueError, match=rf'need {du.lds_bytes(1600, 100, True)} bytes with an allowed mask, more than 163840'):
        big.need(True)
    assert big.need(False) == du.lds_bytes(1600, 100) <= 163840
    # the 8 GiB cap names the byte count; a smaller selection passes it (and is refused for its out= only)
    huge = Deviation(wide(1600, 50, b=20000), 1600, *ones(1600), torch, cpu)
    nbytes = 4 * 20000 * 1600 * 50 * 2
    assert nbytes > 8 << 30 and deviation.table_bytes(20000, 1600, 50, 2) == nbytes
    hp = dict(pos_x=torch.zeros(1), pos_y=torch.zeros(1), rb=torch.zeros(1, dtype=torch.int32), pwr=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match=rf'table of {nbytes} bytes \(float32 \[20000, 1600, 50, 2\]\), more than {8 << 30}'):
        huge.gains(hp, None, None, huge.floor(None, 0), None, 0)
    with pytest.raises(ValueError, match=r'out must be a contiguous float32 \[20000, 2, 50, 2\] tensor'):
        huge.gains(hp, [5, 9], None, huge.floor(None, 0), torch.zeros(1), 0)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch, unopened):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._deviation is None
    for call in (lambda: env.deviation_gains(), lambda: env.best_deviation(), lambda: env.best_deviation_actions()):
        with pytest.raises(ValueError, match=r'deviation_gains\(\) needs the torch path'):
            call()
    assert env._deviation is None
    for name, needles in (('deviation_gains', ('COMA', 'Nash', 'safe-action mask', 'product', r'\+0\.0', 'rb \\* levels \\+ level', '8 GiB',
                                               'nothing is synchronised')),
                          ('best_deviation', ('lowest power', 'regret_mbps', 'leader', '-1', 'same words', 'nothing is synchronised')),
                          ('best_deviation_actions', ('STEEPEST-ASCENT', 'leader', 'repeats'))):
        doc = ' '.join(getattr(VecD2DEnv, name).__doc__.split())
        for needle in needles:
            assert re.search(needle, doc), (name, needle)
    env.close()


def test_best_deviation_actions_move_the_leader_alone_on_a_stubbed_handle(monkeypatch, unopened):
    torch = pytest.importorskip('torch')
    from gym_d2d_amd import _native, deviation
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    b, cues, dues, r = 3, 6, 4, 5
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b, use_torch=False, cue_actions='traffic')
    levels = np.array([24] * cues + [21] * dues)
    rng = np.random.default_rng(8)
    rb, power = rng.integers(0, r, (b, n)), rng.integers(0, levels, (b, n))
    best_rb, best_p = rng.integers(0, r, (b, n)), rng.integers(0, levels, (b, n))
    leader = np.array([cues + 1, -1, n - 1])
    env.device = torch.device('cpu')
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32)
    env._t = {'rb': i32(rb), 'pwr': i32(power)}
    seen = []
    env.best_deviation = lambda *a: seen.append(a) or deviation.BestDeviationResult(i32(best_rb), i32(best_p), None, None, i32(leader))
    actions = env.best_deviation_actions([7, 9], None, 3.0, 0.25)
    assert seen == [([7, 9], None, 3.0, 0.25)] and actions.dtype == torch.int32 and tuple(actions.shape) == (b, dues)
    want = (rb * levels + power)[:, cues:]
    for e in (0, 2):
        want[e, leader[e] - cues] = best_rb[e, leader[e]] * 21 + best_p[e, leader[e]]
    assert np.array_equal(actions.numpy(), want)
    env.close()


# ------------------------------------------------------------------------------------------ the statement on the float64 oracle
@pytest.mark.parametrize('floors', ['none', 'below'])
@pytest.mark.parametrize('case', ORACLE_CASES)
def test_gain_is_the_change_of_the_total_and_the_held_action_holds_plus_zero(case, floors):
    """The identity the feature rests on: groups do not interact, so total(s^(r,q)) - total(s), summed over ALL links, is gain."""
    res = du.oracle_side(case, floors)
    on = np.array([[row.on for row in rows] for rows in res.rows])
    assert on.any()
    err = np.abs(res.delta - res.gain) / res.total[:, None, None, None]
    assert err[on].max() <= 1e-9, err[on].max()
    for e, rows in enumerate(res.rows):
        for a, row in enumerate(rows):
            if row.on:
                assert row.open[row.held] and res.table[e, a][row.held] == 0.0 and not np.signbit(res.table[e, a][row.held])
                assert np.isfinite(res.table[e, a]).sum() == row.open.sum()
            else:
                assert np.isinf(res.table[e, a]).all() and res.gain_link[e, res.links[a]] == 0.0
    # the marks leave at least 99 % of the case's entries to the comparison: a condition of the GPU cross-check, held here
    assert res.near.mean() <= du.MARK_CAP, res.near.mean()


@pytest.mark.parametrize('case', ORACLE_CASES)
def test_openness_is_monotone_under_a_raised_floor(case):
    """Floors close entries and never open one; and a floor raised by 5 dB closes more, on every RB whose members - link i among
    them - meet the raised floor in the held state.  (A member that meets the low floor and starts under the raised one is freed
    by it: "a link already under its floor constrains nothing".  Those RBs are left out, and some must remain.)"""
    c = du.make_case(case)
    envs, links = du.oracle_links(case)
    low_f, high_f = {'cue': -5.0, 'due': 0.0}, du.FLOOR_SETTINGS['below']
    free, low, high = du.oracle_side(case, 'none'), du.by_oracle(c, envs, links, None, low_f), du.oracle_side(case, 'below')
    levels_open = (np.arange(free.lmax)[None, :] < (c.p_max - c.p_min + 1)[links][:, None])[None, :, None, :]
    on = np.array([[row.on for row in rows] for rows in free.rows])[:, :, None, None]
    assert np.array_equal(free.open, np.broadcast_to(levels_open & on, free.open.shape))    # no floors, no mask: every level of a link on an RB
    assert not (low.open & ~free.open).any() and not (high.open & ~free.open).any()
    assert (low.open != free.open).any() and (high.open != free.open).any()
    fh = du.floor_vector(high_f, c.cues, c.dues).astype(np.float64)
    compared = 0
    for x, e in enumerate(envs):
        now = du.oracle_planes(c, e, c.rb[e][None, :], c.pwr[e][None, :])[0][0]
        meets = now >= fh
        for a, i in enumerate(links):
            if not free.rows[x][a].on:
                continue
            w = c.rb[e][None, :] == np.arange(c.r)[:, None]
            w[:, i] = True
            sound = (meets[None, :] | ~w).all(axis=1)                    # [R]: every member of group(r) u {i} meets the raised floor now
            compared += int(sound.sum())
            assert not (high.rows[x][a].open & ~low.rows[x][a].open)[sound].any()
    assert compared > 0 or case in ('d40_r2', 'd300_r8')                 # (in a group of forty somebody always starts under 5 dB)


@pytest.mark.parametrize('min_gain', [0.0, 0.5])
@pytest.mark.parametrize('case', ORACLE_CASES)
def test_best_deviation_is_the_argmax_of_the_table_under_the_tie_rule(case, min_gain):
    c = du.make_case(case)
    envs, links = du.oracle_links(case)
    res = du.oracle_side(case, 'below') if min_gain == 0.0 else du.by_oracle(c, envs, links, None, du.FLOOR_SETTINGS['below'], min_gain)
    rb, pwr = c.rb[envs], c.pwr[envs]
    held_back = 0
    for e in range(len(envs)):
        for a, i in enumerate(links):
            row, best = res.rows[e][a], None
            for l in range(res.lmax):                                   # the lowest power first, then the lowest RB: a strict maximum
                for r in range(c.r):
                    if row.on and row.open[r, l] and (r, l) != row.held and not np.isnan(row.gain[r, l]) \
                            and (best is None or row.gain[r, l] > best[2]):
                        best = (r, l, row.gain[r, l])
            if best is not None and best[2] > min_gain:
                assert (res.rb_out[e, i], res.pwr_out[e, i], res.gain_link[e, i]) == (best[0], c.p_min[i] + best[1], best[2])
            else:
                held_back += best is not None
                assert (res.rb_out[e, i], res.pwr_out[e, i], res.gain_link[e, i]) == (rb[e, i], pwr[e, i], 0.0)
        others = np.setdiff1d(np.arange(c.n), links)
        assert np.array_equal(res.rb_out[e, others], rb[e, others]) and (res.gain_link[e, others] == 0.0).all()
        top = res.gain_link[e].max()
        assert res.regret[e] == top and res.leader[e] == (-1 if top == 0.0 else int(np.nonzero(res.gain_link[e] == top)[0][0]))
    if min_gain > 0.0 and case in ('d50_r25', 'd300_r8', 'd40_r2'):
        assert held_back > 0                                            # half a Mbps holds some links back


# ------------------------------------------------------------------------------------------ what the cases are there for
def test_the_cases_have_what_they_claim():
    laws = [du.LAWS[k['law']] for k in du.CASES.values()]
    assert all(laws.count(law) >= 2 for law in (0, 1, 2))               # each of the three laws on at least two shapes
    shapes = {(k['b'], k['cues'], k['dues'], k['r']) for k in du.CASES.values()}
    assert shapes == {(4, 3, 3, 4), (4, 25, 25, 25), (3, 65, 65, 70), (2, 16, 24, 1), (2, 16, 24, 2), (2, 8, 8, 8), (2, 100, 200, 8)}
    sizes = {}
    for name in du.CASES:
        c = du.make_case(name)
        on = (c.rb >= 0) & (c.rb < c.r)
        sizes[name] = max(np.bincount(c.rb[e][on[e]], minlength=c.r).max() for e in range(c.b))
        assert ((c.pwr >= c.p_min) & (c.pwr <= c.p_max)).all()          # the held powers lie inside the alphabets
        assert (~on).any() == (name == 'd50_r25')                       # a link on no RB, made the way the RB ascent's tests make one
        assert du.lds_bytes(c.n, c.r, True) <= 163840
    assert sizes['d40_r1'] == 40 and sizes['d40_r2'] > 32 and sizes['d300_r8'] > 32
    c = du.make_case('d16_r8_lv')
    assert set(c.levels) == {64, 1}
    c = du.make_case(du.SUBSET_CASE)
    assert (c.r + 31) // 32 == 3 and c.r % 32 != 0 and c.n * c.r * 24 > 16 * 4096
    c = du.make_case('d300_r8')
    assert -(-c.n // max(1, -(-4096 // (c.r * 24)))) > 1               # more than one workgroup per env


@pytest.mark.parametrize('case', ORACLE_CASES)
def test_some_link_starts_under_its_floor_and_some_entries_tie_between_two_rbs(case):
    c = du.make_case(case)
    envs, links = du.oracle_links(case)
    fl = du.floor_vector(du.FLOOR_SETTINGS['below'], c.cues, c.dues).astype(np.float64)
    under = False
    for e in envs:
        sinr, _ = du.oracle_planes(c, e, c.rb[e][None, :], c.pwr[e][None, :])
        on = (c.rb[e] >= 0) & (c.rb[e] < c.r)
        under |= bool((sinr[0][on] < fl[on]).any())
    assert under
    if case == du.SUBSET_CASE:                                           # 130 links on 70 RBs leave RBs empty: a link gains the same on each
        res = du.oracle_side(case, 'none')
        tied = 0
        for e, rows in enumerate(res.rows):
            empty = np.bincount(c.rb[envs[e]], minlength=c.r)[:c.r] == 0
            assert empty.sum() >= 2
            for a, row in enumerate(rows):
                i = links[a]
                best = (res.rb_out[e, i], res.pwr_out[e, i] - c.p_min[i])
                same = np.nonzero(row.open[:, best[1]] & (row.gain[:, best[1]] == row.gain[best]))[0]
                if len(same) >= 2:
                    tied += 1
                    assert best[0] == same.min()                        # the lowest RB of a tie
        assert tied > 0

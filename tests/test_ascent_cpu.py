"""Sum-capacity power ascent, the part that needs no GPU: the library's exported set and its place in the build, the entry point's
refusals, the host class on a stub sim, the properties of the float64 restatement (ascent_util.ascent_ref), and the conditions the
GPU cases are there for, re-derived on the restatement."""
import itertools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import ascent_util as au
import power_control_util as pcu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_ascent.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_ascent.hip'


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_ascent_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_ascent_library()
    assert _native.side_library('ascent') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_ascent.so') == declared == {'d2d_power_ascent', 'd2d_ascent_last_error'}
    assert set(_native.ASCENT_SIGNATURES) == declared and _native.GROWING['ascent'] is _native.ASCENT_SIGNATURES
    # the signature is the header's, argument for argument
    ctype = {'const float*': _native._P, 'const int32_t*': _native._P, 'const uint8_t*': _native._P, 'float*': _native._P,
             'int32_t*': _native._P, 'uint8_t*': _native._P, 'void*': _native._P, 'int32_t': _native._I, 'int64_t': _native.C.c_int64,
             'double': _native.C.c_double}
    args = re.search(r'^int d2d_power_ascent\((.*?)\);', header, flags=re.M | re.S).group(1)
    names = [a.strip().split()[-1].lstrip('*') for a in args.replace('\n', ' ').split(',')]
    kinds = [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args.replace('\n', ' ').split(',')]
    assert kinds == _native.ASCENT_SIGNATURES['d2d_power_ascent'][1] and len(kinds) == 29
    # the prefix is PairKernel.raw_launch_args with capacity=True, then the issue's order
    assert names == ['pos_x', 'pos_y', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'law', 'pow_k', 'n_envs', 'n_dev',
                     'n_links', 'n_rbs', 'p_min', 'p_max', 'adjustable', 'floor_db', 'start', 'min_gain_mbps', 'max_rounds', 'env_mask',
                     'power_dbm', 'sinr_db', 'capacity_mbps', 'rounds', 'moves', 'converged', 'hip_stream']
    for symbol, (res, argtypes) in _native.ASCENT_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_ascent_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'START_HELD', 'START_MIN', 'START_MAX', 'MAX_LINKS', 'MAX_RBS', 'MAX_LEVELS',
                  'MAX_ROUNDS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_ASCENT_%s (\d+)' % const, header).group(1)) == getattr(_native, 'ASCENT_' + const), const
    assert _native.ASCENT_MAX_LDS_BYTES == 160 * 1024 and _native.ASCENT_MAX_LEVELS == 64 and _native.ASCENT_MAX_ROUNDS == 4096
    # the table behind WHOLE: in the build, the digest and the headers, compiled and linked behind everything else
    assert 'ascent' in build.GROWING and 'ascent' in _native.GROWING and set(build.GROWING) == set(_native.GROWING)
    assert build.GROWING['ascent'] == ['d2d_ascent.hip']
    assert list(build.EVERY)[:len(build.WHOLE)] == list(build.WHOLE) and build.EVERY == {**build.WHOLE, **build.GROWING}
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('ascent') == LIB_DIR / 'libd2d_ascent.so' == _native.side_path('ascent')
    assert 'ascent' in build.__doc__ and 'GROWING' in build.__doc__
    assert 'ascent' not in build.WHOLE


def test_a_missing_ascent_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.growing_missing() == [] and build.growing_missing(tmp_path) == ['ascent']
    build.lib_path('ascent', tmp_path).touch()
    assert build.growing_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'growing_missing', lambda lib_dir=build.LIB_DIR: ['ascent'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built() and not build.addons_missing() \
        and not build.families_missing() and not build.extras_missing() and not build.exact_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_ascent\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_ascent_library()


# ------------------------------------------------------------------------------------------ the LDS formula and the entry point
def _header_lds(n, r, power_law):
    """The formula as include/d2d_ascent.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    n4 = (n + 3) // 4 * 4
    return 48 * n + (r16(8 * n) if power_law else 0) + 20 * n4 + r16(4 * (r + 1)) + 64


def test_lds_bytes_are_the_headers_formula_and_the_readme_states_the_largest_shape():
    from gym_d2d_amd import _native, power_ascent
    assert '48 n_links + has_power_law round16(8 n_links) + 20 n4 + round16(4 (n_rbs + 1)) + 64' in HEADER.read_text()
    for n, r in ((1, 1), (37, 5), (300, 7), (1000, 64), (2048, 256), (2047, 8192)):
        for power_law in (False, True):
            assert power_ascent.lds_bytes(n, r, power_law) == _header_lds(n, r, power_law), (n, r)
    limit = _native.ASCENT_MAX_LDS_BYTES
    assert _header_lds(1000, 64, True) > 64 * 1024 > _header_lds(300, 7, True)
    # what the README row states: every N up to 2048 on up to 2031 RBs (6127 with the inverse-square law), 1720 links on 8192 RBs
    assert _header_lds(2048, 2031, True) <= limit < _header_lds(2048, 2032, True)
    assert _header_lds(2048, 6127, False) <= limit < _header_lds(2048, 6128, False)
    assert _header_lds(1720, 8192, True) <= limit < _header_lds(1724, 8192, True)
    readme = (ROOT / 'README.md').read_text()
    assert '2048 links on up to 2031 RBs' in readme and '1720 links on 8192 RBs' in readme


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, start=0, min_gain=0.0, max_rounds=4)

    def call(ptr=8, lo=8, hi=8, adj=0, floor=0, mask=0, out=(8, 16, 24, 32, 40, 48), **kw):
        a = dict(ok, **kw)
        _native.power_ascent(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                             lo, hi, adj, floor, a['start'], a['min_gain'], a['max_rounds'], mask, *out)
    before = _native.ascent_launches
    big = _header_lds(2048, 2032, True)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.ASCENT_MAX_LINKS + 1), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=_native.ASCENT_MAX_RBS + 1), 'n_rbs'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'), (dict(max_rounds=0), r'max_rounds must be in \[1, 4096\]'),
                     (dict(max_rounds=4097), 'max_rounds'), (dict(max_rounds=-2), 'max_rounds'), (dict(start=3), 'unknown start'),
                     (dict(start=-1), 'unknown start'), (dict(min_gain=-0.5), 'min_gain_mbps must be finite and >= 0'),
                     (dict(min_gain=float('nan')), 'min_gain_mbps'), (dict(min_gain=float('inf')), 'min_gain_mbps'),
                     (dict(law=3), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(ptr=0), 'null device pointer'), (dict(lo=0), 'null device pointer'), (dict(hi=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 8 * (i + 1) for i in range(6))), 'null device pointer') for z in range(6)),
                     (dict(out=(8, 8, 24, 32, 40, 48)), 'power_dbm, sinr_db, capacity_mbps, rounds, moves and converged must be six arrays'),
                     (dict(out=(8, 16, 24, 32, 40, 24)), 'must be six arrays'), (dict(out=(8, 16, 24, 40, 40, 48)), 'must be six arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=2032, law=1), rf'n_links and n_rbs need {big} bytes of LDS, more than the 163840 a workgroup can have'),
                     (dict(n_links=2048, n_rbs=6128), 'bytes of LDS'), (dict(n_links=2048, n_rbs=2032, law=1, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(floor=8, adj=8, mask=8), dict(n_links=2048, n_rbs=2031, law=1), dict(n_links=2048, n_rbs=6127),
               dict(max_rounds=4096), dict(start=2, min_gain=3.5)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.ascent_launches == before


def test_the_ascent_touches_no_global_memory_and_places_one_barrier_behind_it():
    """The source between the start of the ascent and the barrier behind it names none of the argument struct's pointers and no
    workgroup barrier; the fence it uses is wavefront-scoped."""
    src = SOURCE.read_text()
    ascent = src[src.index('// ---- the ascent'):src.index('// the one barrier behind the ascent')]
    pointers = re.findall(r'^\s+(?:const )?(?:unsigned char|float|int)\*\s+(\w+);', src[src.index('struct AscentArgs'):src.index('double min_gain;')],
                          flags=re.M)
    assert len(pointers) == 19
    used = set(re.findall(r'\ba\.(\w+)', ascent))
    assert used == {'max_rounds', 'pow_k', 'min_gain'}
    assert ascent.count('__syncthreads()') == 1 and ascent.rstrip().endswith('__syncthreads();')
    assert '__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront")' in ascent
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code.replace('no atomics', '').replace('__ATOMIC_ACQ_REL', '')


# ------------------------------------------------------------------------------------------ the host module on a stub sim
def _stub_sim(route=None, shadowing=False, num_rbs=4):
    from gym_d2d_amd.path_loss_table import NATIVE
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    law = {'a_tx_db': [30.0] * 7, 'a_rx_db': [0.0] * 7, 'exponent': [3.5] * 7, 'shadowing': shadowing}
    return SimpleNamespace(num_envs=3, handle=SimpleNamespace(num_devices=7), config=SimpleNamespace(num_rbs=num_rbs),
                           link_tx=np.asarray([1, 2, 3, 5]), link_rx=np.asarray([0, 0, 4, 6]), _dev_list=[dev] * 7,
                           path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law=law),
                           fixed_positions=lambda: (np.zeros(7, bool), np.zeros((7, 2))))


def test_refusal_texts_name_power_ascent_and_the_pinned_rows_are_unchanged():
    from gym_d2d_amd import power_ascent, power_control, sensing
    assert power_ascent.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: power_ascent.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = power_ascent.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('power_ascent() ') and 'power_control()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where power_control() is
        assert power_control.refusal(*args) is not None
    row = power_ascent.REFUSAL
    assert row[0] == 'power_ascent()' and row[1:3] == sensing.REFUSALS['power_control'][1:3] and row[4] == 'planes'
    assert row[3] != sensing.REFUSALS['power_control'][3] and row[3] in texts['ShadowingPathLoss']
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import _native, power_ascent, sensing
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    lo, hi = np.zeros(4, dtype=np.int32), np.array([23, 23, 20, 20], dtype=np.int32)
    cpu = torch.device('cpu')
    k = power_ascent.PowerAscent(_stub_sim(), 4, lo, hi, agent, torch, cpu)
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4) and k.law == _native.ASCENT_LAW_POW_K
    assert len(k.ptrs) == 4 and tuple(k.cap_cols.shape) == (2, 7)       # opened with capacity=True
    assert len(k.raw_launch_args(1, 2, 3, 4)) == 14
    assert k.adjustable(None).tolist() == [0, 1, 1, 1] and k.adjustable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError, match=r'adjustable must be bool \[4\]'):
        k.adjustable(np.zeros(3, bool))
    assert k.floor(None, 2).tolist() == [-np.inf] * 4 and k.floor(None, 2).dtype == torch.float32
    assert k.floor({'cue': 0.0, 'due': -np.inf}, 2).tolist() == [0.0, 0.0, -np.inf, -np.inf] and k.floor(-7.0, 2) is k.floor(-7.0, 2)
    for bad in (float('nan'), {'cue': 1.0}, [1.0, 2.0], torch.zeros(3)):
        with pytest.raises(ValueError, match='floor_sinr_db'):
            k.floor(bad, 2)
    i32, f32, u8 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    good = (i32(3, 4), f32(3, 4), f32(3, 4), i32(3), i32(3), u8(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4)] * 3 + [(3,)] * 3
    assert [o.dtype for o in k.outputs(None)] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8]
    planes = dict(pos_x=f32(3, 7), pos_y=f32(3, 7), rb=i32(3, 4), pwr=i32(3, 4))
    adj, floor = k.adjustable(None), k.floor(None, 2)
    before = _native.ascent_launches
    shared = i32(3)
    for out in (good[:5], (*good[:3], shared, shared, good[5]), (*good[:5], i32(3)), (good[0], f32(3, 5), *good[2:]), good[0],
                (good[0], f32(3, 8)[:, ::2], *good[2:])):
        with pytest.raises(ValueError, match=r'out must be \(power_dbm, sinr_db, capacity_mbps, rounds, moves, converged\)'):
            k.solve(planes, adj, floor, 'held', 0.0, 16, out, 0)
    for bad in ('top', 'HELD', None, 0, ''):
        with pytest.raises(ValueError, match=r"start must be one of 'held', 'min', 'max'"):
            k.solve(planes, adj, floor, bad, 0.0, 16, None, 0)
    for bad in (-0.5, float('nan'), float('inf'), -1, True, '1', None):
        with pytest.raises(ValueError, match='min_gain_mbps must be a finite number >= 0'):
            k.solve(planes, adj, floor, 'held', bad, 16, None, 0)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match=r'max_rounds must be an int in \[1, 4096\]'):
            k.solve(planes, adj, floor, 'held', 0.0, bad, None, 0)
    with pytest.raises(ValueError, match='env_mask must be'):
        k.solve(planes, adj, floor, 'held', 0.0, 16, None, 0, env_mask=np.ones(4, bool))
    assert _native.ascent_launches == before
    # the shapes the object refuses when it is made
    with pytest.raises(ValueError, match=r'power_ascent\(\) serves at most 8192 RBs'):
        power_ascent.PowerAscent(_stub_sim(num_rbs=8193), 4, lo, hi, agent, torch, cpu)
    with pytest.raises(ValueError, match='the power bounds do not match the env'):
        power_ascent.PowerAscent(_stub_sim(), 4, lo, hi[:3], agent, torch, cpu)
    with pytest.raises(ValueError, match='the power bounds do not match the env'):
        power_ascent.PowerAscent(_stub_sim(), 4, hi, lo, agent, torch, cpu)                 # p_min > p_max
    with pytest.raises(ValueError, match='the power bounds do not match the env'):
        power_ascent.PowerAscent(_stub_sim(), 4, lo, np.array([23, 23, 20, 4096], np.int32), agent, torch, cpu)
    with pytest.raises(ValueError, match=r'at most 64 levels \(D2D_ASCENT_MAX_LEVELS\), got 65'):
        power_ascent.PowerAscent(_stub_sim(), 4, lo, np.array([23, 23, 20, 64], np.int32), agent, torch, cpu)
    power_ascent.PowerAscent(_stub_sim(), 4, lo, np.array([99, 23, 20, 63], np.int32), agent, torch, cpu)      # link 0 never takes a turn
    wide = SimpleNamespace(**{**vars(_stub_sim(num_rbs=2032)), 'link_tx': np.ones(2048, dtype=np.int64), 'link_rx': np.zeros(2048, dtype=np.int64)})
    with pytest.raises(ValueError, match=rf'2048 links on 2032 RBs need {_header_lds(2048, 2032, True)} bytes, more than 163840'):
        power_ascent.PowerAscent(wide, 2048, np.zeros(2048, np.int32), np.full(2048, 20, np.int32), np.ones(2048, bool), torch, cpu)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_ascent_library', lambda: pytest.fail('libd2d_ascent.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._ascent is None
    for call in (lambda: env.power_ascent(), lambda: env.power_ascent(None, 0.0, 'max'), lambda: env.power_ascent_actions()):
        with pytest.raises(ValueError, match=r'power_ascent\(\) needs the torch path'):
            call()
    assert env._ascent is None
    env.close()


def test_power_ascent_actions_encode_the_solved_powers_on_a_stubbed_handle(monkeypatch):
    torch = pytest.importorskip('torch')
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from oracle import d2d_oracle as orc
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    b, cues, dues, r = 3, 6, 4, 5
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b, use_torch=False, cue_actions='traffic')
    levels = np.array([24] * cues + [21] * dues)
    rng = np.random.default_rng(8)
    rb, power = rng.integers(0, r, (b, n)), rng.integers(0, levels, (b, n))
    env.device = torch.device('cpu')
    env._t = {'rb': torch.as_tensor(rb, dtype=torch.int32)}
    seen = []
    env.power_ascent = lambda *a: seen.append(a) or (torch.as_tensor(power, dtype=torch.int32), None, None, None, None, None)
    a = env.power_ascent_actions('mask', {'cue': 0.0, 'due': 5.0}, 'max', 0.05, 9)
    assert seen == [('mask', {'cue': 0.0, 'due': 5.0}, 'max', 0.05, 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()


# ------------------------------------------------------------------------------------------ the restatement's properties
@pytest.mark.parametrize('name,floors,start', [('n37_r5', False, 'held'), ('n37_r5', True, 'held'), ('n37_r5', True, 'max'),
                                               ('n50_r6_hata', False, 'held'), ('n20_r64', False, 'held')])
def test_every_move_raises_its_groups_total_and_a_met_floor_is_kept(name, floors, start):
    case, b, every = au.CASES[name]
    c = pcu.make_case(case)
    ref = au.reference(name, floors, start)
    assert len(ref.raised) == ref.moves.sum() > 0
    assert all(after > before for _, _, before, after in ref.raised)
    if floors:
        # float64 on both sides and the same oracle: a link that meets its floor at the start meets it at the end, exactly
        fl = au.floor_vector(au.FLOORS, c.cues, c.dues).astype(np.float64)
        from oracle import d2d_oracle as orc
        for x in range(b):
            s0, s1 = (orc.step(c.pos[x][None], c.tx, c.rx, c.rb[x][None], np.asarray(p[x])[None], c.cols, c.spec)['sinr_db'][0]
                      for p in (ref.start, ref.power_dbm))
            met = s0 >= fl
            assert met.any() and (s1[met] >= fl[met] - 1e-9).all()


def test_solving_the_groups_one_at_a_time_gives_the_same_powers_and_the_counts_combine():
    c = pcu.make_case('n37_r5')
    envs = np.arange(4)
    for floors, max_rounds in ((None, 16), (au.FLOORS, 4)):
        whole = au.ascent_ref(c, envs, None, floors, 'held', 0.0, max_rounds)
        power = np.array(c.pwr[:4], dtype=np.int64)
        rounds, moves, conv = np.zeros(4, int), np.zeros(4, int), np.ones(4, bool)
        for r in range(c.r):
            for x in envs:
                members = c.rb[x] == r
                if not members.any():
                    continue
                part = au.ascent_ref(c, [x], members, floors, 'held', 0.0, max_rounds)
                power[x, members] = part.power_dbm[0, members]
                assert np.array_equal(part.power_dbm[0, ~members], c.pwr[x, ~members])
                rounds[x], moves[x], conv[x] = max(rounds[x], part.rounds[0]), moves[x] + part.moves[0], conv[x] and part.converged[0]
        assert np.array_equal(power, whole.power_dbm)
        assert np.array_equal(rounds, whole.rounds) and np.array_equal(moves, whole.moves) and np.array_equal(conv, whole.converged)
        if max_rounds == 4:
            assert (~whole.converged).any() and (whole.rounds[~whole.converged] == 4).all()


def _tiny(seed, groups):
    """A case of a few links with at most 4 levels each: `groups` lists the group sizes, one RB each."""
    n = sum(groups)
    cues = 1
    dues = n - cues
    rng = np.random.default_rng(seed)
    from sim_util import default_links, random_layout
    pos = random_layout(rng, 1, cues, dues, cell_radius=200.0)
    tx, rx, _ = default_links(cues, dues)
    rb = np.repeat(np.arange(len(groups)), groups)[None, :]
    p_min = rng.integers(0, 18, n)
    p_max = p_min + rng.integers(0, 4, n)                                # 1 to 4 levels
    from oracle import d2d_oracle as orc
    return SimpleNamespace(name=f'tiny{seed}', cues=cues, dues=dues, n=n, r=len(groups), pos=pos, rb=rb, pwr=rng.integers(p_min, p_max + 1)[None, :],
                           tx=tx, rx=rx, p_min=p_min, p_max=p_max, spec=orc.PathLossSpec('log_distance', 2.1, ple=2.0),
                           cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


def _group_total(c, members, p):
    return float(au.sequential_sum(au.group_tables(c, 0, members, p, 0, np.array([p[members[0]]]))[1], axis=1)[0])


def test_tiny_cases_end_in_a_coordinatewise_optimum_at_most_the_brute_force_one():
    alone = 0
    for seed in range(12):
        groups = [(3, 2, 1), (1, 1, 1), (3, 3), (2, 1)][seed % 4]
        c = _tiny(seed, groups)
        ref = au.ascent_ref(c, [0], None, None, 'held', 0.0, 64)
        assert ref.converged[0]
        p = ref.power_dbm[0]
        for r in range(c.r):
            members = np.nonzero(c.rb[0] == r)[0]
            got = _group_total(c, members, p)
            best = -np.inf
            for combo in itertools.product(*(range(c.p_min[m], c.p_max[m] + 1) for m in members)):
                q = p.copy()
                q[members] = combo
                t = _group_total(c, members, q)
                best = max(best, t)
                if sum(a != b for a, b in zip(combo, p[members])) == 1:
                    assert t <= got                                      # no single link gains by moving: a coordinate-wise optimum
            assert got <= best
            if len(members) == 1:
                assert got == best
                alone += 1
    assert alone >= 12


# ------------------------------------------------------------------------------------------ the GPU cases hold what they are there for
def test_n37_r5_every_env_moves_and_the_rounds_spread_over_3_to_10():
    ref = au.reference('n37_r5')
    print(ref.rounds.tolist(), ref.moves.tolist())
    assert ref.converged.all() and (ref.moves > 0).all()
    assert ref.rounds.min() == 3 and ref.rounds.max() == 10 and len(np.unique(ref.rounds)) >= 5


def test_n37_r5_floors_change_a_choice_in_at_least_half_of_the_envs():
    ref = au.reference('n37_r5', True)
    print(int(ref.floor_changed.sum()), 'of', len(ref.floor_changed))
    assert ref.floor_changed.sum() >= 8
    assert not au.reference('n37_r5').floor_changed.any()


def test_n20_r64_reaches_the_cap_unconverged_in_at_least_one_env():
    ref = au.reference('n20_r64')
    print(ref.rounds.tolist(), ref.converged.astype(int).tolist())
    capped = (ref.rounds == 16) & ~ref.converged
    assert capped.any() and not capped.all()


def test_n96_r1_takes_at_least_3_moving_rounds():
    c = pcu.make_case('n96_r1')
    ref = au.ascent_ref(c, [0])
    print(ref.rounds.tolist(), ref.moves.tolist())
    assert ref.rounds[0] >= 3 and (c.rb[0] == 0).all()


@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False)])
def test_the_reference_alone_stays_inside_the_cap_at_its_own_fixed_point(name, floors):
    """At the restatement's own fixed point the inequality holds with nothing to spare taken (worst <= 0 of the slack) and the share
    of (link, level) checks left out for a SINR within W of a floor or a sensitivity is under the cap."""
    case, b, every = au.CASES[name]
    c = pcu.make_case(case)
    ref = au.reference(name, floors)
    floor = au.FLOORS if floors else None
    chk = au.reference_check(c, np.arange(b), ref.power_dbm, ref.converged, au.adjustable_mask(c.n, every), floor, 0.0, ref.start)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e}')
    assert chk.checks > 1000 and chk.left_out <= au.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 0.0 and chk.floors_kept

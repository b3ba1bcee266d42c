"""Sum-capacity RB ascent on a path-loss table, the part that needs no GPU: the library's exported set and its place in the build,
the entry point's refusals (every one before a launch), the host class on a stub sim, the texts, the LDS formula, rb_ascent()'s
unchanged refusals of the table routes, the properties of the float64 restatement (table_rb_ascent_util.rb_ascent_ref), and the
conditions the GPU cases of test_gpu_table_rb_ascent.py rest on, re-derived on the drawn inputs and the float64 reference alone."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import table_rb_ascent_util as tu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_tabascent.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_tabascent.hip'
ARGS = ['table', 'table_dtype', 'table_rows', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'n_envs', 'n_dev', 'n_links',
        'n_rbs', 'allowed', 'movable', 'floor_db', 'min_gain_mbps', 'max_rounds', 'env_mask', 'gains', 'rb_out', 'sinr_db',
        'capacity_mbps', 'rounds', 'moves', 'converged', 'domain', 'hip_stream']
FORMULA = ('16 n_links + 2 round16(4 n_links) + 8 n4 + has_allowed round16(4 n_links ceil(n_rbs / 32)) '
           '+ round16(4 ceil(n_links / 32) n_rbs) + 112')


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_tabascent_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_tabascent_library()
    assert _native.side_library('tabascent') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_tabascent.so') == declared == {'d2d_table_rb_ascent', 'd2d_tabascent_last_error'}
    assert set(_native.TABASCENT_SIGNATURES) == declared and _native.LATER['tabascent'] is _native.TABASCENT_SIGNATURES
    ctype = {'const void*': _native._P, 'const float*': _native._P, 'const int32_t*': _native._P, 'const uint8_t*': _native._P,
             'const uint32_t*': _native._P, 'float*': _native._P, 'int32_t*': _native._P, 'uint8_t*': _native._P, 'void*': _native._P,
             'int32_t': _native._I, 'int64_t': _native.C.c_int64, 'double': _native.C.c_double}
    args = re.search(r'^int d2d_table_rb_ascent\((.*?)\);', header, flags=re.M | re.S).group(1).replace('\n', ' ').split(',')
    assert [a.strip().split()[-1].lstrip('*') for a in args] == ARGS
    assert [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args] == _native.TABASCENT_SIGNATURES['d2d_table_rb_ascent'][1]
    for symbol, (res, argtypes) in _native.TABASCENT_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_tabascent_last_error(), bytes)
    for const in ('F32', 'F64', 'MAX_LINKS', 'MAX_RBS', 'MAX_ROUNDS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_TABASCENT_%s (\d+)' % const, header).group(1)) == getattr(_native, 'TABASCENT_' + const), const
    # rb_ascent()'s limits, evaluate_table()'s entry types
    assert (_native.TABASCENT_MAX_LINKS, _native.TABASCENT_MAX_RBS, _native.TABASCENT_MAX_ROUNDS, _native.TABASCENT_MAX_LDS_BYTES) == \
        (_native.RBASCENT_MAX_LINKS, _native.RBASCENT_MAX_RBS, _native.RBASCENT_MAX_ROUNDS, _native.RBASCENT_MAX_LDS_BYTES) == \
        (2048, 8192, 4096, 160 * 1024)
    assert (_native.TABASCENT_F32, _native.TABASCENT_F64) == (_native.EVALTAB_F32, _native.EVALTAB_F64)
    # the LATER rows are in both tables, in one order: behind evaltab, in front of goodput, which stays the last row
    order = list(build.LATER)
    assert build.LATER['tabascent'] == ['d2d_tabascent.hip'] and order == list(_native.LATER)
    assert order[0] == 'rbascent' and order[-1] == 'goodput' and order.index('tabascent') == order.index('evaltab') + 1 == len(order) - 2
    assert build.COMPLETE == {**build.EVERY, **build.LATER} and list(build.COMPLETE)[:len(build.EVERY)] == list(build.EVERY)
    assert 'tabascent' not in build.EVERY
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('tabascent') == LIB_DIR / 'libd2d_tabascent.so' == _native.side_path('tabascent')
    assert 'tabascent' in build.__doc__ and '4.27' in build.__doc__
    assert _native.tabascent_launches >= 0 and callable(_native.table_rb_ascent)


def test_a_missing_tabascent_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and 'tabascent' in build.later_missing(tmp_path)
    build.lib_path('tabascent', tmp_path).touch()
    assert 'tabascent' not in build.later_missing(tmp_path)
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_tabascent\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_tabascent_library()


def test_the_source_restates_the_steps_conversion_and_the_turn_loop_writes_no_global_memory():
    src = SOURCE.read_text()
    for name in ('d2d_addon.h', 'd2d_tabascent.h', 'd2d_step_device.h', 'd2d_wave_key.h'):
        assert f'#include "{name}"' in src
    line = '(float)exp2(-0.33219280948873623478703194294894 * x)'
    assert src.count(line) == 1 and line in (SOURCE.parent / 'd2d_evaltab.hip').read_text()
    assert line in (SOURCE.parent / 'd2d_step_device.h').read_text()
    # no atomic operation is called anywhere (the word stands in comments only)
    assert not re.search(r'\batomic\w*\s*\(|__hip_atomic|__atomic', src)
    # between the start of the rounds and the planes behind them the argument struct is read for two scalars only, the result
    # pointers are not there yet, and the two barriers stand behind readfirstlane'd decisions
    loop = src[src.index('// ---- the rounds'):src.index("// ---- evaltab_kernel's planes for the RBs the ascent stopped at")]
    assert set(re.findall(r'\ba\.(\w+)', loop)) == {'max_rounds', 'min_gain'}
    assert loop.count('__syncthreads()') == 2 and loop.count('__builtin_amdgcn_readfirstlane') == 3
    assert 'results_behind_the_loop()' not in loop and 'out.' not in loop
    # the gain block is receiver-major: the walk runs along row m
    assert 'g + (size_t)m * (size_t)N' in src and 'g[(size_t)i * (size_t)N + (size_t)j] = tile[tx][ty + q]' in src


# ------------------------------------------------------------------------------------------ the LDS formula and the entry point
def _header_lds(n, r, allowed=False):
    """The formula as include/d2d_tabascent.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    n4 = (n + 3) // 4 * 4
    return 16 * n + 2 * r16(4 * n) + 8 * n4 + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 112


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, rb_ascent, table_rb_ascent
    header = ' '.join(HEADER.read_text().replace(' *', ' ').split())
    assert FORMULA in header
    for n, r in [(1, 1), (2047, 8), (2048, 256)] + [(c[0] + c[1], c[2]) for c in tu.CASES.values()]:
        for allowed in (False, True):
            assert table_rb_ascent.lds_bytes(n, r, allowed) == tu.lds_bytes(n, r, allowed) == _header_lds(n, r, allowed), (n, r)
            # 24 bytes per link where rb_ascent() has 48 - no coordinates, no exponents - less what two float arrays round up by
            assert rb_ascent.lds_bytes(n, r, False, allowed) - table_rb_ascent.lds_bytes(n, r, allowed) == 24 * n - 2 * (-4 * n % 16)
    limit = _native.TABASCENT_MAX_LDS_BYTES
    assert _header_lds(1000, 320) > 64 * 1024 > _header_lds(300, 7)
    assert _header_lds(2048, 383) <= limit < _header_lds(2048, 384)
    assert _header_lds(128, 8192) <= limit
    assert table_rb_ascent.work_space_bytes(4096, 512) == 4 * 4096 * 512 * 512 == 4294967296        # the 4.3 GB the docstring states
    assert '4.3 GB' in table_rb_ascent.__doc__


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(dtype=0, rows=None, n_envs=2, n_dev=5, n_links=2, n_rbs=3, min_gain=0.0, max_rounds=4)

    def call(ptr=8, allowed=0, movable=0, floor=0, mask=0, gains=64, out=(8, 16, 24, 32, 40, 48, 56), **kw):
        a = dict(ok, **kw)
        _native.table_rb_ascent(ptr, a['dtype'], a['n_links'] if a['rows'] is None else a['rows'], ptr, ptr, ptr, ptr, ptr, ptr,
                                a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'], allowed, movable, floor, a['min_gain'],
                                a['max_rounds'], mask, gains, *out)
    before = _native.tabascent_launches
    big = _header_lds(2048, 384)
    with_mask = _header_lds(2048, 300, True)
    assert with_mask > _native.TABASCENT_MAX_LDS_BYTES >= _header_lds(2048, 300)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=2049), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=8193), r'n_rbs must be in \[1, 8192\]'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'), (dict(max_rounds=0), r'max_rounds must be in \[1, 4096\]'),
                     (dict(max_rounds=4097), 'max_rounds'), (dict(min_gain=-0.5), 'min_gain_mbps must be finite and >= 0'),
                     (dict(min_gain=float('nan')), 'min_gain_mbps'), (dict(min_gain=float('inf')), 'min_gain_mbps'),
                     (dict(dtype=2), 'table_dtype must be'), (dict(dtype=-1), 'table_dtype must be'),
                     (dict(rows=1), r'table_rows must be n_links or n_links \+ 1'), (dict(rows=4), 'table_rows must be'),
                     (dict(ptr=0), 'null device pointer'), (dict(gains=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 8 * (i + 1) for i in range(7))), 'null device pointer') for z in range(7)),
                     (dict(out=(8, 8, 24, 32, 40, 48, 56)), 'must be eight arrays'), (dict(out=(8, 16, 24, 32, 40, 48, 32)), 'must be eight arrays'),
                     (dict(gains=56), 'rb_out, sinr_db, capacity_mbps, rounds, moves, converged, domain and gains must be eight arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=384), rf'n_links and n_rbs need {big} bytes of LDS, more than the 163840 a workgroup can have'),
                     (dict(n_links=2048, n_rbs=300, allowed=8), rf'need {with_mask} bytes of LDS'),
                     (dict(n_links=2048, n_rbs=384, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(allowed=8, movable=8, floor=8, mask=8), dict(n_links=2048, n_rbs=383), dict(rows=3), dict(dtype=1),
               dict(max_rounds=4096), dict(min_gain=3.5), dict(n_links=128, n_rbs=8192)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.tabascent_launches == before


# ------------------------------------------------------------------------------------------ the host module on a stub sim
def _stub_sim(route=None, live=None, num_rbs=4, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    law = {'a_tx_db': [30.0] * 7, 'a_rx_db': [0.0] * 7, 'exponent': [3.5] * 7, 'shadowing': shadowing}
    return SimpleNamespace(num_envs=3, handle=SimpleNamespace(num_devices=7), config=SimpleNamespace(num_rbs=num_rbs),
                           link_tx=np.asarray([1, 2, 3, 5]), link_rx=np.asarray([0, 0, 4, 6]), _dev_list=[dev] * 7,
                           path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law=law, live=live),
                           fixed_positions=lambda: (np.zeros(7, bool), np.zeros((7, 2))))


def test_the_refusal_texts_name_rb_ascent_table_and_rb_ascent_keeps_refusing_the_table_routes_word_for_word():
    from gym_d2d_amd import rb_ascent, sensing, table_evaluate, table_rb_ascent as tra
    # every route, shadowing and export_actions=False are served: the table and the start state may come with the call
    for route in (None, 'device_table', 'link_table', 'array', 'per_step', 'channel'):
        assert tra.refusal(_stub_sim(route), True, True) is None and tra.refusal(_stub_sim(route), False, True) is None
    assert tra.refusal(_stub_sim(shadowing=True), True, True) is None
    assert tra.refusal(_stub_sim(), True, False) == 'rb_ascent_table() needs the torch path (use_torch): its planes are device tensors'
    assert len(tra.ROW) == len(table_evaluate.ROW) == len(sensing.REFUSALS['evaluate']) and 'rb_ascent_table' not in ' '.join(sensing.REFUSALS)
    for route in ('native', 'device_table', 'link_table', 'array', 'per_step', 'channel'):
        text = tra.no_live_table(_stub_sim(route))
        assert text == table_evaluate.no_live_table(_stub_sim(route)).replace('evaluate_table()', 'rb_ascent_table()')
        assert text.startswith('rb_ascent_table() has no live dB table to read on the ') and f"'{route}'" in text and 'pass table=' in text
        assert 'evaluate_table' not in text
    for api in ('rb_ascent_table()', 'rb_ascent_table_actions()'):
        text = tra.no_start_state(api)
        assert text.startswith(api + ' ') and 'rb=' in text and 'power_dbm=' in text and 'export_actions=True' in text
    assert tra.TableRbAscentResult._fields == tu.NAMES
    # rb_ascent() itself: the table routes stay refused, in the words they had
    for route in ('link_table', 'array', 'per_step', 'channel'):
        assert rb_ascent.refusal(_stub_sim(route), True) == (
            f"rb_ascent() does not serve the '{route}' path-loss route (a table, not a law its kernel can evaluate for the RBs no step "
            'has applied); it serves the native power-law models')
    assert rb_ascent.refusal(_stub_sim(shadowing=True), True) == (
        'rb_ascent() does not serve ShadowingPathLoss: a fresh draw per evaluation has no ascent (the capacity a move was made for is '
        'another draw than the one the next link sees)')
    assert rb_ascent.refusal(_stub_sim(), True) is None


def test_the_kernel_object_refuses_bad_arguments_before_a_launch_and_never_opens_the_library(monkeypatch):
    import torch
    from gym_d2d_amd import _native, sensing, table_evaluate, table_rb_ascent as tra
    monkeypatch.setattr(_native, 'load_tabascent_library', lambda: pytest.fail('libd2d_tabascent.so was opened'))
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    cpu = torch.device('cpu')
    live = torch.zeros((3, 5, 4), dtype=torch.float64)
    k = tra.TableRbAscent(_stub_sim('channel', live), 4, agent, torch, cpu)
    assert isinstance(k, table_evaluate.TableEvaluate) and isinstance(k, sensing.PairKernel) and (k.b, k.d, k.n, k.r) == (3, 7, 4, 4)
    assert len(k.ptrs) == 4 and tuple(k.cols.shape) == (3, 7) and tuple(k.cap_cols.shape) == (2, 7) and k.gains is None
    assert k.movable(None).tolist() == [0, 1, 1, 1] and k.movable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError, match=r'movable must be bool \[4\]'):
        k.movable(np.zeros(3, bool))
    assert k.floor(None, 2).tolist() == [-np.inf] * 4 and k.floor({'cue': 0.0, 'due': 5.0}, 2).tolist() == [0.0, 0.0, 5.0, 5.0]
    for bad in (float('nan'), {'cue': 1.0}, [1.0, 2.0], torch.zeros(3)):
        with pytest.raises(ValueError, match='floor_sinr_db'):
            k.floor(bad, 2)
    assert k.words(None) is None and tuple(k.words(np.ones((4, 4), bool)).shape) == (4, 1)
    # the table: the live one, or what TableEvaluate.table() takes
    assert k.table(None)[0] is live and k.table(None)[1:] == (_native.TABASCENT_F64, 5)
    assert k.table(torch.zeros((3, 4, 4)))[1:] == (_native.TABASCENT_F32, 4)
    for bad in (torch.zeros((3, 4, 3)), torch.zeros((3, 6, 4)), torch.zeros((2, 4, 4)), torch.zeros((3, 4, 4), dtype=torch.float16),
                torch.zeros((3, 4, 8))[:, :, ::2], np.zeros((3, 4, 4)), torch.zeros((4, 4))):
        with pytest.raises(ValueError, match='table must be'):
            k.table(bad)
    native = tra.TableRbAscent(_stub_sim(), 4, agent, torch, cpu)
    with pytest.raises(ValueError, match=r"rb_ascent_table\(\) has no live dB table to read on the 'native' path-loss route.*pass table="):
        native.table(None)
    assert native.table(torch.zeros((3, 4, 4)))[2] == 4
    i32, f32, u8 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    rb, pwr = i32(3, 4), i32(3, 4)
    assert k.start(rb, 'rb') is rb
    for bad, name in ((i32(3, 5), 'rb'), (f32(3, 4), 'power_dbm'), (i32(3, 8)[:, ::2], 'rb'), (np.zeros((3, 4), np.int32), 'power_dbm'), (i32(4), 'rb')):
        with pytest.raises(ValueError, match=rf'{name} must be a contiguous int32 tensor \[3, 4\]'):
            k.start(bad, name)
    good = (i32(3, 4), f32(3, 4), f32(3, 4), i32(3), i32(3), u8(3), i32(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4)] * 3 + [(3,)] * 4
    assert [o.dtype for o in k.outputs(None)] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8, torch.int32]
    mov, floor = k.movable(None), k.floor(None, 2)
    before = _native.tabascent_launches
    shared = i32(3)
    for out in (good[:6], (*good[:3], shared, shared, *good[5:]), (*good[:6], u8(3)), (good[0], f32(3, 5), *good[2:]), good[0],
                (good[0], f32(3, 8)[:, ::2], *good[2:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, sinr_db, capacity_mbps, rounds, moves, converged, domain\)'):
            k.solve(None, rb, pwr, None, mov, floor, 0.0, 16, out, 0)
    for bad in (-0.5, float('nan'), float('inf'), -1, True, '1', None):
        with pytest.raises(ValueError, match='min_gain_mbps must be a finite number >= 0'):
            k.solve(None, rb, pwr, None, mov, floor, bad, 16, None, 0)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match=r'max_rounds must be an int in \[1, 4096\]'):
            k.solve(None, rb, pwr, None, mov, floor, 0.0, bad, None, 0)
    for bad in (np.ones((4, 5), bool), np.ones((4, 4), np.int32)):
        with pytest.raises(ValueError, match=r'allowed must be bool \[4, 4\]'):
            k.solve(None, rb, pwr, bad, mov, floor, 0.0, 16, None, 0)
    with pytest.raises(ValueError, match='env_mask must be'):
        k.solve(None, rb, pwr, None, mov, floor, 0.0, 16, None, 0, env_mask=np.ones(4, bool))
    with pytest.raises(ValueError, match='table must be'):
        k.solve(torch.zeros((3, 3, 4)), rb, pwr, None, mov, floor, 0.0, 16, None, 0)
    with pytest.raises(ValueError, match='no live dB table'):
        native.solve(None, rb, pwr, None, mov, floor, 0.0, 16, None, 0)
    assert _native.tabascent_launches == before and k.gains is None and native.gains is None         # no work space before a launch
    # the shapes the object refuses when it is made, and the one only a mask pushes past the limit
    with pytest.raises(ValueError, match=r'rb_ascent_table\(\) serves at most 8192 RBs'):
        tra.TableRbAscent(_stub_sim(num_rbs=8193), 4, agent, torch, cpu)
    with pytest.raises(ValueError, match='the agent mask does not match the env'):
        tra.TableRbAscent(_stub_sim(), 4, agent[:3], torch, cpu)

    def wide(r):
        return SimpleNamespace(**{**vars(_stub_sim(num_rbs=r)), 'link_tx': np.ones(2048, dtype=np.int64), 'link_rx': np.zeros(2048, dtype=np.int64)})
    with pytest.raises(ValueError, match=rf'rb_ascent_table\(\).*2048 links on 384 RBs need {_header_lds(2048, 384)} bytes, more than 163840'):
        tra.TableRbAscent(wide(384), 2048, np.ones(2048, bool), torch, cpu)
    k = tra.TableRbAscent(wide(300), 2048, np.ones(2048, bool), torch, cpu)
    with pytest.raises(ValueError, match=rf'need {_header_lds(2048, 300, True)} bytes with an allowed mask, more than 163840'):
        k.need(True)
    assert k.need(False) == _header_lds(2048, 300)


def test_an_env_that_does_not_ask_never_opens_the_library_and_the_numpy_path_is_refused_by_name(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_tabascent_library', lambda: pytest.fail('libd2d_tabascent.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._table_rbascent is None
    for call in (lambda: env.rb_ascent_table(), lambda: env.rb_ascent_table(table=np.zeros((6, 5, 5))), lambda: env.rb_ascent_table_actions()):
        with pytest.raises(ValueError, match=r'rb_ascent_table\(\) needs the torch path'):
            call()
    with pytest.raises(ValueError, match=r'rb_ascent\(\) needs the torch path'):
        env.rb_ascent()
    assert env._table_rbascent is None
    doc = VecD2DEnv.rb_ascent_table.__doc__
    assert '4.3 GB' in doc and 'evaluate_table()' in doc and 'export_actions=True' in doc
    env.close()


def test_rb_ascent_table_actions_encode_the_solved_rbs_on_a_stubbed_handle(monkeypatch):
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
    env._t = {'pwr': torch.as_tensor(power, dtype=torch.int32)}
    seen = []
    env.rb_ascent_table = lambda *a: seen.append(a) or (torch.as_tensor(rb, dtype=torch.int32),) + (None,) * 6
    a = env.rb_ascent_table_actions('tab', 'mask', 'some', {'cue': 0.0, 'due': 5.0}, 0.05, 9)
    assert seen == [('tab', None, None, 'mask', 'some', {'cue': 0.0, 'due': 5.0}, 0.05, 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()


# ------------------------------------------------------------------------------------------ the conditions of the GPU cases
def test_the_case_table_covers_what_the_gpu_test_is_there_for():
    shapes = {(c[0] + c[1], c[2]) for c in tu.CASES.values()}
    assert shapes == {(3, 1), (37, 5), (20, 64), (20, 300), (96, 2), (300, 7), (50, 6), (1000, 320)}
    assert {(c[5], c[6]) for c in tu.CASES.values()} == {('float64', 0), ('float64', 1), ('float32', 0), ('float32', 1)}
    assert tu.lds_bytes(1000, 320) > 64 * 1024 and tu.CASES['n1000_r320'][4] > 1 and tu.CASES['n300_r7'][4] == 5
    assert [name for name, c in tu.CASES.items() if c[7]] == ['n50_r6_no_rb']


@pytest.mark.parametrize('name', list(tu.CASES))
def test_the_drawn_inputs_hold_what_the_gpu_cases_rest_on(name):
    c = tu.make_case(name)
    n, r, b = c.n, c.r, c.b
    t = c.table[:, :n]
    assert c.table.shape == (b, n + c.extra, n) and str(c.table.dtype) == c.dtype and np.array_equal(c.pl, t.astype(np.float64))
    assert np.isfinite(t).all() and (c.extra == 0 or np.isnan(c.table[:, n]).all())
    assert (tu.domain_of(c.table, n) == 0).all()                         # the NaN row of the live layout is no part of the block
    if c.extra:
        assert (tu.domain_of(c.table, n + 1) == 1).all()
    # not symmetric, no entry equals its neighbour in memory: a transposed or mis-pitched gain block shows
    off = ~np.eye(n, dtype=bool)
    assert (t != t.transpose(0, 2, 1))[:, off].all()
    flat = t.reshape(-1)
    assert (flat[1:] != flat[:-1]).all()
    on = (c.rb >= 0) & (c.rb < r)
    if name == 'n50_r6_no_rb':
        assert (c.rb[:, tu.NO_RB[0]] == -1).all() and (c.rb[:, tu.NO_RB[1]] == r).all() and (~on).sum() == 2 * b
    else:
        assert on.all()
    assert c.rb.dtype == c.pwr.dtype == np.int32 and c.pwr.min() >= 0 and (c.pwr[:, :c.cues] <= 23).all() and (c.pwr[:, c.cues:] <= 20).all()
    groups = [np.bincount(c.rb[e][on[e]], minlength=r) for e in range(b)]
    if name == 'n96_r2':
        assert min(g.min() for g in groups) >= 38                        # groups near 48
    if name in ('n20_r64', 'n20_r300'):
        assert all((g == 0).any() for g in groups)
    if name == 'n20_r300':
        assert r > 256 and r % 32 == 12
    if name == 'n300_r7':
        assert n > 256 and (n + 31) // 32 == 10


# ------------------------------------------------------------------------------------------ the restatement's properties
REFERENCE_CASES = [('n37_r5', False), ('n37_r5', True), ('n37_r5_f32', True), ('n50_r6_no_rb', False)]


@pytest.mark.parametrize('name,floors', REFERENCE_CASES)
def test_every_move_raises_the_envs_oracle_total_and_a_met_floor_is_kept(name, floors):
    c = tu.make_case(name)
    ref = tu.reference(name, floors)
    assert len(ref.raised) == len(ref.kept) == ref.moves.sum() > 0 and ref.converged.all()
    assert all(after > before for _, _, before, after in ref.raised)
    assert all(ok for _, _, ok in ref.kept)
    still = ~((c.rb >= 0) & (c.rb < c.r))
    assert np.array_equal(ref.rb[still], c.rb[still])                    # a link on no RB keeps the value it had
    if floors:
        # float64 on both sides and the same formulas: a link that meets its floor at the start meets it at the end, exactly
        fl = tu.floor_vector(tu.FLOORS, c.cues, c.dues).astype(np.float64)
        some = False
        for x in range(c.b):
            s0, s1 = (tu.oracle_planes(c, x, np.asarray(v[x])[None, :], c.pwr[x])[0][0] for v in (ref.start, ref.rb))
            met = s0 >= fl
            some |= bool(met.any())
            assert (s1[met] >= fl[met]).all()
        assert some


def test_the_restatement_on_a_table_of_a_law_is_rb_ascent_utils():
    """On the table a native law gives, the table restatement walks rb_ascent_util's restatement move for move: the two differ in
    where the path loss comes from and in nothing else."""
    import rb_ascent_util as ru
    from oracle import d2d_oracle as orc
    c0 = ru.make_case('n37_r5')
    envs = np.arange(3)
    pos = c0.pos[envs].astype(np.float64)
    tx, rx = np.asarray(c0.tx), np.asarray(c0.rx)
    d = pos[:, tx][:, :, None, :] - pos[:, rx][:, None, :, :]                                  # [e, tx link j, rx link i]
    dist = (d[..., 0] ** 2 + d[..., 1] ** 2) ** 0.5
    pl = orc.path_loss_db(c0.spec, dist, c0.cols.ant_h_m[tx][None, :, None], c0.cols.ant_h_m[rx][None, None, :])
    c = SimpleNamespace(name='law', cues=c0.cues, dues=c0.dues, n=c0.n, r=c0.r, b=3, pl=pl, rb=c0.rb[envs], pwr=c0.pwr[envs], tx=tx, rx=rx,
                        cols=c0.cols)
    got = tu.rb_ascent_ref(c, envs, floor=tu.FLOORS)
    want = ru.rb_ascent_ref(c0, envs, floor=ru.FLOORS)
    assert np.array_equal(got.rb, want.rb) and np.array_equal(got.moves, want.moves) and np.array_equal(got.rounds, want.rounds)
    assert got.moves.sum() > 0 and got.converged.all()


@pytest.mark.parametrize('name,floors', REFERENCE_CASES)
def test_the_reference_alone_stays_inside_the_cap_at_its_own_fixed_point(name, floors):
    """At the restatement's own fixed point the inequality holds with nothing to spare taken (worst <= 0 of the slack) and the share
    of (link, RB) checks left out for a SINR within W of a floor or a sensitivity is under the cap of 25 %."""
    c = tu.make_case(name)
    ref = tu.reference(name, floors)
    floor = tu.FLOORS if floors else None
    chk = tu.reference_check(c, np.arange(c.b), ref.rb, ref.converged, None, tu.movable_mask(c), floor, 0.0)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e}')
    assert chk.checks > 500 and chk.left_out <= tu.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 0.0


def test_floors_change_a_decision_the_gain_bar_stops_moves_and_two_rounds_leave_some_env_moving():
    free, fl = tu.reference('n37_r5'), tu.reference('n37_r5', True)
    assert not np.array_equal(free.rb, fl.rb)                            # the floors are felt
    two = tu.reference('n37_r5', False, 2)
    print(free.rounds.tolist(), two.rounds.tolist(), two.converged.astype(int).tolist())
    assert ((two.rounds == 2) & ~two.converged).any() and (free.rounds > 2).any()
    c = tu.make_case('n37_r5')
    gated = tu.rb_ascent_ref(c, np.arange(4), min_gain=0.5)
    assert (gated.moves <= free.moves[:4]).all() and (gated.moves < free.moves[:4]).any()


def test_the_domain_word_is_about_the_whole_block():
    c = tu.make_case('n37_r5')
    t = c.table.copy()
    t[1, 3, 30], t[4, 36, 0], t[2, 5, 6], t[7, c.n, 4] = np.nan, -np.inf, np.inf, -np.inf          # env 7: the row nobody reads
    assert tu.domain_of(t, c.n).tolist() == [0, 1, 0, 0, 1] + [0] * 11

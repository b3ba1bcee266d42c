"""Difference rewards on a path-loss table, the part that needs no GPU: the library's exported set and its place in the build, the
entry point's refusals (every one before a launch), the host class on a stub sim, the texts, the LDS formula, marginal_capacity()'s
unchanged refusals of the table routes, the float64 reference (table_marginal_util.marginal_ref) against a leave-one-out loop over
table_evaluate_util.reference, and the conditions the GPU cases of test_gpu_table_marginal.py rest on, re-derived on the drawn
inputs and the float64 reference alone."""
import json
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import table_evaluate_util as teu
import table_marginal_util as tmu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_tabmarg.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_tabmarg.hip'
ARGS = ['table', 'table_dtype', 'table_rows', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'n_envs', 'n_dev', 'n_links',
        'n_rbs', 'harm_mbps', 'difference_mbps', 'domain', 'hip_stream']
FORMULA = '16 n_links + round16(8 n_links) + 8 n4 + 3 round16(4 n_links) + round16(4 (n_rbs + 1)) + 16 bytes'


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_tabmarg_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_tabmarg_library()
    assert _native.side_library('tabmarg') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_tabmarg.so') == declared == {'d2d_table_marginal', 'd2d_tabmarg_last_error'}
    assert set(_native.TABMARG_SIGNATURES) == declared and _native.LATER['tabmarg'] is _native.TABMARG_SIGNATURES
    ctype = {'const void*': _native._P, 'const float*': _native._P, 'const int32_t*': _native._P, 'float*': _native._P,
             'int32_t*': _native._P, 'void*': _native._P, 'int32_t': _native._I, 'int64_t': _native.C.c_int64}
    args = re.search(r'^int d2d_table_marginal\((.*?)\);', header, flags=re.M | re.S).group(1).replace('\n', ' ').split(',')
    assert [a.strip().split()[-1].lstrip('*') for a in args] == ARGS
    assert [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args] == _native.TABMARG_SIGNATURES['d2d_table_marginal'][1]
    for symbol, (res, argtypes) in _native.TABMARG_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_tabmarg_last_error(), bytes)
    for const in ('F32', 'F64', 'MAX_LINKS', 'MAX_RBS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_TABMARG_%s (\d+)' % const, header).group(1)) == getattr(_native, 'TABMARG_' + const), const
    # marginal_capacity()'s limits, evaluate_table()'s entry types
    assert (_native.TABMARG_MAX_LINKS, _native.TABMARG_MAX_RBS, _native.TABMARG_MAX_LDS_BYTES) == (2048, _native.MARGINAL_MAX_RBS, 160 * 1024)
    assert (_native.TABMARG_F32, _native.TABMARG_F64) == (_native.EVALTAB_F32, _native.EVALTAB_F64)
    # the LATER rows are in both tables, in one order: between deviate and evaltab; rbascent first, goodput last, evaltab and
    # tabascent the two rows before it
    order = list(build.LATER)
    assert build.LATER['tabmarg'] == ['d2d_tabmarg.hip'] and order == list(_native.LATER)
    assert order.index('deviate') + 1 == order.index('tabmarg') == order.index('evaltab') - 1
    assert order[0] == 'rbascent' and order[-3:] == ['evaltab', 'tabascent', 'goodput']
    assert build.COMPLETE == {**build.EVERY, **build.LATER} and 'tabmarg' not in build.EVERY
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('tabmarg') == LIB_DIR / 'libd2d_tabmarg.so' == _native.side_path('tabmarg')
    assert 'tabmarg' in build.__doc__ and '4.28' in build.__doc__
    # the file is compiled as d2d_evaltab.hip is: the same flags give the same conversion
    assert build.flags_for('d2d_tabmarg.hip') == build.flags_for('d2d_evaltab.hip') == build.FLAGS
    assert _native.tabmarg_launches >= 0 and callable(_native.table_marginal)


def test_a_missing_tabmarg_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and 'tabmarg' in build.later_missing(tmp_path)
    build.lib_path('tabmarg', tmp_path).touch()
    assert 'tabmarg' not in build.later_missing(tmp_path)
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_tabmarg\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_tabmarg_library()


def test_the_source_restates_the_steps_conversion_and_calls_no_atomic():
    src = SOURCE.read_text()
    for name in ('d2d_addon.h', 'd2d_tabmarg.h', 'd2d_same_rb.h', 'd2d_step_device.h'):
        assert f'#include "{name}"' in src
    line = '(float)exp2(-0.33219280948873623478703194294894 * x)'
    assert src.count(line) == 1 and line in (SOURCE.parent / 'd2d_evaltab.hip').read_text()
    assert not re.search(r'\batomic\w*\s*\(|__hip_atomic|__atomic', src)
    # phase 1 walks the receiver's column, phase 2 the transmitter's row; one launch per call, no gain block
    assert '(size_t)__float_as_int(o.y) * (size_t)N + (size_t)i' in src and '(size_t)i * (size_t)N + (size_t)j' in src
    assert src.count('launch(&tabmarg_kernel<') == 2 and not re.search(r'\bgains\b', src)


# ------------------------------------------------------------------------------------------ the LDS formula and the entry point
def _header_lds(n, r):
    """The formula as include/d2d_tabmarg.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    n4 = (n + 3) // 4 * 4
    return 16 * n + r16(8 * n) + 8 * n4 + 3 * r16(4 * n) + r16(4 * (r + 1)) + 16


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, table_marginal
    header = ' '.join(HEADER.read_text().replace(' *', ' ').split())
    assert FORMULA in header
    for n, r in [(1, 1), (2047, 8), (2048, 256), (2048, 8192)] + [(c[0], c[1]) for c in tmu.CASES]:
        assert table_marginal.lds_bytes(n, r) == tmu.lds_bytes(n, r) == _header_lds(n, r), (n, r)
    # the largest shape the two limits admit fits: the refusal past 160 KiB stands for a limit that moves
    assert _header_lds(2048, 8192) == 122912 <= _native.TABMARG_MAX_LDS_BYTES and '122912' in header


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(dtype=0, rows=None, n_envs=2, n_dev=5, n_links=2, n_rbs=3)

    def call(ptr=8, out=(8, 16, 24), **kw):
        a = dict(ok, **kw)
        _native.table_marginal(ptr, a['dtype'], a['n_links'] if a['rows'] is None else a['rows'], ptr, ptr, ptr, ptr, ptr, ptr,
                               a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'], *out)
    before = _native.tabmarg_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=2049), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=8193), r'n_rbs must be in \[1, 8192\]'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'),
                     (dict(dtype=2), 'table_dtype must be'), (dict(dtype=-1), 'table_dtype must be'),
                     (dict(rows=1), r'table_rows must be n_links or n_links \+ 1'), (dict(rows=4), 'table_rows must be'),
                     (dict(ptr=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 8 * (i + 1) for i in range(3))), 'null device pointer') for z in range(3)),
                     (dict(out=(8, 8, 24)), 'harm_mbps and difference_mbps must be two planes')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(n_links=2048, n_rbs=8192), dict(rows=3), dict(dtype=1)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.tabmarg_launches == before


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


def test_the_refusal_texts_name_the_api_and_marginal_capacity_keeps_refusing_the_table_routes_word_for_word():
    from gym_d2d_amd import marginal, sensing, table_evaluate, table_marginal as tm
    for route in (None, 'device_table', 'link_table', 'array', 'per_step', 'channel'):
        assert tm.refusal(_stub_sim(route), True, True) is None and tm.refusal(_stub_sim(route), False, True) is None
    assert tm.refusal(_stub_sim(shadowing=True), True, True) is None
    assert tm.refusal(_stub_sim(), True, False) == 'marginal_capacity_table() needs the torch path (use_torch): its planes are device tensors'
    assert len(tm.ROW) == len(table_evaluate.ROW) and 'marginal_capacity_table' not in ' '.join(sensing.REFUSALS)
    for route in ('native', 'device_table', 'link_table', 'array', 'per_step', 'channel'):
        text = tm.no_live_table(_stub_sim(route))
        assert text == table_evaluate.no_live_table(_stub_sim(route)).replace('evaluate_table()', 'marginal_capacity_table()')
        assert text.startswith('marginal_capacity_table() has no live dB table to read on the ') and f"'{route}'" in text
        assert 'pass table=' in text and 'evaluate_table' not in text
    text = tm.no_start_state()
    assert text.startswith('marginal_capacity_table() ') and 'rb=' in text and 'power_dbm=' in text and 'export_actions=True' in text
    assert tm.TableMarginalResult._fields == ('difference_mbps', 'harm_mbps', 'domain')
    # what an env tells a reward / obs function that asks for the planes on every step, by name
    who = 'TableDifferenceRewardFunction'
    for route in ('channel', 'per_step', 'array'):
        assert tm.reward_refusal(_stub_sim(route), True, True, who) is None
    assert tm.reward_refusal(_stub_sim('channel'), True, False, who).startswith(who + ' needs the torch path')
    for route in (None, 'device_table', 'link_table'):
        text = tm.reward_refusal(_stub_sim(route), True, True, who)
        assert text.startswith(who + ' needs a live dB table') and f"'{_stub_sim(route).path_loss_table.route}'" in text
    text = tm.reward_refusal(_stub_sim('channel'), False, True, who)
    assert text.startswith(who + ': marginal_capacity_table() ') and 'export_actions=True' in text
    # marginal_capacity() itself: the table routes stay refused, in the golden words
    golden = json.loads((ROOT / 'tests' / 'golden' / 'pair_kernel_messages.json').read_text())
    for route in ('link_table', 'per_step', 'channel'):
        assert marginal.refusal(_stub_sim(route), True) == golden[f'marginal.refusal/{route}'] == (
            f"marginal_capacity() does not serve the '{route}' path-loss route (a table, not a law its kernel can evaluate from the "
            "transmitter's side); it serves the native power-law models")
    assert marginal.refusal(_stub_sim(), True) is None


def test_the_kernel_object_refuses_bad_arguments_before_a_launch_and_never_opens_the_library(monkeypatch):
    import torch
    from gym_d2d_amd import _native, sensing, table_evaluate, table_marginal as tm
    monkeypatch.setattr(_native, 'load_tabmarg_library', lambda: pytest.fail('libd2d_tabmarg.so was opened'))
    cpu = torch.device('cpu')
    live = torch.zeros((3, 5, 4), dtype=torch.float64)
    k = tm.TableMarginal(_stub_sim('channel', live), 4, torch, cpu)
    assert isinstance(k, table_evaluate.TableEvaluate) and isinstance(k, sensing.PairKernel) and (k.b, k.d, k.n, k.r) == (3, 7, 4, 4)
    assert len(k.ptrs) == 4 and tuple(k.cols.shape) == (3, 7) and tuple(k.cap_cols.shape) == (2, 7) and k.own is None
    assert k.table(None)[0] is live and k.table(None)[1:] == (_native.TABMARG_F64, 5)
    assert k.table(torch.zeros((3, 4, 4)))[1:] == (_native.TABMARG_F32, 4)
    for bad in (torch.zeros((3, 4, 3)), torch.zeros((3, 6, 4)), torch.zeros((2, 4, 4)), torch.zeros((3, 4, 4), dtype=torch.float16),
                torch.zeros((3, 4, 8))[:, :, ::2], np.zeros((3, 4, 4)), torch.zeros((4, 4))):
        with pytest.raises(ValueError, match='table must be'):
            k.table(bad)
    native = tm.TableMarginal(_stub_sim(), 4, torch, cpu)
    with pytest.raises(ValueError, match=r"marginal_capacity_table\(\) has no live dB table to read on the 'native' path-loss route.*pass table="):
        native.table(None)
    i32, f32 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s))
    rb, pwr = i32(3, 4), i32(3, 4)
    assert k.start(rb, 'rb') is rb
    for bad, name in ((i32(3, 5), 'rb'), (f32(3, 4), 'power_dbm'), (i32(3, 8)[:, ::2], 'rb'), (np.zeros((3, 4), np.int32), 'power_dbm'), (i32(4), 'rb')):
        with pytest.raises(ValueError, match=rf'{name} must be a contiguous int32 tensor \[3, 4\]'):
            k.start(bad, name)
    good = (f32(3, 4), f32(3, 4), i32(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4), (3, 4), (3,)]
    assert [o.dtype for o in k.outputs(None)] == [torch.float32, torch.float32, torch.int32]
    before = _native.tabmarg_launches
    shared = f32(3, 4)
    for out in (good[:2], (shared, shared, good[2]), (good[0], good[1], f32(3)), (good[0], f32(3, 5), good[2]), good[0],
                (good[0], f32(3, 8)[:, ::2], good[2]), (good[0], good[1], i32(4))):
        with pytest.raises(ValueError, match=r'out must be \(difference_mbps, harm_mbps, domain\)'):
            k.marginal(None, rb, pwr, out, 0)
    with pytest.raises(ValueError, match='table must be'):
        k.marginal(torch.zeros((3, 3, 4)), rb, pwr, None, 0)
    with pytest.raises(ValueError, match='no live dB table'):
        native.marginal(None, rb, pwr, None, 0)
    assert _native.tabmarg_launches == before
    with pytest.raises(ValueError, match=r'marginal_capacity_table\(\) serves at most 8192 RBs'):
        tm.TableMarginal(_stub_sim(num_rbs=8193), 4, torch, cpu)


def test_an_env_that_does_not_ask_never_opens_the_library_and_the_numpy_path_is_refused_by_name(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import TableDifferenceRewardFunction, VecD2DEnv
    from gym_d2d_amd.envs.reward_fn import DifferenceRewardFunction, RewardFunction
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_tabmarg_library', lambda: pytest.fail('libd2d_tabmarg.so was opened'))
    cfg = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}
    env = VecD2DEnv(cfg, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._table_marginal is None and not env._wants_table_marginal
    for call in (lambda: env.marginal_capacity_table(), lambda: env.marginal_capacity_table(table=np.zeros((6, 5, 5)))):
        with pytest.raises(ValueError, match=r'marginal_capacity_table\(\) needs the torch path'):
            call()
    assert env._table_marginal is None
    doc = VecD2DEnv.marginal_capacity_table.__doc__
    assert 'evaluate_table()' in doc and 'export_actions=True' in doc and 'csrc/d2d_tabmarg.hip' in doc
    env.close()
    # the reward function: its fields, and the construction refusal of the NumPy path, by name
    fn = TableDifferenceRewardFunction()
    assert isinstance(fn, RewardFunction) and fn.native_id == _native.REWARD_NONE and fn.needs_table_marginal is True
    assert not getattr(fn, 'needs_marginal', False) and not getattr(DifferenceRewardFunction, 'needs_table_marginal', False)
    view = SimpleNamespace(difference_mbps=object())
    assert fn.compute(view) is view.difference_mbps
    with pytest.raises(RuntimeError, match='VecD2DEnv'):
        fn({}, {})
    with pytest.raises(ValueError, match=r'TableDifferenceRewardFunction needs the torch path'):
        VecD2DEnv(dict(cfg, reward_fn=TableDifferenceRewardFunction), num_envs=6, use_torch=False)


# ------------------------------------------------------------------------------------------ the reference and the GPU cases' conditions
@pytest.mark.parametrize('case', [(3, 1, 5, 'float32', 1), (50, 6, 5, 'float64', 1)])
def test_the_reference_is_a_leave_one_out_over_the_evaluate_reference(case):
    """Candidate 0 is the state, candidate i + 1 has link i at rb -1 (on no RB: it harms nobody): harm[i] is what the OTHER links'
    capacities gain from candidate 0 to candidate i + 1."""
    c, ref = tmu.make_case(*case), tmu.case_ref(*case)
    n = c['n']
    rb = np.repeat(c['rb'][:, None, :], n + 1, axis=1)
    rb[:, np.arange(n) + 1, np.arange(n)] = -1
    _, cap, _, _ = teu.reference(c, rb=rb, pwr=np.repeat(c['pwr'][:, None, :], n + 1, axis=1))
    others = ~np.eye(n, dtype=bool)
    harm = ((cap[:, 1:] - cap[:, :1]) * others[None]).sum(axis=2)
    assert np.abs(cap[:, 0] - ref['capacity']).max() <= 1e-9
    assert np.abs(harm - ref['harm']).max() <= 1e-9 and np.abs(cap[:, 0] - harm - ref['difference']).max() <= 1e-9
    assert (ref['harm'] > 0).any() and (ref['harm'] >= 0).all()


def test_the_case_table_and_the_share_of_undecided_links():
    assert tmu.CASES == ((1, 1, 1, 'float64', 0), (3, 1, 5, 'float32', 1), (50, 6, 5, 'float64', 1), (130, 70, 5, 'float32', 1),
                         (300, 2, 1, 'float64', 0), (300, 2, 5, 'float32', 1))
    assert tmu.THRESHOLD_CAP == 0.01 and tmu.THRESHOLD_DB == 1e-4 and tmu.BAR == 1e-5
    assert 130 % 64 == 2 and 300 > tmu.THREADS
    left = []
    for case in tmu.CASES:
        c, ref = tmu.make_case(*case), tmu.case_ref(*case)
        n, r, b, dtype, extra = case
        assert c['table'].shape == (b, n + extra, n) and str(c['table'].dtype) == dtype and c['rb'].shape == c['pwr'].shape == (b, n)
        assert extra == 0 or np.isnan(c['table'][:, n]).all()
        left.append(int((~ref['decided']).sum()))
        assert left[-1] <= tmu.THRESHOLD_CAP * b * n
        if n >= 50:
            assert (c['rb'] == -1).any() and (c['rb'] == r).any()        # links on no RB, on either side
            assert (ref['harm'] > 0).mean() > 0.5
        off = (c['rb'] < 0) | (c['rb'] >= r)
        alone = off | (tmu.same_rb(c['rb'], r).sum(axis=1) == 0)
        assert (ref['harm'][alone] == 0.0).all() and np.array_equal(ref['difference'][alone], ref['capacity'][alone])
    print('undecided links per case:', left)
    assert tuple(left) == tmu.LEFT_OUT == (0,) * 6
    groups = np.bincount(tmu.make_case(*tmu.CASES[4])['rb'][0].clip(0, 2), minlength=3)[:2]
    assert groups.min() >= 120                                           # groups of about 150


def test_the_planted_pair_lifts_its_victim_over_the_threshold():
    c, p, q = tmu.planted_lifted()
    e, r = tmu.PLANT_ENV, tmu.PLANT_RB
    assert np.flatnonzero(c['rb'][e] == r).tolist() == sorted([p, q]) and teu.DEAD_LINK not in (p, q)
    ref = tmu.marginal_ref(c)
    sens = c['ocols'].sens_dbm[np.asarray(c['rx'])]
    assert abs(ref['sinr_db'][e, q] - (sens[q] - 3.0)) < 1e-9 and ref['capacity'][e, q] == 0.0
    assert ref['lifted'][e, p] == 1 and ref['harm'][e, p] > 1.0 and ref['decided'][e, p] and ref['decided'][e, q]
    # harm[p] is q's whole capacity alone, its SNR's
    rb = c['rb'].copy()
    rb[e, p] = -1
    assert abs(tmu.marginal_ref(c, rb=rb)['capacity'][e, q] - ref['harm'][e, p]) <= 1e-12

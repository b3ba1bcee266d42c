"""What-if evaluation on a path-loss table, the part that needs no GPU: the library's exported set and its place in the build, the
entry point's refusals (every one before the launch), the texts of the host module, the LDS formula, and the conditions the GPU
cases of test_gpu_table_evaluate.py rest on, re-derived on the drawn inputs and on the float64 reference alone."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import table_evaluate_util as teu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_evaltab.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_evaltab.hip'
ARGS = ['table', 'table_dtype', 'table_rows', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'n_envs', 'n_cand', 'n_dev',
        'n_links', 'n_rbs', 'sinr_db', 'capacity_mbps', 'total_mbps', 'domain', 'hip_stream']


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_evaltab_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_evaltab_library()
    assert _native.side_library('evaltab') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_evaltab.so') == declared == {'d2d_evaluate_table', 'd2d_evaltab_last_error'}
    assert set(_native.EVALTAB_SIGNATURES) == declared and _native.LATER['evaltab'] is _native.EVALTAB_SIGNATURES
    ctype = {'const void*': _native._P, 'const float*': _native._P, 'const int32_t*': _native._P, 'float*': _native._P,
             'int32_t*': _native._P, 'void*': _native._P, 'int32_t': _native._I, 'int64_t': _native.C.c_int64}
    args = re.search(r'^int d2d_evaluate_table\((.*?)\);', header, flags=re.M | re.S).group(1).replace('\n', ' ').split(',')
    assert [a.strip().split()[-1].lstrip('*') for a in args] == ARGS
    assert [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args] == _native.EVALTAB_SIGNATURES['d2d_evaluate_table'][1]
    for symbol, (res, argtypes) in _native.EVALTAB_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_evaltab_last_error(), bytes)
    for const in ('F32', 'F64', 'MAX_LINKS', 'MAX_RBS', 'CHUNK', 'MAX_CANDIDATES', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_EVALTAB_%s (\d+)' % const, header).group(1)) == getattr(_native, 'EVALTAB_' + const), const
    # evaluate()'s limits, and the entry types of the live table's own constants
    assert (_native.EVALTAB_MAX_RBS, _native.EVALTAB_CHUNK, _native.EVALTAB_MAX_CANDIDATES, _native.EVALTAB_MAX_LDS_BYTES) == \
        (_native.EVALUATE_MAX_RBS, _native.EVALUATE_CHUNK, _native.EVALUATE_MAX_CANDIDATES, _native.EVALUATE_MAX_LDS_BYTES)
    assert (_native.EVALTAB_F32, _native.EVALTAB_F64) == (_native.F32, _native.F64) and teu.CHUNK == _native.EVALTAB_CHUNK
    # the LATER rows are in both tables, in one order: behind rbascent, in front of goodput, which stays the last row
    order = list(build.LATER)
    assert build.LATER['evaltab'] == ['d2d_evaltab.hip'] and order == list(_native.LATER)
    assert order[0] == 'rbascent' and order[-1] == 'goodput' and 0 < order.index('evaltab') < len(order) - 1
    assert build.COMPLETE == {**build.EVERY, **build.LATER} and list(build.COMPLETE)[:len(build.EVERY)] == list(build.EVERY)
    assert 'evaltab' not in build.EVERY
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('evaltab') == LIB_DIR / 'libd2d_evaltab.so' == _native.side_path('evaltab')
    assert 'evaltab' in build.__doc__ and '4.26' in build.__doc__
    assert _native.evaltab_launches >= 0 and callable(_native.evaluate_table)


def test_a_missing_evaltab_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and 'evaltab' in build.later_missing(tmp_path)
    build.lib_path('evaltab', tmp_path).touch()
    assert 'evaltab' not in build.later_missing(tmp_path)
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_evaltab\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_evaltab_library()


def test_the_source_includes_the_shared_headers_and_holds_no_atomic():
    src = SOURCE.read_text()
    for name in ('d2d_addon.h', 'd2d_evaltab.h', 'd2d_same_rb.h', 'd2d_step_device.h'):
        assert f'#include "{name}"' in src
    assert 'atomic' not in src and 'table_gain_db' in src                    # the conversion is restated with a pointer at the step's
    assert '(float)exp2(-0.33219280948873623478703194294894 * x)' in src
    assert '(float)exp2(-0.33219280948873623478703194294894 * x)' in (SOURCE.parent / 'd2d_step_device.h').read_text()


# ------------------------------------------------------------------------------------------ the entry point's refusals
def _call(ptr=8, dtype=0, rows=None, total=8, domain=8, sinr=16, cap=24, **kw):
    from gym_d2d_amd import _native
    a = dict(dict(n_envs=2, n_cand=3, n_dev=9, n_links=4, n_rbs=3), **kw)
    _native.evaluate_table(ptr, dtype, a['n_links'] if rows is None else rows, ptr, ptr, ptr, ptr, ptr, ptr, a['n_envs'], a['n_cand'],
                           a['n_dev'], a['n_links'], a['n_rbs'], sinr, cap, total, domain)


def test_the_entry_point_refuses_bad_arguments_by_name_before_any_launch():
    from gym_d2d_amd import _native
    before = _native.evaltab_launches
    for kw, text in ((dict(n_envs=-1), r'n_envs must be in \[0, 2\^31\)'), (dict(n_envs=2 ** 31), 'n_envs must be'),
                     (dict(n_cand=0), r'n_cand must be in \[1, 524280\]'), (dict(n_cand=524281), 'n_cand must be'),
                     (dict(n_links=0), r'n_links must be in \[1, 2048\]'), (dict(n_links=2049), 'n_links must be'),
                     (dict(n_rbs=0), r'n_rbs must be in \[1, 8192\]'), (dict(n_rbs=8193), 'n_rbs must be'),
                     (dict(n_dev=0), 'n_dev must be >= 1'), (dict(dtype=2), 'table_dtype must be'), (dict(dtype=-1), 'table_dtype must be'),
                     (dict(rows=3), r'table_rows must be n_links or n_links \+ 1'), (dict(rows=6), 'table_rows must be'),
                     (dict(ptr=0), 'null device pointer'), (dict(total=0), 'null device pointer'), (dict(domain=0), 'null device pointer'),
                     (dict(sinr=16, cap=16), 'must be two planes')):
        with pytest.raises(_native.NativeError, match=text):
            _call(**kw)
    _call(n_envs=0)                                    # nothing to do: no launch, no error
    _call(n_envs=0, rows=5, sinr=0, cap=0)
    assert _native.evaltab_launches == before


def test_lds_bytes_are_the_layout_of_the_kernel_and_stay_below_the_limit_at_the_caps():
    from gym_d2d_amd import _native, table_evaluate
    r16 = lambda x: (x + 15) // 16 * 16
    for n, r in [(c[0], c[1]) for c in teu.CASES] + [(2, 1), (5, 7), (2047, 8191), (2048, 8192)]:
        want = 16 * n + r16(4 * n) + r16(8 * n) + 4 * ((n + 3) // 4 * 4) + r16(4 * n) + r16(4 * (r + 1)) + 48
        assert table_evaluate.lds_bytes(n, r) == teu.lds_bytes(n, r) == want, (n, r)
    assert table_evaluate.lds_bytes(2048, 8192) == 106560 < _native.EVALTAB_MAX_LDS_BYTES            # 36 bytes per link
    src = ' '.join(SOURCE.read_text().split())
    assert 'ca float4[N] (tx constant, bw_mhz, rx_lin, noise) | sens float[N]' in src
    assert 'bytes of LDS, more than the' in src


# ------------------------------------------------------------------------------------------ the host module's texts
def _sim(route, live=None, n=4, b=2):
    table = SimpleNamespace(route=route, live=live, law=None)
    return SimpleNamespace(path_loss_table=table, link_tx=np.zeros(n, np.int32), num_envs=b)


def test_the_refusals_and_the_out_text_name_evaluate_table():
    from gym_d2d_amd import sensing, table_evaluate as te
    assert 'evaluate_table' not in ' '.join(sensing.REFUSALS) and len(te.ROW) == len(te.ROW_ACTIONS) == len(sensing.REFUSALS['evaluate'])
    assert te.refusal(_sim('native'), True, True) is None and te.refusal(_sim('channel'), False, True) is None
    why = te.refusal(_sim('native'), True, False)
    assert why == 'evaluate_table() needs the torch path (use_torch): its planes are device tensors'
    why = te.fixed_links_refusal(_sim('channel'), False)
    assert why.startswith('evaluate_table_actions() ') and why.endswith(': build the env with export_actions=True')
    assert te.fixed_links_refusal(_sim('channel'), True) is None
    for route in ('native', 'device_table', 'link_table', 'array', 'per_step', 'channel'):
        assert te.live_table(_sim(route)) is None
        text = te.no_live_table(_sim(route))
        assert text.startswith('evaluate_table() ') and f"'{route}'" in text and 'pass table=' in text
    live = SimpleNamespace(shape=(2, 5, 4))
    for route in ('array', 'per_step', 'channel'):
        assert te.live_table(_sim(route, live)) is live
        assert te.live_table(_sim(route, live, n=3)) is None                 # a table of another link list is not this env's
    for route in ('native', 'device_table', 'link_table'):
        assert te.live_table(_sim(route, live)) is None
    text = te.out_message('cuda:0', {'total_mbps': (2, 3), 'domain': (2, 3), 'sinr_db': (2, 3, 4)})
    assert text.startswith('evaluate_table(): out must be a dict of contiguous float32 tensors (domain: int32) on cuda:0 that do not share')
    assert text.endswith('total_mbps [2, 3], domain [2, 3], sinr_db [2, 3, 4]')


def test_the_folded_columns_are_the_steps_columns_of_its_table_modes():
    from gym_d2d_amd.table_evaluate import fold_table_columns
    ocols = teu.columns(50)[0]
    budget = {'eirp_off_db': ocols.eirp_off_db, 'rx_off_db': ocols.rx_off_db, 'noise_dbm': ocols.noise_dbm}
    cols = fold_table_columns(budget)
    assert cols.dtype == np.float32 and cols.shape == (3, len(ocols.noise_dbm))
    for row, name in enumerate(('eirp_off_db', 'rx_off_db', 'noise_dbm')):
        assert np.array_equal(cols[row], (10.0 ** (np.asarray(budget[name], dtype=np.float64) / 10.0)).astype(np.float32))
    with pytest.raises(ValueError, match='outside the float32 linear range'):
        fold_table_columns(dict(budget, noise_dbm=np.full_like(ocols.noise_dbm, -400.0)))


# ------------------------------------------------------------------------------------------ the conditions of the GPU cases
def test_the_case_table_covers_what_the_gpu_test_is_there_for():
    shapes = {(c[0], c[1]) for c in teu.CASES}
    assert shapes == {(1, 1), (3, 1), (50, 6), (130, 70), (300, 2)}
    assert {c[2] for c in teu.CASES} == {1, teu.CHUNK, teu.CHUNK + 1, 2 * teu.CHUNK + 1}
    assert {c[3] for c in teu.CASES} == {1, 5}
    assert {(c[4], c[5]) for c in teu.CASES} == {('float64', 0), ('float64', 1), ('float32', 0), ('float32', 1)}
    assert max(c[0] for c in teu.CASES) > teu.THREADS


@pytest.mark.parametrize('case', teu.CASES)
def test_the_drawn_inputs_hold_what_the_gpu_cases_rest_on(case):
    n, r, k, b, dtype, extra = case
    c = teu.make_case(*case)
    # entries: every float64 draw is its own value; the table the kernel reads is not symmetric and no entry equals its neighbour in
    # memory (all a float32 table of this size can hold), and the reference reads exactly the kernel's entries
    assert len(np.unique(c['draw'])) == c['draw'].size and np.isfinite(c['draw']).all()
    t = c['table'][:, :n]
    assert c['table'].shape == (b, n + extra, n) and str(c['table'].dtype) == dtype and np.array_equal(c['pl'], t.astype(np.float64))
    assert extra == 0 or np.isnan(c['table'][:, n]).all()
    off = ~np.eye(n, dtype=bool)
    assert (t != t.transpose(0, 2, 1))[:, off].all()
    flat = t.reshape(-1)
    assert (flat[1:] != flat[:-1]).all()
    if dtype == 'float64':
        assert len(np.unique(t)) == t.size
    # planes: an RB with at least 3 members (from 3 links on), a link on no RB, both kinds of it where there are two links to spare
    rb = c['rb']
    on = (rb >= 0) & (rb < r)
    assert (~on).any() and set(np.unique(rb[~on])) <= {-1, r}
    if n >= 5:
        assert set(np.unique(rb[~on])) == {-1, r}
    if n >= 3:
        members = max(int(np.bincount(rb[e, q][on[e, q]], minlength=r).max()) for e in range(b) for q in range(k))
        assert members >= 3
    if (n, r) == (300, 2):
        assert members >= 140
    assert c['pwr'].min() == teu.P_LOW and c['pwr'].max() == teu.P_HIGH
    # the reference alone: finite, at most 1 % of the capacities within the near-threshold margin, live and dead links both there
    sinr, cap, total, decided = teu.case_ref(*case)
    assert np.isfinite(sinr).all() and np.isfinite(cap).all() and (cap > 0).any()
    assert float((~decided).mean()) <= teu.THRESHOLD_CAP
    if n > teu.DEAD_LINK:
        assert (cap[:, :, teu.DEAD_LINK] == 0).all() and (sinr[:, :, teu.DEAD_LINK] < c['ocols'].sens_dbm[c['rx'][teu.DEAD_LINK]]).all()


def test_the_total_restated_on_the_host_is_a_sum_of_the_capacities():
    rng = np.random.default_rng(3)
    for n, r in ((1, 1), (50, 6), (300, 2)):
        cap = rng.uniform(0, 50, n).astype(np.float32)
        rb = rng.integers(-1, r + 1, n)
        got = teu.total_in_order(cap, rb, r)
        assert got.dtype == np.float32 and abs(float(got) / cap.astype(np.float64).sum() - 1.0) <= 1e-7
    assert teu.totals_in_order(np.ones((2, 3, 5), np.float32), np.zeros((2, 3, 5), int), 1).tolist() == [[5.0] * 3] * 2

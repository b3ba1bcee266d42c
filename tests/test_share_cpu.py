"""Exact optimal RB sharing, the part that needs no GPU: the solver's restatement against brute force over all R^M placements, the
float64 value block against evaluate_util.evaluate_ref along whole placements, the library's exported set and its place in the build,
the refusals, the host class on a stub sim, and the conditions the GPU cases are there for (share_util)."""
import itertools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import evaluate_util as evu
import share_util as shu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_share.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_share.hip'


# ------------------------------------------------------------------------------------------ the restatement against brute force
def _blocks():
    """(block [R, 2^M], quota) for (M, R) = (1, 1), (4, 3), (5, 4), (6, 3): continuous values (a unique maximum almost surely) three
    times out of four, small integers (ties abound) else; holes of -inf, NaN and +inf; quotas of 0 / 1 / 2 / 3 / none."""
    rng = np.random.default_rng(21)
    quotas = (None, 2, 1, 'mixed', None, 'zero')
    for m, r, count in ((1, 1, 12), (4, 3, 40), (5, 4, 24), (6, 3, 24)):
        for i in range(count):
            kind = 'integers' if i % 4 == 3 else 'continuous'
            v = shu.random_block(rng, 1, r, m, kind, holes=0.06 if i % 2 else 0.0)[0]
            quota = quotas[i % len(quotas)]
            if quota == 'mixed':
                quota = rng.integers(1, 4, r)
                quota[i % r] = 0
            elif quota == 'zero':
                quota = np.where(np.arange(r) == i % r, m, 0)            # every RB closed but one
            yield v, quota


def test_the_restatement_equals_brute_force_over_every_placement():
    cases = ties = infeasible = 0
    for v, quota in _blocks():
        best, where = shu.brute_force(v, quota)
        col, value, feasible = shu.solve_ref(v[None], quota)
        cases += 1
        if best is None:
            infeasible += 1
            assert feasible.tolist() == [0] and (col == -1).all() and value[0] == 0.0 and not np.signbit(value[0])
            continue
        # equal as floats: max is exact, and a placement's value is one chain of additions in RB order in both
        assert feasible.tolist() == [1] and value[0] == best, (v, quota, value, best)
        assert tuple(col[0].tolist()) in where
        if len(where) > 1:
            ties += 1
        else:
            assert tuple(col[0].tolist()) == where[0]
    print(f'{cases} blocks: {ties} with a tied maximum, {infeasible} infeasible')
    assert cases == 100 and 0 < ties <= cases // 4 and 0 < infeasible < cases // 4


def test_ties_go_to_the_lowest_subset_and_what_is_not_finite_is_never_chosen():
    # all equal: on the last RB the lowest S with g finite is S = 0 until RB 0, which must take everybody
    col, value, feasible = shu.solve_ref(np.full((1, 3, 8), 1.5))
    assert col.tolist() == [[0, 0, 0]] and value.tolist() == [4.5] and feasible.tolist() == [1]
    # two placements of equal value: link 0 on RB 1 (S = 1 there) or on RB 0: at the last RB S = 0 is the lower subset
    v = np.zeros((1, 2, 2))
    assert shu.solve_ref(v)[0].tolist() == [[0]]
    v[0, 0, 1] = -np.inf                                                 # RB 0 refuses the link
    assert shu.solve_ref(v)[0].tolist() == [[1]]
    for hole in (np.nan, np.inf, -np.inf):
        v = np.array([[[1.0, 2.0], [1.0, hole]]])
        col, value, feasible = shu.solve_ref(v)
        assert col.tolist() == [[0]] and value.tolist() == [3.0]
        v = np.array([[[1.0, hole], [hole, 2.0]]])                       # the only placement left
        assert shu.solve_ref(v)[0].tolist() == [[1]] and shu.solve_ref(v)[1].tolist() == [3.0]
        v = np.array([[[1.0, 2.0], [hole, hole]]])                       # RB 1 has no admissible subset, not even S = 0: no placement
        assert [x.tolist() for x in shu.solve_ref(v)] == [[[-1]], [0.0], [0]]
    # quota 1 is the one-to-one matching
    import assign_util as asu
    rng = np.random.default_rng(3)
    for _ in range(20):
        w = rng.normal(5.0, 2.0, (4, 5))
        block = np.full((1, 5, 16), -np.inf)
        block[0, :, 0] = 0.0
        for a in range(4):
            block[0, :, 1 << a] = w[a]
        col, value, _ = shu.solve_ref(block, 1)
        assert abs(value[0] - asu.brute_force(w)) <= 1e-12 * abs(value[0]) and len(set(col[0].tolist())) == 4


# ------------------------------------------------------------------------------------------ the value block against the oracle's definition
@pytest.mark.parametrize('name,law', [('one_link', 'ld2'), ('one_wave', 'mixed'), ('two_waves', 'ld35'), ('closed', 'ld2')])
def test_the_reference_block_summed_along_a_placement_is_the_total_capacity(name, law):
    """Sum over r of values_ref[r, S_r] = the float64 reference's capacity of the links on an RB for that complete assignment, at
    1e-9 relative (the float64 identity bar of test_assign_cpu.py): random placements, everybody on one RB, nobody anywhere."""
    c, links, _, _ = shu.value_case(name, law)
    values, closed, _ = shu.values_ref(c, links)
    b, n, r, m = c['b'], c['n'], c['r'], len(links)
    rng = np.random.default_rng(4)
    open_rbs = [np.nonzero(closed[e] == 0)[0] for e in range(b)]
    placements = [np.stack([rng.choice(open_rbs[e], m) for e in range(b)]) for _ in range(6)]
    placements.append(np.stack([np.full(m, open_rbs[e][0]) for e in range(b)]))
    worst = 0.0
    for cols in placements:
        rb = np.array(c['rb'], dtype=np.int64)
        rb[:, links] = cols
        _, cap, _ = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rb[:, None], np.asarray(c['pwr'])[:, None], c, r)
        on = (rb >= 0) & (rb < r)
        want = (cap[:, 0] * on).sum(axis=1)
        got = np.array([shu.placement_total(values[e], cols[e]) for e in range(b)])
        worst = max(worst, float(np.abs(got / want - 1.0).max()))
    # the S = 0 column alone is the background
    rb = np.array(c['rb'], dtype=np.int64)
    rb[:, links] = -1
    _, cap, _ = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rb[:, None], np.asarray(c['pwr'])[:, None], c, r)
    want = (cap[:, 0] * ((rb >= 0) & (rb < r))).sum(axis=1)
    worst = max(worst, float(np.abs(values[:, :, 0].sum(axis=1) / want - 1.0).max()))
    print(f'{name}, {law}: the identity holds to {worst:.2e}')
    assert worst <= 1e-9


# ------------------------------------------------------------------------------------------ the GPU cases hold what they are there for
def test_the_value_cases_hold_what_they_are_there_for():
    for name, (b, cues, dues, r, m) in shu.VALUE_CASES.items():
        for law in shu.LAWS:
            c, links, allowed, other = shu.value_case(name, law)
            assert c['b'] == b and c['n'] == cues + dues and c['r'] == r and len(links) == m == len(set(links.tolist()))
            assert (np.diff(links) > 0).all() and not allowed[links[m // 2]].any() and other.shape == (b, c['n'])
            assert (np.asarray(other) != np.asarray(c['pwr'])).any()
            assert shu.value_case(name, law)[0] is c                     # the same arrays on every call
    assert [1 << v[4] for v in shu.VALUE_CASES.values()] == [2, 64, 128, 4096, 32]
    c, links, _, _ = shu.value_case('closed', 'ld2')
    movable = np.zeros(c['n'], bool)
    movable[links] = True
    for e in range(c['b']):
        members = [int((~movable & (c['rb'][e] == layer)).sum()) for layer in range(c['r'])]
        assert members[:3] == [64, 65, 0] and max(members[3:]) <= 64 and sum(members) == c['n'] - 5 - 3
    values, closed, near = shu.values_ref(c, links)
    assert closed.tolist() == [[0, 1, 0, 0, 0, 0, 0]] * 2 and np.isneginf(values[:, 1, 1:]).all() and (values[:, 1, 0] > 0).all()
    assert np.isfinite(values[:, [0, 2, 3, 4, 5, 6]]).all() and near.mean() <= shu.THRESHOLD_CAP
    rb, pwr = shu.candidates(c, links)
    assert rb.shape == (2, 7 * 32, 300) and (rb[:, 3 * 32 + 5, links] == np.array([3, 7, 3, 7, 7])).all()
    assert (rb[:, :, ~movable] == c['rb'][:, None, ~movable]).all() and (pwr == c['pwr'][:, None, :]).all()


def test_the_solve_cases_hold_what_they_are_there_for():
    shapes = {name: row[:3] for name, row in shu.SOLVE_CASES.items()}
    assert {s[2] for s in shapes.values()} == {1, 6, 7, 12} and {s[1] for s in shapes.values()} >= {1, 2, 25, 300}
    assert {s[0] for s in shapes.values()} >= {1, 70}
    for name in ('smallest', 'one_wave', 'every_tie', 'one_open_rb', 'quota_short', 'dead_between', 'two_waves_25_rbs'):
        v, quota = shu.solve_case(name)
        col, value, feasible = shu.solve_case_ref(name)
        b, r, m = shapes[name]
        assert v.shape == (b, r, 1 << m) and v.dtype == np.float64 and shu.solve_case(name)[0] is v
        if name == 'every_tie':
            assert (v == 2.5).all() and (col == 0).all() and (value == 2.5 * r).all()
        elif name == 'one_open_rb':
            assert (col == 2).all() and feasible.tolist() == [1] * b
        elif name == 'quota_short':
            assert feasible.tolist() == [0] * b and (col == -1).all() and (value == 0.0).all()
        elif name == 'dead_between':
            assert feasible.tolist() == [1, 0, 1] and (col[1] == -1).all() and (col[[0, 2]] >= 0).all()
        else:
            assert feasible.any()
        if name in ('one_wave', 'two_waves_25_rbs', 'dead_between'):
            assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
    # integers in 0 .. 2 on 25 RBs: the maximum is tied in every env that has one
    v, quota = shu.solve_case('two_waves_25_rbs')
    assert quota == 2 and set(np.unique(v[np.isfinite(v)]).tolist()) == {0.0, 1.0, 2.0}


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_share_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_share_library()
    assert _native.side_library('share') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_share.so') == declared == {'d2d_share_values', 'd2d_share_solve', 'd2d_share_last_error'}
    assert set(_native.SHARE_SIGNATURES) == declared and _native.EXACT['share'] is _native.SHARE_SIGNATURES
    # the signatures are the header's, argument for argument
    ctype = {'const float*': _native._P, 'const int32_t*': _native._P, 'const uint32_t*': _native._P, 'const double*': _native._P,
             'double*': _native._P, 'int32_t*': _native._P, 'uint16_t*': _native._P, 'void*': _native._P, 'int32_t': _native._I,
             'int64_t': _native.C.c_int64}
    for symbol in ('d2d_share_values', 'd2d_share_solve'):
        args = re.search(r'^int %s\((.*?)\);' % symbol, header, flags=re.M | re.S).group(1)
        kinds = [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args.replace('\n', ' ').split(',')]
        assert kinds == _native.SHARE_SIGNATURES[symbol][1], symbol
    assert len(_native.SHARE_SIGNATURES['d2d_share_values'][1]) == 20 and len(_native.SHARE_SIGNATURES['d2d_share_solve'][1]) == 10
    for symbol, (res, args) in _native.SHARE_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(lib.d2d_share_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MAX_LINKS', 'MAX_RBS', 'MAX_MOVABLE', 'MAX_BACKGROUND', 'MAX_LDS_BYTES',
                  'MAX_BLOCK_BYTES'):
        assert int(re.search(r'#define D2D_SHARE_%s (\d+)' % const, header).group(1)) == getattr(_native, 'SHARE_' + const), const
    assert _native.SHARE_MAX_MOVABLE == shu.MAX_MOVABLE == 12 and _native.SHARE_MAX_BACKGROUND == shu.MAX_BACKGROUND == 64
    assert _native.SHARE_MAX_LDS_BYTES == 160 * 1024 and _native.SHARE_MAX_BLOCK_BYTES == 8 * 1024 ** 3
    # the sixth table: present in the build, the digest and the headers, compiled and linked behind everything else
    assert build.EXACT == {'share': ['d2d_share.hip']} and set(build.EXACT) == set(_native.EXACT)
    assert build.WHOLE == {**build.ALL, **build.EXACT} and list(build.WHOLE) == list(build.ALL) + ['share']
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('share') == LIB_DIR / 'libd2d_share.so' == _native.side_path('share')
    assert 'share' in build.__doc__ and 'EXACT' in build.__doc__
    # the five old tables and ALL as they were
    assert build.ALL == {**build.TARGETS, **build.EXTRAS} and list(build.ALL) == list(build.TARGETS) + ['stable']
    assert build.EXTRAS == {'stable': ['d2d_stable.hip']} and list(_native.EXTRAS) == ['stable']
    assert build.FAMILIES == {'balance': ['d2d_balance.hip']} and list(_native.FAMILIES) == ['balance']
    assert len(build.LIBRARIES) == 14 and len(_native.SIDE) == 12 and set(build.SOLVERS) == set(_native.SOLVERS) == {'assign'}
    assert list(build.ADDONS) == list(_native.ADDONS) == ['assignpwr', 'color']
    for table in (build.LIBRARIES, build.SOLVERS, build.ADDONS, build.BUILT, build.EVERYTHING, build.FAMILIES, build.TARGETS, build.EXTRAS,
                  build.ALL, _native.SIDE, _native.SOLVERS, _native.ADDONS, _native.FAMILIES, _native.EXTRAS):
        assert 'share' not in table


def test_a_missing_share_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.exact_missing() == [] and build.exact_missing(tmp_path) == ['share']
    build.lib_path('share', tmp_path).touch()
    assert build.exact_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'exact_missing', lambda lib_dir=build.LIB_DIR: ['share'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built() and not build.addons_missing() \
        and not build.families_missing() and not build.extras_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_share\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_share_library()


# ------------------------------------------------------------------------------------------ the LDS formulas and the entry points
def _header_values_lds(n, m, power_law):
    """The formula as include/d2d_share.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    u, big = min(n, 64) + m, n + 12
    return r16(8 * -(-n // 64)) + r16(4 * u) + r16(4 * u * (u | 1)) + 32 * big + 2 * r16(4 * big) + r16(8 * big) \
        + (r16(8 * big) if power_law else 0)


def test_lds_bytes_are_the_headers_formulas():
    from gym_d2d_amd import _native, sharing
    header = HEADER.read_text()
    assert 'round16(8 ceil(n_links / 64)) + round16(4 U) + round16(4 U (U | 1)) + 32 L + 2 round16(4 L) + round16(8 L)' in header
    assert '26 * 2^n_movable bytes' in header
    for n, m in ((1, 1), (9, 1), (40, 12), (63, 5), (64, 12), (65, 12), (300, 5), (2048, 12)):
        for power_law in (False, True):
            assert sharing.values_lds_bytes(n, m, power_law) == _header_values_lds(n, m, power_law), (n, m)
    assert _header_values_lds(2048, 12, True) <= _native.SHARE_MAX_LDS_BYTES       # every shape within the limits is served
    assert _header_values_lds(2048, 12, True) > 64 * 1024 > _header_values_lds(300, 5, True)
    assert [sharing.solve_lds_bytes(m) for m in (1, 6, 12, 13)] == [52, 1664, 106496, 212992]
    assert sharing.solve_lds_bytes(12) <= _native.SHARE_MAX_LDS_BYTES < sharing.solve_lds_bytes(13)     # why M stops at 12


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=11, n_links=5, n_rbs=3, n_movable=2)

    def values(ptrs=tuple(range(8, 72, 8)), movable=80, allowed=0, out=(96, 104), **kw):
        a = dict(ok, **kw)
        _native.share_values(*ptrs, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'], movable, a['n_movable'],
                             allowed, *out)

    def solve(v=8, quota=0, out=(16, 24, 32, 40), **kw):
        a = dict(ok, **kw)
        _native.share_solve(v, quota, a['n_envs'], a['n_rbs'], a['n_movable'], *out)
    before = _native.share_values_launches, _native.share_solve_launches
    budget = r'need 8589967360 bytes, more than the 8589934592 \(D2D_SHARE_MAX_BLOCK_BYTES\)'
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=2049), r'n_links must be in \[1, 2048\]'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=8193), r'n_rbs must be in \[1, 8192\]'), (dict(n_envs=-1), 'n_envs'), (dict(n_dev=0), 'n_dev'),
                     (dict(n_movable=0), r'n_movable must be in \[1, 12\] \(D2D_SHARE_MAX_MOVABLE\)'), (dict(n_movable=13), r'n_movable must be in \[1, 12\]'),
                     (dict(n_movable=6), 'at most n_links'), (dict(law=3), 'unknown law'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(n_envs=209716, n_links=20, n_rbs=1, n_movable=12), budget),
                     (dict(movable=0), 'null device pointer'), (dict(out=(0, 104)), 'null device pointer'), (dict(out=(96, 0)), 'null device pointer'),
                     *((dict(ptrs=tuple(0 if i == z else 8 + 8 * i for i in range(8))), 'null device pointer') for z in range(8))):
        with pytest.raises(_native.NativeError, match=text):
            values(**kw)
    for kw, text in ((dict(n_movable=0), r'n_movable must be in \[1, 12\] \(D2D_SHARE_MAX_MOVABLE\)'), (dict(n_movable=13), r'n_movable must be in \[1, 12\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=8193), 'n_rbs'), (dict(n_envs=2 ** 31), 'n_envs'),
                     (dict(n_envs=209716, n_rbs=1, n_movable=12), budget), (dict(v=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 16 + 8 * i for i in range(4))), 'null device pointer') for z in range(4))):
        with pytest.raises(_native.NativeError, match=text):
            solve(**kw)
    values(n_envs=0)                                                     # nothing to do: accepted, and no launch on a device
    values(n_envs=0, n_links=2048, n_movable=12, law=1)
    solve(n_envs=0)
    solve(n_envs=0, n_movable=12, n_rbs=8192)
    assert (_native.share_values_launches, _native.share_solve_launches) == before


# ------------------------------------------------------------------------------------------ the host class on a stub sim
def _stub_sim(route=None, shadowing=False, num_rbs=4, links=4):
    from gym_d2d_amd.path_loss_table import NATIVE
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    d = 2 * links
    law = {'a_tx_db': [30.0] * d, 'a_rx_db': [0.0] * d, 'exponent': [3.5] * d, 'shadowing': shadowing}
    return SimpleNamespace(num_envs=3, handle=SimpleNamespace(num_devices=d), config=SimpleNamespace(num_rbs=num_rbs),
                           link_tx=np.arange(links), link_rx=np.arange(links, 2 * links), _dev_list=[dev] * d,
                           path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law=law),
                           fixed_positions=lambda: (np.zeros(d, bool), np.zeros((d, 2))))


def test_refusal_texts_name_share_rbs_and_the_pinned_rows_are_unchanged():
    from gym_d2d_amd import assignment, sensing, sharing
    assert sharing.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 7), np.array([[100.1, -20.3]] + [[0, 0]] * 7))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: sharing.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = sharing.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('share_rbs() ') and 'assign_rbs()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where assign_rbs() is, in its words
        assert assignment.refusal(*args).replace('assign_rbs()', 'share_rbs()') == texts[needle]
    assert sharing.REFUSAL == ('share_rbs()', *sensing.REFUSALS['assign_rbs'][1:])
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11


def test_shapes_are_refused_by_name_before_anything_is_launched():
    import torch
    from gym_d2d_amd import _native, assignment, sharing
    # M = 13, M = 0 and the byte budget
    with pytest.raises(ValueError, match=r'share_rbs\(\) places 1 to 12 movable links \(D2D_SHARE_MAX_MOVABLE.*got M = 13'):
        sharing.check_shape(4, 25, 13)
    with pytest.raises(ValueError, match=r'share_rbs\(\) places 1 to 12 movable links .*got M = 0'):
        sharing.check_shape(4, 25, 0)
    assert sharing.block_bytes(1024, 25, 12) == 1024 * 25 * 4096 * 10 and sharing.block_bytes(3, 2, 1) == 120
    sharing.check_shape(8388, 25, 12)                                    # 8 589 312 000 bytes
    with pytest.raises(ValueError, match=r'share_rbs\(\) keeps a value block and choice words of 8400 x 25 x 2\^12 entries: 8601600000 '
                                         r'bytes, more than the 8589934592 \(D2D_SHARE_MAX_BLOCK_BYTES\)'):
        sharing.check_shape(8400, 25, 12)
    # through the host class: 14 links of which 13 are movable, none movable, and the shapes of solve_sharing()
    cpu = torch.device('cpu')
    sim = _stub_sim(links=14)
    agent = np.arange(14) >= 1
    assign = assignment.Assignment(sim, 14, agent, agent, torch, cpu)
    k = sharing.Sharing(sim, 14, assign, torch, cpu)
    with pytest.raises(ValueError, match='does not match the env'):
        sharing.Sharing(_stub_sim(links=14), 14, assign, torch, cpu)
    f32, i32, f64 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s, dtype=torch.float64))
    planes = dict(pos_x=f32(3, 28), pos_y=f32(3, 28), rb=i32(3, 14), pwr=i32(3, 14))
    before = _native.share_values_launches, _native.share_solve_launches
    for call in (lambda mv: k.values(planes, mv, None, None, None, 0), lambda mv: k.rbs(planes, mv, None, None, None, None, 0)):
        with pytest.raises(ValueError, match=r'share_rbs\(\) places 1 to 12 movable links .*got M = 13'):
            call(None)
        with pytest.raises(ValueError, match=r'share_rbs\(\) places 1 to 12 movable links .*got M = 0'):
            call(np.zeros(14, bool))
        with pytest.raises(ValueError, match='movable marks link 0, which has no action column'):
            call(np.arange(14) < 2)
    few = np.arange(14) >= 10
    with pytest.raises(ValueError, match=r'power_dbm must be a contiguous int32 tensor \[3, 14\]'):
        k.values(planes, few, None, i32(3, 13), None, 0)
    with pytest.raises(ValueError, match=r'out must be \(values\)'):
        k.values(planes, few, None, None, f64(3, 4, 8), 0)
    with pytest.raises(ValueError, match=r'out must be \(rb, value_mbps, feasible, closed\)'):
        k.rbs(planes, few, None, None, None, (i32(3, 14), f32(3), i32(3)), 0)
    for bad in (-1, True, 1.5, [1, 1, 1], [1, 1, 1, -1], np.ones(4, bool), 'one'):
        with pytest.raises(ValueError, match=r'quota must be None, an int or \[4\] ints \(RB\), each >= 0'):
            k.rbs(planes, few, None, bad, None, None, 0)
    assert k.quota(None, 4, 4) is None and k.quota(2, 4, 4).tolist() == [2] * 4 and k.quota(2, 4, 4) is k.quota([2, 2, 2, 2], 4, 4)
    assert k.quota([0, 9, 1, 4], 4, 4).tolist() == [0, 4, 1, 4]          # a quota above M never binds
    with pytest.raises(ValueError, match=r'quota as a tensor must be contiguous int32 \[4\]'):
        k.quota(torch.ones(4, dtype=torch.int64), 4, 4)
    for bad in (f32(3, 4, 16), f64(4, 16), f64(3, 4, 1), f64(3, 4, 12), f64(3, 4, 32)[:, :, ::2], f64(3, 0, 16), np.zeros((3, 4, 16))):
        with pytest.raises(ValueError, match=r'values must be a contiguous float64 tensor \[B, R, 2\^M\]|a power of two in 2 \.\. 4096; got (1|12)'):
            k.solve(bad, None, None, 0)
    with pytest.raises(ValueError, match=r'a power of two in 2 \.\. 4096; got 8192'):
        k.solve(torch.empty(1, 1, 8192, dtype=torch.float64), None, None, 0)
    with pytest.raises(ValueError, match=r'out must be \(col, value, feasible\)'):
        k.solve(f64(3, 4, 16), None, (i32(3, 4), f32(3), i32(3)), 0)
    with pytest.raises(ValueError, match=r'8601600000 bytes together, more than the 8589934592 \(D2D_SHARE_MAX_BLOCK_BYTES\)'):
        meta = torch.device('meta')                                      # a shape without its memory
        sharing.Sharing._block(SimpleNamespace(torch=torch, device=meta), torch.empty(8400, 25, 4096, dtype=torch.float64, device=meta))
    assert (_native.share_values_launches, _native.share_solve_launches) == before


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_share_library', lambda: pytest.fail('libd2d_share.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._share is None
    for call in (lambda: env.share_rbs(), lambda: env.share_rbs(quota=2), lambda: env.share_rbs_actions(), lambda: env.sharing_values(),
                 lambda: env.solve_sharing(None)):
        with pytest.raises(ValueError, match=r'share_rbs\(\) needs the torch path'):
            call()
    assert env._share is None and env._assign is None
    env.close()


def test_share_rbs_actions_encode_the_solved_rbs_on_a_stubbed_handle(monkeypatch):
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
    env.share_rbs = lambda *a: seen.append(a) or (torch.as_tensor(rb, dtype=torch.int32), None, None, None)
    a = env.share_rbs_actions('mask', 'allowed', 2, 'power')
    assert seen == [('mask', 'allowed', 2, 'power')]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()

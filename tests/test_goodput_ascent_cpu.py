"""Queue-aware goodput ascent, the part that needs no GPU: the library's exported set and its place in the build, the entry point's
refusals, the host class on a stub sim, the properties of the float64 restatement (goodput_ascent_util.goodput_ref), and the
conditions the GPU cases are there for, re-derived on the restatement."""
import itertools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import goodput_ascent_util as gu
import power_control_util as pcu
from test_rb_ascent_cpu import _stub_sim

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_goodput.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_goodput.hip'
ARGS = ['pos_x', 'pos_y', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'law', 'pow_k', 'n_envs', 'n_dev', 'n_links', 'n_rbs',
        'p_min', 'p_max', 'weight', 'demand_bits', 'bits_per_mbps', 'allowed', 'movable', 'floor_db', 'move_mask', 'min_gain', 'max_rounds',
        'env_mask', 'rb_out', 'power_dbm', 'sinr_db', 'capacity_mbps', 'served_bits', 'value', 'rounds', 'moves', 'converged', 'hip_stream']


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_goodput_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_goodput_library()
    assert _native.side_library('goodput') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_goodput.so') == declared == {'d2d_goodput_ascent', 'd2d_goodput_last_error'}
    assert set(_native.GOODPUT_SIGNATURES) == declared and _native.LATER['goodput'] is _native.GOODPUT_SIGNATURES
    # the signature is the header's, argument for argument
    ctype = {'const float*': _native._P, 'const int32_t*': _native._P, 'const uint8_t*': _native._P, 'const uint32_t*': _native._P,
             'float*': _native._P, 'int32_t*': _native._P, 'int64_t*': _native._P, 'uint8_t*': _native._P, 'void*': _native._P,
             'int32_t': _native._I, 'int64_t': _native.C.c_int64, 'double': _native.C.c_double}
    args = re.search(r'^int d2d_goodput_ascent\((.*?)\);', header, flags=re.M | re.S).group(1)
    names = [a.strip().split()[-1].lstrip('*') for a in args.replace('\n', ' ').split(',')]
    kinds = [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args.replace('\n', ' ').split(',')]
    assert kinds == _native.GOODPUT_SIGNATURES['d2d_goodput_ascent'][1] and len(kinds) == 36
    assert names == ARGS                                                # the prefix is PairKernel.raw_launch_args with cap_cols
    for symbol, (res, argtypes) in _native.GOODPUT_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_goodput_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MOVE_RB', 'MOVE_POWER', 'MAX_LINKS', 'MAX_RBS', 'MAX_LEVELS', 'MAX_ROUNDS',
                  'MAX_WEIGHT', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_GOODPUT_%s (\d+)' % const, header).group(1)) == getattr(_native, 'GOODPUT_' + const), const
    assert _native.GOODPUT_MAX_LDS_BYTES == 160 * 1024 and _native.GOODPUT_MAX_WEIGHT == 1 << 20 and _native.GOODPUT_MAX_LEVELS == 64
    assert 2048 * (1 << 20) * ((1 << 31) - 1) < 1 << 62                 # V < 2^62: int64 sums are exact
    # the table behind EVERY: in the build, the digest and the headers, compiled and linked behind everything else
    assert 'goodput' in build.LATER and 'goodput' in _native.LATER and list(build.LATER) == list(_native.LATER)
    assert build.LATER['goodput'] == ['d2d_goodput.hip'] and build.COMPLETE == {**build.EVERY, **build.LATER}
    assert list(build.COMPLETE)[-1] == 'goodput' and 'goodput' not in build.EVERY
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('goodput') == LIB_DIR / 'libd2d_goodput.so' == _native.side_path('goodput')
    assert 'goodput' in build.__doc__ and '4.24' in build.__doc__
    assert _native.goodput_launches >= 0 and callable(_native.goodput_ascent)


def test_a_missing_goodput_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and build.later_missing(tmp_path) == list(build.LATER)
    build.lib_path('rbascent', tmp_path).touch()
    assert build.later_missing(tmp_path) == [s for s in build.LATER if s != 'rbascent'] and 'goodput' in build.later_missing(tmp_path)
    for stem in build.LATER:
        build.lib_path(stem, tmp_path).touch()
    assert build.later_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'later_missing', lambda lib_dir=build.LIB_DIR: ['goodput'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and not build.growing_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_goodput\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_goodput_library()


# ------------------------------------------------------------------------------------------ the LDS formula and the entry point
def _header_lds(n, r, allowed=False):
    """The formula as include/d2d_goodput.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    return 96 * n + (r16(4 * n * ((r + 31) // 32)) if allowed else 0) + r16(4 * ((n + 31) // 32) * r) + 208


def _call(ptr=8, p_min=8, weight=0, demand=0, bpm=1000.0, allowed=0, movable=0, floor=0, mask=0, out=tuple(range(8, 80, 8)), **kw):
    from gym_d2d_amd import _native
    a = dict(dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, move=3, min_gain=0, max_rounds=4), **kw)
    _native.goodput_ascent(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                           p_min, ptr, weight, demand, bpm, allowed, movable, floor, a['move'], a['min_gain'], a['max_rounds'], mask, *out)


def test_lds_bytes_are_the_headers_formula_on_both_sides_of_the_limit():
    from gym_d2d_amd import _native, goodput_ascent
    header = ' '.join(HEADER.read_text().replace(' *', ' ').split())
    assert '96 n_links + has_allowed round16(4 n_links ceil(n_rbs / 32)) + round16(4 ceil(n_links / 32) n_rbs) + 208' in header
    for n, r in ((1, 1), (37, 5), (300, 7), (1000, 64), (1600, 50), (2048, 256)):
        for allowed in (False, True):
            assert goodput_ascent.lds_bytes(n, r, allowed) == _header_lds(n, r, allowed), (n, r)
    limit = _native.GOODPUT_MAX_LDS_BYTES
    assert _header_lds(1000, 64) > 64 * 1024 > _header_lds(300, 7)
    # what the header and the README state: 1600 links on up to 50 RBs, 512 links on up to 1788, nothing past 1702 links
    assert _header_lds(1600, 50) <= limit < _header_lds(1600, 51)
    assert _header_lds(512, 1788) <= limit < _header_lds(512, 1789)
    assert _header_lds(1702, 1) <= limit < _header_lds(1703, 1)
    assert '1600 links on up to 50 RBs' in HEADER.read_text() and '1600 links on up to 50 RBs' in (ROOT / 'README.md').read_text()
    # the entry point refuses and accepts on the same sides, before any launch (n_envs = 0: nothing to do)
    before = _native.goodput_launches
    for n, r, allowed in ((1600, 51, 0), (512, 1789, 0), (1703, 1, 0), (2048, 1, 0), (1600, 50, 8), (256, 8192, 0)):
        need = _header_lds(n, r, bool(allowed))
        assert need > limit
        with pytest.raises(_native.NativeError, match=rf'n_links and n_rbs need {need} bytes of LDS, more than the 163840 a workgroup can have'):
            _call(n_links=n, n_rbs=r, allowed=allowed, n_envs=0)
    for n, r, allowed in ((1600, 50, 0), (512, 1788, 0), (1702, 1, 0), (1400, 50, 8), (1, 1, 0)):
        assert _header_lds(n, r, bool(allowed)) <= limit
        _call(n_links=n, n_rbs=r, allowed=allowed, n_envs=0)
    assert _native.goodput_launches == before


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    before = _native.goodput_launches
    nine = 'rb_out, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves and converged must be nine arrays'
    good = tuple(range(8, 80, 8))
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.GOODPUT_MAX_LINKS + 1), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=_native.GOODPUT_MAX_RBS + 1), 'n_rbs'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'), (dict(max_rounds=0), r'max_rounds must be in \[1, 4096\]'),
                     (dict(max_rounds=4097), 'max_rounds'), (dict(max_rounds=-2), 'max_rounds'),
                     (dict(move=0), r'move_mask must be 1 \(RBs\), 2 \(powers\) or 3 \(both\)'), (dict(move=4), 'move_mask'), (dict(move=-1), 'move_mask'),
                     (dict(min_gain=-1), r'min_gain must be in \[0, 2\^62\)'), (dict(min_gain=1 << 62), 'min_gain'),
                     (dict(bpm=0.0), 'bits_per_mbps must be finite and > 0'), (dict(bpm=-1.0), 'bits_per_mbps'),
                     (dict(bpm=float('nan')), 'bits_per_mbps'), (dict(bpm=float('inf')), 'bits_per_mbps'),
                     (dict(law=3), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(ptr=0), 'null device pointer'), (dict(p_min=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else v for i, v in enumerate(good))), 'null device pointer') for z in range(9)),
                     (dict(out=(8, 8, *good[2:])), nine), (dict(out=(*good[:8], 24)), 'must be nine arrays'),
                     (dict(out=(*good[:5], 56, *good[6:])), 'must be nine arrays')):
        with pytest.raises(_native.NativeError, match=text):
            _call(**kw)
    for kw in (dict(), dict(weight=8, demand=8, allowed=8, movable=8, floor=8, mask=8), dict(move=1), dict(move=2), dict(max_rounds=4096),
               dict(min_gain=(1 << 62) - 1), dict(bpm=1e12), dict(law=2, pow_k=4), dict(law=1)):
        _call(n_envs=0, **kw)                                           # nothing to do: accepted, and no launch on a device
    assert _native.goodput_launches == before


def test_the_turn_loop_touches_no_global_memory_and_its_barriers_stand_on_scalar_decisions():
    """The source between the start of the rounds and the planes behind them names none of the argument struct's pointers; the two
    barriers inside stand behind readfirstlane'd decisions; the result pointers wait in LDS; the source holds no `atomic`."""
    src = SOURCE.read_text()
    loop = src[src.index('// ---- the rounds'):src.index("// ---- evaluate_kernel's planes for the state the ascent stopped at")]
    assert set(re.findall(r'\ba\.(\w+)', loop)) == {'max_rounds', 'move_mask', 'pow_k', 'bits_per_mbps', 'min_gain'}
    assert loop.count('__syncthreads()') == 2 and loop.count('__builtin_amdgcn_readfirstlane') == 2
    assert 'out.' not in loop and 'blockIdx' not in loop
    assert loop.count('walk<MODE>(') == 1                               # one walk, one call site: the leaving pass is its first pass
    assert 'atomic' not in src


# ------------------------------------------------------------------------------------------ the host module on a stub sim
def test_refusal_texts_name_goodput_ascent_and_the_pinned_rows_are_unchanged():
    from gym_d2d_amd import goodput_ascent, rb_ascent, sensing
    assert goodput_ascent.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: goodput_ascent.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = goodput_ascent.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('goodput_ascent() ') and 'rb_ascent()' not in text \
            and 'best_response_dynamics()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where rb_ascent() is
        assert rb_ascent.refusal(*args) is not None
    row = goodput_ascent.REFUSAL                                        # derived the way rb_ascent.REFUSAL is
    assert row[0] == 'goodput_ascent()' and row[1:] == rb_ascent.REFUSAL[1:] and row[1:3] == sensing.REFUSALS['best_response_dynamics'][1:3]
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11


def _kernel(torch, **kw):
    from gym_d2d_amd import goodput_ascent
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    p_min, p_max = np.zeros(4, np.int32), np.array([23, 23, 20, 20], np.int32)
    return goodput_ascent.GoodputAscent(_stub_sim(**kw), 4, p_min, p_max, agent, torch, torch.device('cpu'))


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import _native, goodput_ascent, sensing
    cpu = torch.device('cpu')
    k = _kernel(torch)
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4) and k.law == _native.GOODPUT_LAW_POW_K
    assert len(k.ptrs) == 4 and tuple(k.cap_cols.shape) == (2, 7) and len(k.raw_launch_args(1, 2, 3, 4)) == 14
    assert k.movable(None).tolist() == [0, 1, 1, 1] and k.movable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    assert k.floor(None, 2).tolist() == [-np.inf] * 4 and k.floor({'cue': 0.0, 'due': -np.inf}, 2).tolist() == [0.0, 0.0, -np.inf, -np.inf]
    assert k.words(None) is None and tuple(k.words(np.ones((4, 4), bool)).shape) == (4, 1)
    assert k.p_min.tolist() == [0] * 4 and k.p_max.tolist() == [23, 23, 20, 20] and k.p_min.dtype == torch.int32
    # move
    assert [goodput_ascent.move_mask(m) for m in (('rb', 'power'), ['power', 'rb'], ('rb',), 'rb', 'power', {'power'})] == [3, 3, 1, 1, 2, 2]
    for bad in ((), [], None, 'both', ('rb', 'pwr'), 3, ('rb', 1)):
        with pytest.raises(ValueError, match="move must name 'rb', 'power' or both"):
            goodput_ascent.move_mask(bad)
    # weight and demand planes: scalars and [N] rows broadcast; host values are checked, tensors are not read
    assert k.plane(None, 'weight', 0, 5) is None
    for v in (3, np.int64(3), np.full(4, 3), np.full((3, 4), 3, np.int16), torch.full((4,), 3, dtype=torch.int64), torch.tensor(3, dtype=torch.int32)):
        got = k.plane(v, 'weight', 0, 1 << 20)
        assert got.dtype == torch.int32 and tuple(got.shape) == (3, 4) and got.is_contiguous() and (got == 3).all()
    assert k.plane(np.arange(4), 'weight', 0, 3).tolist() == [[0, 1, 2, 3]] * 3
    assert k.plane(torch.tensor([2 ** 40, -2 ** 40, 5, -5]), 'demand_bits', -2 ** 31, 2 ** 31 - 1).tolist() == [[2 ** 31 - 1, -2 ** 31, 5, -5]] * 3
    assert k.plane(-7, 'demand_bits', -2 ** 31, 2 ** 31 - 1).tolist() == [[-7] * 4] * 3                # a negative demand is the kernel's 0
    for bad in ((1 << 20) + 1, -1, np.array([0, 1, 2, (1 << 20) + 1])):
        with pytest.raises(ValueError, match=r'weight must lie in \[0, 1048576\]'):
            k.plane(bad, 'weight', 0, 1 << 20)
    with pytest.raises(ValueError, match=r'demand_bits must lie in'):
        k.plane(1 << 31, 'demand_bits', -2 ** 31, 2 ** 31 - 1)
    for bad in (1.0, True, np.ones(4), np.ones(3, np.int32), np.ones((4, 3), np.int32), torch.ones(4), torch.ones(5, dtype=torch.int32), 'x'):
        with pytest.raises(ValueError, match=r'weight must be None or ints, a scalar, \[4\] or \[3, 4\]'):
            k.plane(bad, 'weight', 0, 1 << 20)
    # out=, the scalars, the masks: refused before any launch
    i32, f32, u8 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    good = (i32(3, 4), i32(3, 4), f32(3, 4), f32(3, 4), i32(3, 4), torch.zeros(3, dtype=torch.int64), i32(3), i32(3), u8(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4)] * 5 + [(3,)] * 4
    assert [o.dtype for o in k.outputs(None)] == [o.dtype for o in good]
    planes = dict(pos_x=f32(3, 7), pos_y=f32(3, 7), rb=i32(3, 4), pwr=i32(3, 4))
    mov, floor = k.movable(None), k.floor(None, 2)
    both = ('rb', 'power')
    before = _native.goodput_launches
    for out in (good[:8], (*good[:5], i32(3), *good[6:]), (*good[:6], good[7], good[7], good[8]), good[0], (good[0], f32(3, 4), *good[2:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, power_dbm, sinr_db, capacity_mbps, served_bits, value, rounds, moves, converged\)'):
            k.solve(planes, 5, None, 1000.0, both, None, mov, floor, 0, 16, out, 0)
    for bad in (-1, 0.5, 1.0, True, '1', None, 1 << 62):
        with pytest.raises(ValueError, match=r'min_gain_bits must be an int in \[0, 2\^62\)'):
            k.solve(planes, 5, None, 1000.0, both, None, mov, floor, bad, 16, None, 0)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match=r'max_rounds must be an int in \[1, 4096\]'):
            k.solve(planes, 5, None, 1000.0, both, None, mov, floor, 0, bad, None, 0)
    for bad in (0, -1.0, float('nan'), float('inf'), True, '1', None):
        with pytest.raises(ValueError, match='bits_per_mbps must be a finite number > 0'):
            k.solve(planes, 5, None, bad, both, None, mov, floor, 0, 16, None, 0)
    with pytest.raises(ValueError, match='move must name'):
        k.solve(planes, 5, None, 1000.0, (), None, mov, floor, 0, 16, None, 0)
    with pytest.raises(ValueError, match=r'allowed must be bool \[4, 4\]'):
        k.solve(planes, 5, None, 1000.0, both, np.ones((4, 5), bool), mov, floor, 0, 16, None, 0)
    with pytest.raises(ValueError, match='weight must lie'):
        k.solve(planes, 5, 1 << 21, 1000.0, both, None, mov, floor, 0, 16, None, 0)
    with pytest.raises(ValueError, match='env_mask must be'):
        k.solve(planes, 5, None, 1000.0, both, None, mov, floor, 0, 16, None, 0, env_mask=np.ones(4, bool))
    assert _native.goodput_launches == before
    # the shapes and classes the object refuses when it is made
    from gym_d2d_amd.goodput_ascent import GoodputAscent
    agent = np.array([False, True, True, True])
    with pytest.raises(ValueError, match=r'goodput_ascent\(\) serves at most 8192 RBs'):
        _kernel(torch, num_rbs=8193)
    with pytest.raises(ValueError, match='the agent mask does not match the env'):
        GoodputAscent(_stub_sim(), 4, np.zeros(4, np.int32), np.ones(4, np.int32), agent[:3], torch, cpu)
    with pytest.raises(ValueError, match='the power bounds do not match the env'):
        GoodputAscent(_stub_sim(), 4, np.ones(4, np.int32), np.zeros(4, np.int32), agent, torch, cpu)
    with pytest.raises(ValueError, match=r'goodput_ascent\(\) .* at most 64 levels \(D2D_GOODPUT_MAX_LEVELS\), got 65'):
        GoodputAscent(_stub_sim(), 4, np.zeros(4, np.int32), np.array([23, 23, 64, 20], np.int32), agent, torch, cpu)
    GoodputAscent(_stub_sim(), 4, np.zeros(4, np.int32), np.array([64, 23, 63, 20], np.int32), agent, torch, cpu)    # 64 levels; link 0 never moves

    def wide(n, r):
        return SimpleNamespace(**{**vars(_stub_sim(num_rbs=r)), 'link_tx': np.ones(n, dtype=np.int64), 'link_rx': np.zeros(n, dtype=np.int64)})
    with pytest.raises(ValueError, match=rf'goodput_ascent\(\) .*1600 links on 51 RBs need {_header_lds(1600, 51)} bytes, more than 163840'):
        GoodputAscent(wide(1600, 51), 1600, np.zeros(1600, np.int32), np.ones(1600, np.int32), np.ones(1600, bool), torch, cpu)
    k = GoodputAscent(wide(1600, 50), 1600, np.zeros(1600, np.int32), np.ones(1600, np.int32), np.ones(1600, bool), torch, cpu)
    with pytest.raises(ValueError, match=rf'need {_header_lds(1600, 50, True)} bytes with an allowed mask, more than 163840'):
        k.need(True)
    assert k.need(False) == _header_lds(1600, 50)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_goodput_library', lambda: pytest.fail('libd2d_goodput.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._goodput is None
    for call in (lambda: env.goodput_ascent(), lambda: env.goodput_ascent(100, None, 1000.0), lambda: env.goodput_ascent_actions()):
        with pytest.raises(ValueError, match=r'goodput_ascent\(\) needs the torch path'):
            call()
    assert env._goodput is None
    doc = VecD2DEnv.goodput_ascent.__doc__
    for needle in ('max-weight', 'backlog_bits >> k', 'arrive or expire', 'no off state', 'lowest', 'never both', 'nothing is synchronised'):
        assert needle in doc, needle
    env.close()


def test_goodput_ascent_actions_encode_the_solved_rbs_and_powers_on_a_stubbed_handle(monkeypatch):
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
    seen = []
    env.goodput_ascent = lambda *a: seen.append(a) or (torch.as_tensor(rb, dtype=torch.int32), torch.as_tensor(power, dtype=torch.int32)) + (None,) * 7
    a = env.goodput_ascent_actions(7, 2, 1000.0, ('power',), 'mask', 'some', {'cue': 0.0, 'due': 5.0}, 3, 9)
    assert seen == [(7, 2, 1000.0, ('power',), 'mask', 'some', {'cue': 0.0, 'due': 5.0}, 3, 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()


# ------------------------------------------------------------------------------------------ the restatement's properties
def _tiny(seed, n, r, levels=4):
    """A case of a few links on r RBs whose classes have `levels` power levels each, so that every state can be enumerated."""
    from oracle import d2d_oracle as orc
    from sim_util import default_links, random_layout
    cues, dues = 1, n - 1
    rng = np.random.default_rng(seed)
    pos = random_layout(rng, 1, cues, dues, cell_radius=150.0)
    tx, rx, _ = default_links(cues, dues)
    p_min = np.array([14] * cues + [8] * dues)
    return SimpleNamespace(name=f'gptiny{seed}_{n}_{r}', cues=cues, dues=dues, n=n, r=r, pos=pos, rb=rng.integers(0, r, (1, n)),
                           pwr=(p_min + rng.integers(0, levels, n))[None, :], tx=tx, rx=rx, p_min=p_min, p_max=p_min + levels - 1,
                           spec=orc.PathLossSpec('log_distance', 2.1, ple=2.0), cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


def test_every_move_raises_v_and_tiny_cases_end_at_or_below_the_brute_force_optimum():
    strictly = 0
    for seed in range(6):
        n, r = (3, 2) if seed % 2 else (4, 2)
        c = _tiny(200 + seed, n, r)
        rng = np.random.default_rng(seed)
        demand = np.where(rng.random((1, n)) < 0.4, rng.integers(100, 1500, (1, n)), gu.UNCAPPED)
        weight = rng.integers(1, 4, (1, n))
        ref = gu.goodput_ref(c, [0], demand, weight, gu.BPM, max_rounds=64)
        assert ref.converged[0]
        assert all(after > before for _, _, before, after in ref.raised) and len(ref.raised) == ref.moves[0]
        states = [np.array(s) for s in itertools.product(*([range(r)] * n + [range(c.p_min[j], c.p_max[j] + 1) for j in range(n)]))]
        rows = np.array(states)
        cap = gu.oracle_planes(c, 0, rows[:, :n], rows[:, n:])[1]
        dem, wgt = gu.planes_of(demand, weight, 1, n)
        values = (wgt * np.minimum(gu.budget64(cap, gu.BPM), dem)).sum(axis=1)
        at = lambda rb, p: int(values[(rows == np.concatenate([rb, p])[None, :]).all(axis=1)][0])
        start, got = at(c.rb[0], c.pwr[0]), at(ref.rb[0], ref.power_dbm[0])
        assert got == ref.value[0] and start <= got <= values.max()
        if ref.raised:
            assert ref.raised[0][2] == start and ref.raised[-1][3] == got
        # no single coordinate of a single link gains: integers, so exactly
        final = np.concatenate([ref.rb[0], ref.power_dbm[0]])
        diff = rows != final[None, :]
        one_away = (diff.sum(axis=1) == 1)
        assert (values[one_away] <= got).all()
        strictly += got > start
    assert strictly >= 3


@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False)])
def test_the_reference_alone_keeps_met_floors_and_stays_inside_the_cap_at_its_own_fixed_point(name, floors):
    """At the restatement's own fixed point no float64-admissible candidate has a positive Delta64 (worst <= 0 of the slack), the
    share of checks left out for a SINR within W of a floor or a sensitivity is under the cap, every move raised V64, and a link that
    met its floor at the start meets it at the end."""
    c, b, mov, demand, weight, bpm = gu.case_inputs(name, 'mix')
    ref = gu.reference(name, floors)
    floor = gu.FLOORS if floors else None
    assert len(ref.raised) == ref.moves.sum() > 0 and all(after > before for _, _, before, after in ref.raised)
    assert ref.converged.all()
    chk = gu.reference_check(c, np.arange(b), ref.rb, ref.power_dbm, ref.converged, demand, weight, bpm, movable=mov, floor=floor)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e}')
    assert chk.checks > 1000 and chk.left_out <= gu.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 0.0
    if floors:
        fl = gu.floor_vector(gu.FLOORS, c.cues, c.dues).astype(np.float64)
        for x in range(b):
            s0 = gu.oracle_planes(c, x, ref.start_rb[x][None, :], ref.start_pwr[x][None, :])[0][0]
            s1 = gu.oracle_planes(c, x, ref.rb[x][None, :], ref.power_dbm[x][None, :])[0][0]
            met = s0 >= fl
            assert met.any() and (s1[met] >= fl[met]).all()


def test_the_patterns_hold_what_they_are_there_for():
    c, b, mov, demand, weight, bpm = gu.case_inputs('n37_r5', 'mix')
    assert (demand < 0).any() and (demand == 0).any() and ((demand > 0) & (demand < 400)).any() and (demand == gu.UNCAPPED).any()
    assert set(np.unique(weight)) == {0, 1, 1 << 20}
    zero = gu.pattern('zero', b, c.n)
    assert (zero[0] == 0).all() and zero[1] is None
    assert gu.pattern('uncapped', b, c.n)[:2] == (gu.UNCAPPED, None)
    sat = gu.pattern('saturate', b, c.n)
    cap = gu.oracle_planes(c, 0, c.rb[0][None, :], c.pwr[0][None, :])[1][0]
    assert sat[0] == gu.UNCAPPED and (gu.budget64(cap, sat[2]) == gu.UNCAPPED).any() and (gu.budget64(cap, bpm) < gu.UNCAPPED).all()
    # the budget rule is queue_util's, and the float64 one agrees with it on float32 values
    from queue_util import budget_bits
    assert gu.budget_bits is budget_bits
    x = np.array([np.nan, -1.0, 0.0, 0.5, 1.0, 3.0e9, np.inf], dtype=np.float32)
    assert budget_bits(x, 1000.0).tolist() == gu.budget64(x, 1000.0).tolist() == [0, 0, 0, 500, 1000, gu.UNCAPPED, gu.UNCAPPED]
    # all demand zero: the restatement makes no move and V is 0
    ref = gu.goodput_ref(c, [0, 1], zero[0][:2], None, bpm)
    assert ref.moves.sum() == 0 and ref.converged.all() and (ref.value == 0).all()

"""Sum-capacity RB ascent, the part that needs no GPU: the library's exported set and its place in the build, the entry point's
refusals, the host class on a stub sim, the properties of the float64 restatement (rb_ascent_util.rb_ascent_ref), and the
conditions the GPU cases are there for, re-derived on the restatement."""
import itertools
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import power_control_util as pcu
import rb_ascent_util as ru

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_rbascent.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_rbascent.hip'


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_rbascent_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_rbascent_library()
    assert _native.side_library('rbascent') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_rbascent.so') == declared == {'d2d_rb_ascent', 'd2d_rbascent_last_error'}
    assert set(_native.RBASCENT_SIGNATURES) == declared and _native.LATER['rbascent'] is _native.RBASCENT_SIGNATURES
    # the signature is the header's, argument for argument
    ctype = {'const float*': _native._P, 'const int32_t*': _native._P, 'const uint8_t*': _native._P, 'const uint32_t*': _native._P,
             'float*': _native._P, 'int32_t*': _native._P, 'uint8_t*': _native._P, 'void*': _native._P, 'int32_t': _native._I,
             'int64_t': _native.C.c_int64, 'double': _native.C.c_double}
    args = re.search(r'^int d2d_rb_ascent\((.*?)\);', header, flags=re.M | re.S).group(1)
    names = [a.strip().split()[-1].lstrip('*') for a in args.replace('\n', ' ').split(',')]
    kinds = [ctype[re.sub(r'\s*\w+$', '', a.strip())] for a in args.replace('\n', ' ').split(',')]
    assert kinds == _native.RBASCENT_SIGNATURES['d2d_rb_ascent'][1] and len(kinds) == 27
    # the prefix is PairKernel.raw_launch_args with cap_cols, then the issue's order
    assert names == ['pos_x', 'pos_y', 'rb', 'pwr_dbm', 'link_tx', 'link_rx', 'dev_cols', 'cap_cols', 'law', 'pow_k', 'n_envs', 'n_dev',
                     'n_links', 'n_rbs', 'allowed', 'movable', 'floor_db', 'min_gain_mbps', 'max_rounds', 'env_mask', 'rb_out', 'sinr_db',
                     'capacity_mbps', 'rounds', 'moves', 'converged', 'hip_stream']
    for symbol, (res, argtypes) in _native.RBASCENT_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == argtypes
    assert isinstance(lib.d2d_rbascent_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MAX_LINKS', 'MAX_RBS', 'MAX_ROUNDS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_RBASCENT_%s (\d+)' % const, header).group(1)) == getattr(_native, 'RBASCENT_' + const), const
    assert _native.RBASCENT_MAX_LDS_BYTES == 160 * 1024 and _native.RBASCENT_MAX_ROUNDS == 4096
    # the table behind EVERY: in the build, the digest and the headers, compiled and linked behind everything else; its length is
    # nobody's business
    assert 'rbascent' in build.LATER and 'rbascent' in _native.LATER and set(build.LATER) == set(_native.LATER)
    assert build.LATER['rbascent'] == ['d2d_rbascent.hip']
    assert list(build.COMPLETE)[:len(build.EVERY)] == list(build.EVERY) and build.COMPLETE == {**build.EVERY, **build.LATER}
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('rbascent') == LIB_DIR / 'libd2d_rbascent.so' == _native.side_path('rbascent')
    assert 'rbascent' in build.__doc__ and 'LATER' in build.__doc__
    # the tables before it are as they were
    assert build.GROWING == {'ascent': ['d2d_ascent.hip']} and set(_native.GROWING) == {'ascent'}
    assert build.EVERY == {**build.WHOLE, **build.GROWING} and 'rbascent' not in build.EVERY
    assert _native.rbascent_launches >= 0 and callable(_native.rb_ascent)


def test_a_missing_rbascent_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.later_missing() == [] and 'rbascent' in build.later_missing(tmp_path)
    assert build.growing_missing(tmp_path) == ['ascent']
    for stem in build.LATER:
        build.lib_path(stem, tmp_path).touch()
    assert build.later_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'later_missing', lambda lib_dir=build.LIB_DIR: ['rbascent'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built() and not build.addons_missing() \
        and not build.families_missing() and not build.extras_missing() and not build.exact_missing() and not build.growing_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_rbascent\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_rbascent_library()


# ------------------------------------------------------------------------------------------ the LDS formula and the entry point
def _header_lds(n, r, power_law, allowed=False):
    """The formula as include/d2d_rbascent.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    n4 = (n + 3) // 4 * 4
    return (48 * n + (r16(8 * n) if power_law else 0) + 8 * n4 + (r16(4 * n * ((r + 31) // 32)) if allowed else 0)
            + r16(4 * ((n + 31) // 32) * r) + 112)


def test_lds_bytes_are_the_headers_formula_and_the_readme_states_the_largest_shape():
    from gym_d2d_amd import _native, rb_ascent
    header = ' '.join(HEADER.read_text().replace(' *', ' ').split())
    assert ('48 n_links + has_power_law round16(8 n_links) + 8 n4 + has_allowed round16(4 n_links ceil(n_rbs / 32)) '
            '+ round16(4 ceil(n_links / 32) n_rbs) + 112') in header
    for n, r in ((1, 1), (37, 5), (300, 7), (1000, 64), (2048, 256)):
        for power_law in (False, True):
            for allowed in (False, True):
                assert rb_ascent.lds_bytes(n, r, power_law, allowed) == _header_lds(n, r, power_law, allowed), (n, r)
    limit = _native.RBASCENT_MAX_LDS_BYTES
    assert _header_lds(1000, 64, True) > 64 * 1024 > _header_lds(300, 7, True)
    assert _header_lds(2048, 256, False) > limit
    # what the README row states: 2048 links on up to 127 RBs (191 with the inverse-square law), 128 links on 8192 RBs
    assert _header_lds(2048, 127, True) <= limit < _header_lds(2048, 128, True)
    assert _header_lds(2048, 191, False) <= limit < _header_lds(2048, 192, False)
    assert _header_lds(128, 8192, True) <= limit < _header_lds(129, 8192, True)
    readme = (ROOT / 'README.md').read_text()
    assert '2048 links on up to 127 RBs' in readme and '128 links on 8192 RBs' in readme


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, min_gain=0.0, max_rounds=4)

    def call(ptr=8, allowed=0, movable=0, floor=0, mask=0, out=(8, 16, 24, 32, 40, 48), **kw):
        a = dict(ok, **kw)
        _native.rb_ascent(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                          allowed, movable, floor, a['min_gain'], a['max_rounds'], mask, *out)
    before = _native.rbascent_launches
    big = _header_lds(2048, 128, True)
    with_mask = _header_lds(2048, 127, True, True)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.RBASCENT_MAX_LINKS + 1), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=_native.RBASCENT_MAX_RBS + 1), 'n_rbs'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'), (dict(max_rounds=0), r'max_rounds must be in \[1, 4096\]'),
                     (dict(max_rounds=4097), 'max_rounds'), (dict(max_rounds=-2), 'max_rounds'),
                     (dict(min_gain=-0.5), 'min_gain_mbps must be finite and >= 0'),
                     (dict(min_gain=float('nan')), 'min_gain_mbps'), (dict(min_gain=float('inf')), 'min_gain_mbps'),
                     (dict(law=3), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(ptr=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 8 * (i + 1) for i in range(6))), 'null device pointer') for z in range(6)),
                     (dict(out=(8, 8, 24, 32, 40, 48)), 'rb_out, sinr_db, capacity_mbps, rounds, moves and converged must be six arrays'),
                     (dict(out=(8, 16, 24, 32, 40, 24)), 'must be six arrays'), (dict(out=(8, 16, 24, 40, 40, 48)), 'must be six arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=128, law=1), rf'n_links and n_rbs need {big} bytes of LDS, more than the 163840 a workgroup can have'),
                     (dict(n_links=2048, n_rbs=127, law=1, allowed=8), rf'need {with_mask} bytes of LDS'),
                     (dict(n_links=2048, n_rbs=192), 'bytes of LDS'), (dict(n_links=2048, n_rbs=128, law=1, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(allowed=8, movable=8, floor=8, mask=8), dict(n_links=2048, n_rbs=127, law=1), dict(n_links=2048, n_rbs=191),
               dict(max_rounds=4096), dict(min_gain=3.5), dict(n_links=128, n_rbs=8192, law=1)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.rbascent_launches == before


def test_the_turn_loop_touches_no_global_memory_and_its_barriers_stand_on_scalar_decisions():
    """The source between the start of the rounds and the planes behind them names none of the argument struct's pointers; the two
    barriers inside stand behind readfirstlane'd decisions; the source holds no `atomic`."""
    src = SOURCE.read_text()
    loop = src[src.index('// ---- the rounds'):src.index('// ---- evaluate_kernel\'s planes for the RBs the ascent stopped at')]
    used = set(re.findall(r'\ba\.(\w+)', loop))
    assert used == {'max_rounds', 'pow_k', 'min_gain'}
    assert loop.count('__syncthreads()') == 2 and loop.count('__builtin_amdgcn_readfirstlane') == 3
    assert 'results_behind_the_loop()' not in loop
    assert 'atomic' not in src


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


def test_refusal_texts_name_rb_ascent_and_the_pinned_rows_are_unchanged():
    from gym_d2d_amd import power_ascent, rb_ascent, sensing
    assert rb_ascent.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: rb_ascent.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = rb_ascent.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('rb_ascent() ') and 'power_ascent()' not in text \
            and 'best_response_dynamics()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where power_ascent() is
        assert power_ascent.refusal(*args) is not None
    row = rb_ascent.REFUSAL
    assert row[0] == 'rb_ascent()' and row[1:3] == sensing.REFUSALS['best_response_dynamics'][1:3] and row[4] == 'planes'
    assert row[3] in texts['ShadowingPathLoss']
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import _native, rb_ascent, sensing
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    cpu = torch.device('cpu')
    k = rb_ascent.RbAscent(_stub_sim(), 4, agent, torch, cpu)
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4) and k.law == _native.RBASCENT_LAW_POW_K
    assert len(k.ptrs) == 4 and tuple(k.cap_cols.shape) == (2, 7)       # opened with capacity=True
    assert len(k.raw_launch_args(1, 2, 3, 4)) == 14
    assert k.movable(None).tolist() == [0, 1, 1, 1] and k.movable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError, match=r'movable must be bool \[4\]'):
        k.movable(np.zeros(3, bool))
    assert k.floor(None, 2).tolist() == [-np.inf] * 4 and k.floor(None, 2).dtype == torch.float32
    assert k.floor({'cue': 0.0, 'due': -np.inf}, 2).tolist() == [0.0, 0.0, -np.inf, -np.inf] and k.floor(-7.0, 2) is k.floor(-7.0, 2)
    for bad in (float('nan'), {'cue': 1.0}, [1.0, 2.0], torch.zeros(3)):
        with pytest.raises(ValueError, match='floor_sinr_db'):
            k.floor(bad, 2)
    assert k.words(None) is None and tuple(k.words(np.ones((4, 4), bool)).shape) == (4, 1)
    i32, f32, u8 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.uint8))
    good = (i32(3, 4), f32(3, 4), f32(3, 4), i32(3), i32(3), u8(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4)] * 3 + [(3,)] * 3
    assert [o.dtype for o in k.outputs(None)] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32, torch.uint8]
    planes = dict(pos_x=f32(3, 7), pos_y=f32(3, 7), rb=i32(3, 4), pwr=i32(3, 4))
    mov, floor = k.movable(None), k.floor(None, 2)
    before = _native.rbascent_launches
    shared = i32(3)
    for out in (good[:5], (*good[:3], shared, shared, good[5]), (*good[:5], i32(3)), (good[0], f32(3, 5), *good[2:]), good[0],
                (good[0], f32(3, 8)[:, ::2], *good[2:])):
        with pytest.raises(ValueError, match=r'out must be \(rb, sinr_db, capacity_mbps, rounds, moves, converged\)'):
            k.solve(planes, None, mov, floor, 0.0, 16, out, 0)
    for bad in (-0.5, float('nan'), float('inf'), -1, True, '1', None):
        with pytest.raises(ValueError, match='min_gain_mbps must be a finite number >= 0'):
            k.solve(planes, None, mov, floor, bad, 16, None, 0)
    for bad in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError, match=r'max_rounds must be an int in \[1, 4096\]'):
            k.solve(planes, None, mov, floor, 0.0, bad, None, 0)
    for bad in (np.ones((4, 5), bool), np.ones((4, 4), np.int32)):
        with pytest.raises(ValueError, match=r'allowed must be bool \[4, 4\]'):
            k.solve(planes, bad, mov, floor, 0.0, 16, None, 0)
    with pytest.raises(ValueError, match='env_mask must be'):
        k.solve(planes, None, mov, floor, 0.0, 16, None, 0, env_mask=np.ones(4, bool))
    assert _native.rbascent_launches == before
    # the shapes the object refuses when it is made, and the one only a mask pushes past the limit
    with pytest.raises(ValueError, match=r'rb_ascent\(\) serves at most 8192 RBs'):
        rb_ascent.RbAscent(_stub_sim(num_rbs=8193), 4, agent, torch, cpu)
    with pytest.raises(ValueError, match='the agent mask does not match the env'):
        rb_ascent.RbAscent(_stub_sim(), 4, agent[:3], torch, cpu)

    def wide(r):
        return SimpleNamespace(**{**vars(_stub_sim(num_rbs=r)), 'link_tx': np.ones(2048, dtype=np.int64), 'link_rx': np.zeros(2048, dtype=np.int64)})
    with pytest.raises(ValueError, match=rf'2048 links on 128 RBs need {_header_lds(2048, 128, True)} bytes, more than 163840'):
        rb_ascent.RbAscent(wide(128), 2048, np.ones(2048, bool), torch, cpu)
    k = rb_ascent.RbAscent(wide(127), 2048, np.ones(2048, bool), torch, cpu)
    with pytest.raises(ValueError, match=rf'need {_header_lds(2048, 127, True, True)} bytes with an allowed mask, more than 163840'):
        k.need(True)
    assert k.need(False) == _header_lds(2048, 127, True)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_rbascent_library', lambda: pytest.fail('libd2d_rbascent.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._rbascent is None
    for call in (lambda: env.rb_ascent(), lambda: env.rb_ascent(None, None, 0.0), lambda: env.rb_ascent_actions()):
        with pytest.raises(ValueError, match=r'rb_ascent\(\) needs the torch path'):
            call()
    assert env._rbascent is None
    assert 'power_ascent_actions()' in VecD2DEnv.rb_ascent_actions.__doc__      # it says what it composes with
    env.close()


def test_rb_ascent_actions_encode_the_solved_rbs_on_a_stubbed_handle(monkeypatch):
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
    env.rb_ascent = lambda *a: seen.append(a) or (torch.as_tensor(rb, dtype=torch.int32), None, None, None, None, None)
    a = env.rb_ascent_actions('mask', 'some', {'cue': 0.0, 'due': 5.0}, 0.05, 9)
    assert seen == [('mask', 'some', {'cue': 0.0, 'due': 5.0}, 0.05, 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()


# ------------------------------------------------------------------------------------------ the restatement's properties
@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False), ('n20_r64', False)])
def test_every_move_raises_the_envs_oracle_total_and_a_met_floor_is_kept(name, floors):
    case, b, every = ru.CASES[name]
    c = ru.make_case(case)
    ref = ru.reference(name, floors)
    assert len(ref.raised) == ref.moves.sum() > 0
    assert all(after > before for _, _, before, after in ref.raised)
    if floors:
        # float64 on both sides and the same oracle: a link that meets its floor at the start meets it at the end, exactly
        fl = ru.floor_vector(ru.FLOORS, c.cues, c.dues).astype(np.float64)
        for x in range(b):
            s0, s1 = (ru.oracle_planes(c, x, np.asarray(v[x])[None, :], c.pwr[x])[0][0] for v in (ref.start, ref.rb))
            met = s0 >= fl
            assert met.any() and (s1[met] >= fl[met]).all()


def _tiny(seed, n, r, rb):
    """A case of a few links on r RBs at rb [N]."""
    cues = 1
    dues = n - cues
    rng = np.random.default_rng(seed)
    from oracle import d2d_oracle as orc
    from sim_util import default_links, random_layout
    pos = random_layout(rng, 1, cues, dues, cell_radius=200.0)
    tx, rx, _ = default_links(cues, dues)
    p_min, p_max, _ = pcu.bounds(cues, dues)
    return SimpleNamespace(name=f'rbtiny{seed}_{n}_{r}', cues=cues, dues=dues, n=n, r=r, pos=pos, rb=np.asarray(rb)[None, :],
                           pwr=rng.integers(p_min, p_max + 1)[None, :], tx=tx, rx=rx, spec=orc.PathLossSpec('log_distance', 2.1, ple=2.0),
                           cols=orc.device_columns(*orc.device_configs(cues, dues)[1:]))


def test_a_link_alone_with_an_empty_alternative_never_moves():
    for seed in range(6):
        c = _tiny(seed, 4, 7, [0, 2, 3, 5])                             # every link alone; RBs 1, 4 and 6 empty
        ref = ru.rb_ascent_ref(c, [0], max_rounds=8)
        assert ref.moves[0] == 0 and ref.converged[0] and ref.rounds[0] == 0 and np.array_equal(ref.rb, c.rb)


def test_tiny_cases_end_at_or_below_the_brute_force_optimum_over_all_placements():
    strictly = 0
    for seed in range(8):
        n, r = (4, 3) if seed % 2 else (5, 2)
        c = _tiny(100 + seed, n, r, np.random.default_rng(seed).integers(0, r, n))
        ref = ru.rb_ascent_ref(c, [0], max_rounds=64)
        assert ref.converged[0]
        rows = np.array(list(itertools.product(range(r), repeat=n)))
        totals = ru.sequential_sum(ru.oracle_planes(c, 0, rows, c.pwr[0])[1], axis=1)
        got = totals[(rows == ref.rb[0][None, :]).all(axis=1)][0]
        start = totals[(rows == c.rb[0][None, :]).all(axis=1)][0]
        assert start <= got <= totals.max()
        # no single link gains by moving: a coordinate-wise optimum, up to the rounding of two different summation orders
        one_away = (rows != ref.rb[0][None, :]).sum(axis=1) == 1
        assert (totals[one_away] <= got * (1 + 1e-12)).all()
        strictly += got > start
    assert strictly >= 4


# ------------------------------------------------------------------------------------------ the GPU cases hold what they are there for
def test_n37_r5_floors_change_at_least_one_decision():
    ref = ru.reference('n37_r5', True)
    print(int(ref.floor_changed.sum()), 'of', len(ref.floor_changed))
    assert ref.floor_changed.any()
    assert not ru.reference('n37_r5').floor_changed.any()


def test_some_env_is_still_moving_at_two_rounds():
    ref = ru.reference('n37_r5', False, 2)
    print(ref.rounds.tolist(), ref.converged.astype(int).tolist())
    assert ((ref.rounds == 2) & ~ref.converged).any()
    assert (ru.reference('n37_r5').rounds > 2).any()                    # and it is the cap that stopped them


def test_n20_r300_has_empty_rbs_and_links_alone():
    c = ru.make_case('n20_r300')
    assert c.r == 300 and c.r > 256 and c.r % 32 == 12 and c.b == 8
    for e in range(c.b):
        g = np.bincount(c.rb[e], minlength=c.r)
        assert (g == 0).any() and (g == 1).any()
    g = np.bincount(ru.make_case('n96_r2').rb[0], minlength=2)
    assert g.min() >= 40                                                # groups near 48


@pytest.mark.parametrize('name,floors', [('n37_r5', False), ('n37_r5', True), ('n50_r6_hata', False)])
def test_the_reference_alone_stays_inside_the_cap_at_its_own_fixed_point(name, floors):
    """At the restatement's own fixed point the inequality holds with nothing to spare taken (worst <= 0 of the slack) and the share
    of (link, RB) checks left out for a SINR within W of a floor or a sensitivity is under the cap."""
    case, b, every = ru.CASES[name]
    c = ru.make_case(case)
    ref = ru.reference(name, floors)
    floor = ru.FLOORS if floors else None
    chk = ru.reference_check(c, np.arange(b), ref.rb, ref.converged, None, ru.movable_mask(c.n, every), floor, 0.0)
    print(f'{name} floors={floors}: {chk.checks} checks, {chk.left_out} left out, worst {chk.worst:.3e}')
    assert chk.checks > 1000 and chk.left_out <= ru.CAP * chk.checks
    assert chk.violations == [] and chk.worst <= 0.0

"""Max-min SINR balancing, the part that needs no GPU: the library's exported set and its place in the build, the entry point's
refusals, the LDS formula, the kernels' register report, the host module on a stub sim, and the float64 reference (balance_util):
its ambiguity cap on the GPU tests' cases and the linear scan of every level on the small ones."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import balance_util as bu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_balance.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_balance.hip'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


# ------------------------------------------------------------------------------------------ exports and tables
def test_balance_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_balance_library()
    assert _native.side_library('balance') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_balance.so') == declared == {'d2d_balance_sinr', 'd2d_balance_last_error'}
    assert set(_native.BALANCE_SIGNATURES) == declared and _native.FAMILIES['balance'] is _native.BALANCE_SIGNATURES
    assert len(_native.BALANCE_SIGNATURES['d2d_balance_sinr'][1]) == 28
    for symbol, (res, args) in _native.BALANCE_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(lib.d2d_balance_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MAX_LINKS', 'MAX_RBS', 'MAX_MARGINS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_BALANCE_%s (\d+)' % const, header).group(1)) == getattr(_native, 'BALANCE_' + const), const
    assert _native.BALANCE_MAX_LINKS == _native.MAX_LINKS and _native.BALANCE_MAX_LDS_BYTES == 160 * 1024 and _native.BALANCE_MAX_MARGINS == 4096
    # the law ids are power control's: sensing.fold_columns serves both
    assert (_native.BALANCE_LAW_INV_SQUARE, _native.BALANCE_LAW_POWER, _native.BALANCE_LAW_POW_K) == \
        (_native.POWERCTL_LAW_INV_SQUARE, _native.POWERCTL_LAW_POWER, _native.POWERCTL_LAW_POW_K)
    # the fourth table: present in the build, the digest and the headers
    assert build.FAMILIES == {'balance': ['d2d_balance.hip']} and set(build.FAMILIES) == set(_native.FAMILIES)
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert build.CSRC / 'd2d_powerctl_device.h' in build.HEADERS and build.CSRC / 'd2d_powerctl_device.h' in build.digest_files()
    assert build.lib_path('balance') == LIB_DIR / 'libd2d_balance.so' == _native.side_path('balance')
    assert list(build.TARGETS) == list(build.EVERYTHING) + ['balance']   # compiled and linked behind everything else
    # the four pinned tables as they were
    assert len(build.LIBRARIES) == 14 and len(_native.SIDE) == 12 and set(build.SOLVERS) == set(_native.SOLVERS) == {'assign'}
    assert list(build.ADDONS) == list(_native.ADDONS) == ['assignpwr', 'color']
    assert build.BUILT == {**build.LIBRARIES, **build.SOLVERS} and build.EVERYTHING == {**build.BUILT, **build.ADDONS}
    for table in (build.LIBRARIES, build.SOLVERS, build.ADDONS, build.BUILT, build.EVERYTHING, _native.SIDE, _native.SOLVERS, _native.ADDONS):
        assert 'balance' not in table
    text = Path(build.__file__).read_text()                            # ADDONS is no longer called the table that grows; FAMILIES is
    assert 'balance' in build.__doc__ and text.count('the one that grows') == 1
    assert text.index('ADDONS = {') < text.index('the one that grows') < text.index('FAMILIES = {')


def test_a_missing_balance_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.families_missing() == [] and build.families_missing(tmp_path) == ['balance']
    build.lib_path('balance', tmp_path).touch()
    assert build.families_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'families_missing', lambda lib_dir=build.LIB_DIR: ['balance'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built() and not build.addons_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_balance\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_balance_library()


# ------------------------------------------------------------------------------------------ the LDS formula
def _header_lds(n, r, power_law):
    """The formula as include/d2d_balance.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    n4 = (n + 3) // 4 * 4
    return 32 * n + (2 + int(power_law)) * r16(8 * n) + 28 * n4 + r16(4 * (r + 1)) + 64


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, balance
    header = HEADER.read_text()
    assert '32 n_links + (2 + has_power_law) round16(8 n_links) + 28 n4 + round16(4 (n_rbs + 1)) + 64' in header
    for n, r in ((1, 1), (2, 3), (37, 5), (50, 6), (300, 7), (1000, 64), (2048, 256), (2048, 8192)):
        for law in (_native.BALANCE_LAW_INV_SQUARE, _native.BALANCE_LAW_POWER, _native.BALANCE_LAW_POW_K):
            assert balance.lds_bytes(n, r, law) == _header_lds(n, r, law != _native.BALANCE_LAW_INV_SQUARE), (n, r, law)
    assert _header_lds(1, 1, False) == 32 + 32 + 28 * 4 + 16 + 64
    assert _header_lds(2048, 256, False) == 2048 * 76 + 1040 + 64 and _header_lds(1000, 64, True) == 1000 * 84 + 272 + 64
    # the GPU cases past the 64 KiB branch, and the two shapes on either side of the limit
    assert _header_lds(1000, 64, True) > 64 * 1024 and _header_lds(2048, 256, False) > 64 * 1024 > _header_lds(300, 7, False)
    assert _header_lds(2048, 2031, False) == _native.BALANCE_MAX_LDS_BYTES < _header_lds(2048, 2032, False)
    assert _header_lds(1948, 35, True) <= _native.BALANCE_MAX_LDS_BYTES < _header_lds(1949, 35, True)


# ------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, n_margins=4, max_iters=4)

    def call(ptr=8, base=8, floor=0, margins=8, lo=8, hi=8, adj=0, mask=0, out=(8, 16, 24, 32, 40), **kw):
        a = dict(ok, **kw)
        _native.balance_sinr(ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                             base, floor, margins, a['n_margins'], lo, hi, adj, a['max_iters'], mask, *out)
    before = _native.balance_launches
    big = _header_lds(2048, 2032, False)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.BALANCE_MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.BALANCE_MAX_RBS + 1), 'n_rbs'), (dict(n_envs=-1), 'n_envs'), (dict(n_envs=2 ** 31), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(n_margins=0), r'n_margins must be in \[1, 4096\]'), (dict(n_margins=4097), 'n_margins'),
                     (dict(n_margins=-1), 'n_margins'), (dict(max_iters=0), 'max_iters'), (dict(max_iters=-3), 'max_iters'),
                     (dict(law=3), 'unknown law'), (dict(law=-1), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(ptr=0), 'null device pointer'), (dict(base=0), 'null device pointer'), (dict(margins=0), 'null device pointer'),
                     (dict(lo=0), 'null device pointer'), (dict(hi=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 8 * (i + 1) for i in range(5))), 'null device pointer') for z in range(5)),
                     (dict(out=(8, 8, 24, 32, 40)), 'power_dbm, sinr_db, margin_db, level and probes must be five arrays'),
                     (dict(out=(8, 16, 24, 32, 24)), 'must be five arrays'), (dict(out=(8, 16, 24, 40, 40)), 'must be five arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=2032), rf'n_links and n_rbs need {big} bytes of LDS, more than the 163840 \(D2D_BALANCE_MAX_LDS_BYTES\)'),
                     (dict(n_links=1949, n_rbs=35, law=1), 'bytes of LDS'), (dict(n_links=2048, n_rbs=2032, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(floor=8, adj=8, mask=8), dict(n_links=2048, n_rbs=2031), dict(n_links=1948, n_rbs=35, law=2, pow_k=4),
               dict(n_margins=1), dict(n_margins=4096)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.balance_launches == before


# ------------------------------------------------------------------------------------------ the kernels' budget
@pytest.fixture(scope='module')
def balance_asm(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_balance')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'balance.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return next(tmp.glob('*gfx950*.s')).read_text()


def test_register_report_shows_no_scratch_no_spills_and_no_static_lds(balance_asm):
    """law in {inverse square 0, power 1, pow-k 4}, read from the metadata as test_power_control_cpu.py reads it.  The figures of
    the build this was written on: 52, 54 and 56 VGPRs (two more than powerctl_kernel each), no AGPRs; LDS is dynamic."""
    found = {}
    for blk in re.split(r'\n  - ', balance_asm[balance_asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'balance_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        found[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                        'private_segment_fixed_size', 'group_segment_fixed_size', 'max_flat_workgroup_size')}
    assert set(found) == {0, 1, 4}
    for key, k in found.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0 and k['max_flat_workgroup_size'] == 256, (key, k)
    assert 'scratch_' not in balance_asm
    # no atomics of any kind, in the ISA and in the source
    assert not re.search(r'^\s*(global|flat|buffer|ds)_\w*(atomic|_rtn_|cmpst|_add_u32|_max_|_min_|_or_b32)', balance_asm, flags=re.M)
    code = SOURCE.read_text().split('#include', 1)[1]
    assert 'atomic' not in code.replace('no atomics', '')


def test_the_only_global_reads_of_the_loops_are_the_margins(balance_asm):
    """The source between the start of the search and the results names global memory - the argument struct's pointers - only as
    a.margins[mid]: no other a.<pointer> is read or written inside the probe and sweep loops."""
    src = SOURCE.read_text()
    loops = src[src.index('// ---- the search'):src.index('// ---- the SINR at the kept powers')]
    pointers = re.findall(r'^\s+(?:const )?(?:unsigned char|float|int)\*\s+(\w+);', src[src.index('struct BalanceArgs'):src.index('int D, N, R, K;')], flags=re.M)
    assert len(pointers) == 19
    used = set(re.findall(r'\ba\.(\w+)', loops))
    assert used & set(pointers) == {'margins'} and used <= {'margins', 'max_iters', 'pow_k', 'K'}


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


def test_refusal_texts_name_balance_sinr_and_the_other_rows_are_unchanged():
    from gym_d2d_amd import balance, power_control, sensing
    assert balance.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: balance.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = balance.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('balance_sinr() ') and 'power_control()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where power_control() is
        assert power_control.refusal(*args) is not None
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11
    assert sensing.REFUSALS['power_control'][0] == 'power_control()' and sensing.REFUSALS['assign_rbs_power'][0] == 'assign_rbs_power()'


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import _native, balance, sensing
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    lo, hi = np.zeros(4, dtype=np.int32), np.array([23, 23, 20, 20], dtype=np.int32)
    cpu = torch.device('cpu')
    k = balance.SinrBalance(_stub_sim(), 4, lo, hi, agent, torch, cpu)
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4) and k.law == _native.BALANCE_LAW_POW_K
    assert k.adjustable(None).tolist() == [0, 1, 1, 1] and k.adjustable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError, match=r'adjustable must be bool \[4\]'):
        k.adjustable(np.zeros(3, bool))
    # base and floor: power_control.link_values under names of their own, each with its own cache
    assert k.base(3.0, 2).tolist() == [3.0] * 4 and k.base(3.0, 2).dtype == torch.float32
    assert k.floor(None, 2) is None and k.floor({'cue': -5.0, 'due': -np.inf}, 2).tolist() == [-5.0, -5.0, -np.inf, -np.inf]
    same_base, same_floor = k.base([1.0, 2.0, 3.0, 4.0], 2), k.floor(-7.0, 2)
    assert k.base(np.array([1.0, 2.0, 3.0, 4.0]), 2) is same_base and k.floor(-7.0, 2) is same_floor       # neither evicts the other
    for bad in (float('nan'), {'cue': 1.0}, [1.0, 2.0], torch.zeros(3)):
        with pytest.raises(ValueError, match='base_sinr_db'):
            k.base(bad, 2)
        with pytest.raises(ValueError, match='floor_sinr_db'):
            k.floor(bad, 2)
    # margins_db: the default grid, host values checked here, tensors by dtype, shape and device
    assert k.margins(None).tolist() == [float(x) for x in range(-20, 41)] and k.margins(None) is k.margins(None)
    assert k.margins([0.0]).tolist() == [0.0] and k.margins((-1, 0.5, 7)).dtype == torch.float32
    assert k.margins(np.arange(4096)).shape == (4096,)
    t = torch.tensor([3.0, 1.0])                                        # a tensor's order is the caller's promise
    assert k.margins(t) is t
    for bad in ([], 3.0, [[0.0, 1.0]], [0.0, 0.0], [1.0, 0.0], [0.0, np.inf], [0.0, np.nan], np.arange(4097), 'grid',
                [16777216.0, 16777217.0]):                               # ascending as float64, equal as float32
        with pytest.raises(ValueError, match='margins_db must be 1 to 4096 finite values in strictly ascending order'):
            k.margins(bad)
    for bad in (torch.zeros(3, dtype=torch.float64), torch.zeros((2, 2)), torch.zeros(0), torch.zeros(4097), torch.zeros(3, device='meta')):
        with pytest.raises(ValueError, match=r'margins_db as a tensor must be float32 \[K\]'):
            k.margins(bad)
    # out= and max_iters, refused before the library is touched
    i32, f32 = (lambda *s: torch.zeros(*s, dtype=torch.int32)), (lambda *s: torch.zeros(*s))
    good = (i32(3, 4), f32(3, 4), f32(3), i32(3), i32(3))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    assert [tuple(o.shape) for o in k.outputs(None)] == [(3, 4), (3, 4), (3,), (3,), (3,)]
    assert [o.dtype for o in k.outputs(None)] == [torch.int32, torch.float32, torch.float32, torch.int32, torch.int32]
    shared = i32(3)
    planes = dict(pos_x=f32(3, 7), pos_y=f32(3, 7), rb=i32(3, 4), pwr=i32(3, 4))
    before = _native.balance_launches
    for out in (good[:4], (good[0], good[1], good[2], shared, shared), (good[0], good[1], i32(3), good[3], good[4]),
                (good[0], f32(3, 5), good[2], good[3], good[4]), good[0], (good[0], f32(3, 8)[:, ::2], good[2], good[3], good[4])):
        with pytest.raises(ValueError, match=r'out must be \(power_dbm, sinr_db, margin_db, level, probes\)'):
            k.solve(planes, k.base(0.0, 2), k.margins(None), None, k.adjustable(None), 64, out, 0)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='max_iters must be an int >= 1'):
            k.solve(planes, k.base(0.0, 2), k.margins(None), None, k.adjustable(None), bad, None, 0)
    with pytest.raises(ValueError, match='env_mask must be'):
        k.solve(planes, k.base(0.0, 2), k.margins(None), None, k.adjustable(None), 64, None, 0, env_mask=np.ones(4, bool))
    assert _native.balance_launches == before
    with pytest.raises(ValueError, match=r'balance_sinr\(\) serves at most 8192 RBs'):
        balance.SinrBalance(_stub_sim(num_rbs=8193), 4, lo, hi, agent, torch, cpu)
    with pytest.raises(ValueError, match='the power bounds do not match the env'):
        balance.SinrBalance(_stub_sim(), 4, lo, hi[:3], agent, torch, cpu)
    # past the LDS of a workgroup: refused by name with the bytes, when the kernel object is made
    wide = SimpleNamespace(**{**vars(_stub_sim(num_rbs=64)), 'link_tx': np.ones(2048, dtype=np.int64), 'link_rx': np.zeros(2048, dtype=np.int64)})
    with pytest.raises(ValueError, match=rf'2048 links on 64 RBs need {_header_lds(2048, 64, True)} bytes, more than 163840'):
        balance.SinrBalance(wide, 2048, np.zeros(2048, np.int32), np.full(2048, 20, np.int32), np.ones(2048, bool), torch, cpu)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_balance_library', lambda: pytest.fail('libd2d_balance.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._balance is None
    for call in (lambda: env.balance_sinr(), lambda: env.balance_sinr(3.0, [0.0, 1.0]), lambda: env.balance_sinr_actions()):
        with pytest.raises(ValueError, match=r'balance_sinr\(\) needs the torch path'):
            call()
    assert env._balance is None
    env.close()


def test_balance_sinr_actions_encode_the_balanced_powers_on_a_stubbed_handle(monkeypatch):
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
    env.balance_sinr = lambda *a: seen.append(a) or (torch.as_tensor(power, dtype=torch.int32), None, None, None, None)
    a = env.balance_sinr_actions(2.0, [0.0, 1.0], {'cue': -5.0, 'due': -np.inf}, 'mask', 9)
    assert seen == [(2.0, [0.0, 1.0], {'cue': -5.0, 'due': -np.inf}, 'mask', 9)]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()


# ------------------------------------------------------------------------------------------ the float64 reference
def test_the_reference_on_a_link_alone_finds_the_last_level_its_maximum_reaches():
    """One CUE alone on its RB: level k is reachable iff snr at p_max >= margins[k], so the search must end on the last such level,
    at the least power that gives it, after probe 0 and the halvings of the fixed rule."""
    c, base, margins, floor, adj = bu.row('n1')
    ref = bu.reference('n1')
    from oracle import d2d_oracle as orc
    snr_max = orc.step(c.pos, c.tx, c.rx, c.rb, np.broadcast_to(c.p_max[None], (c.b, 1)), c.cols, c.spec)['snr_db'][:, 0]
    want = np.searchsorted(margins.astype(np.float64), snr_max, side='right') - 1
    clear = np.abs(snr_max - margins.astype(np.float64)[want]) > bu.W
    assert clear.sum() >= 48 and not ref.ambiguous[clear].any()
    assert np.array_equal(ref.level[clear], want[clear])
    assert np.array_equal(ref.margin_db, margins[ref.level].astype(np.float64))
    assert (ref.sinr_db[clear, 0] >= ref.margin_db[clear] - 1e-9).all() and (ref.sinr_db[clear, 0] < ref.margin_db[clear] + 1.0 + 1e-9).all()
    # the count of probes is the rule's: 1, then the halvings of [0, K)
    for e in range(c.b):
        lo, hi, count = 0, len(margins), 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if mid <= ref.level[e] else (lo, mid)
            count += 1
        assert count == ref.probes[e] and lo == ref.level[e]


@pytest.mark.parametrize('name', list(bu.TABLE))
def test_reference_ambiguity_of_the_gpu_cases_stays_inside_the_cap(name):
    """The rows the GPU test compares with balance_ref, on the reference alone: at most 25 % of a row's envs are ambiguous, and the
    rows exercise what they are there for."""
    c, base, margins, floor, adj = bu.row(name)
    ref = bu.reference(name)
    k_all = len(margins)
    share = float(ref.ambiguous.mean())
    infeasible, top = int((ref.level < 0).sum()), int((ref.level == k_all - 1).sum())
    print(f'{name}: K = {k_all}, {int(ref.ambiguous.sum())}/{c.b} envs ambiguous, {infeasible} infeasible, {top} end at K - 1, levels '
          f'{ref.level[ref.level >= 0].min()}..{ref.level.max()}, probes {ref.probes.min()}..{ref.probes.max()}')
    assert ref.ambiguous.shape == (c.b,) and share <= bu.CAP and (~ref.ambiguous).sum() >= 3
    assert (ref.probes[ref.level < 0] == 1).all() and np.isneginf(ref.margin_db[ref.level < 0]).all()
    assert (ref.probes <= 1 + int(np.ceil(np.log2(k_all)))).all() and (ref.level < k_all).all()
    assert (ref.power_dbm >= c.p_min[None]).all() and (ref.power_dbm <= c.p_max[None]).all() or name.endswith('no_rb')
    if floor is not None:                                               # both outcomes of the floor, and no floor is broken
        assert 0 < infeasible < c.b
        ok = ref.level >= 0
        assert (ref.sinr_db[ok][:, :c.cues] >= floor[None, :c.cues]).all()
        assert np.array_equal(ref.power_dbm[:, :c.cues], c.pwr[:, :c.cues])                 # the protected links never move
    else:
        assert infeasible == 0
    if name.endswith('_top'):
        assert top > 0
    else:
        assert top == 0 and len(np.unique(ref.level)) >= 3             # an interior answer that differs between envs
    if name.endswith('no_rb'):
        assert (~ref.on_rb).sum() == c.b and np.isnan(ref.sinr_db[~ref.on_rb]).all()


@pytest.mark.parametrize('name', list(bu.EXACT_ONLY))
def test_the_two_rows_past_the_cap_are_the_ones_left_to_the_exact_yardstick(name):
    ref = bu.reference(name)
    print(f'{name}: {int(ref.ambiguous.sum())}/{len(ref.ambiguous)} envs ambiguous')
    assert ref.ambiguous.mean() > bu.CAP


@pytest.mark.parametrize('name', bu.SCANNED)
def test_linear_scan_is_monotone_and_ends_where_the_bisection_does(name):
    """Every level probed one by one: on the envs balance_ref does not call ambiguous the passes are a prefix of the grid, and the
    bisection's level is the last of them (-1: none).  (Both are properties of the float64 run itself; the count over all envs is
    printed.)"""
    c, base, margins, floor, adj = bu.row(name)
    ref = bu.reference(name)
    passes, amb = bu.scan_ref(c, base, margins, floor, adj)
    ok = ~ref.ambiguous
    assert (ref.ambiguous <= amb.any(axis=0)).all()                     # the scan ran every probe the bisection ran
    count = passes.sum(axis=0)
    prefix = (passes == (np.arange(len(margins))[:, None] < count[None, :])).all(axis=0)
    agree = prefix & (ref.level == count - 1)
    print(f'{name}: {int(ok.sum())}/{c.b} envs unambiguous; passes per env {count.min()}..{count.max()} of {len(margins)} levels; monotone '
          f'and equal to the bisection in {int(agree.sum())}/{c.b} envs')
    assert prefix[ok].all()
    assert np.array_equal(ref.level[ok], count[ok] - 1)

"""Stable RB matching, the part that needs no GPU: the two NumPy restatements against each other and against brute force
(stable_util), the library's exported set and its place in the build, the LDS formula, the entry point's refusals, the host class
on a stub sim, and the kernel's register report."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import stable_util as su

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_stable.h'
SOURCE = ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_stable.hip'


# ------------------------------------------------------------------------------------------ the restatements
def _instances():
    """Random instances with heavy ties and holes: M above, at and below the total quota, quotas 0 to 3."""
    rng = np.random.default_rng(7)
    for i in range(120):
        m, r = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        quota = rng.integers(0, 4, r)
        if i % 3 == 0 and quota.sum() > 0:
            m = int(quota.sum())                                        # exactly as many links as places
        elif i % 3 == 1:
            m = int(quota.sum()) + int(rng.integers(1, 4))              # more links than places
        lp, rp = su.random_instance(rng, m, r, alphabet=su.ALPHABET if i % 2 == 0 else None)
        yield lp, rp, quota


def test_the_two_restatements_agree_exactly_and_leave_no_blocking_pair():
    seen = {'over': 0, 'at': 0, 'under': 0, 'closed': 0, 'unmatched': 0, 'kinds': set()}
    for lp, rp, quota in _instances():
        a, b = su.sequential(lp, rp, quota), su.rounds(lp, rp, quota)
        assert np.array_equal(a.col, b.col) and np.array_equal(a.load, b.load), (lp, rp, quota)
        assert a.proposals == b.proposals and a.unmatched == b.unmatched == int((a.col < 0).sum()), (lp, rp, quota)
        assert su.feasible(lp, rp, quota, a.col) and su.blocking_pairs(lp, rp, quota, a.col) == [], (lp, rp, quota)
        m = lp.shape[0]
        seen['over' if m > quota.sum() else 'at' if m == quota.sum() else 'under'] += 1
        seen['closed'] += int((quota == 0).any())
        seen['unmatched'] += int(a.unmatched > 0)
        for x in (lp, rp):
            seen['kinds'] |= {k for k, f in (('nan', np.isnan), ('+inf', np.isposinf), ('-inf', np.isneginf)) if f(x).any()}
    assert min(seen['over'], seen['at'], seen['under'], seen['closed'], seen['unmatched']) >= 10, seen
    assert seen['kinds'] == {'nan', '+inf', '-inf'}


def test_the_two_zeros_tie_and_the_index_decides():
    """Both links like both RBs 'equally' in zeros of either sign, and so do the RBs: link 0 takes RB 0, link 1 RB 1."""
    lp = np.array([[-0.0, 0.0], [0.0, -0.0]], dtype=np.float32)
    rp = np.array([[0.0, -0.0], [-0.0, 0.0]], dtype=np.float32)
    for how in (su.sequential, su.rounds):
        res = how(lp, rp, 1)
        assert res.col.tolist() == [0, 1] and res.proposals == 3 and res.unmatched == 0
    # a bit-pattern order would have ranked +0.0 above -0.0: link 0 would take RB 1
    assert su.sequential(lp, rp, [0, 2]).col.tolist() == [1, 1] and su.sequential(lp, rp, [0, 2]).proposals == 4


def test_blocking_pair_finder_finds_them():
    lp = np.array([[2.0, 1.0], [2.0, 1.0]], dtype=np.float32)
    rp = np.array([[1.0, 1.0], [2.0, 2.0]], dtype=np.float32)          # both RBs prefer link 1
    assert su.sequential(lp, rp, 1).col.tolist() == [1, 0]
    assert su.blocking_pairs(lp, rp, 1, np.array([0, 1])) == [(1, 0)]   # link 1 and RB 0 would rather be together
    assert su.blocking_pairs(lp, rp, 1, np.array([-1, 0])) == [(0, 1)]  # RB 1 is under quota
    assert su.blocking_pairs(lp, rp, [1, 0], np.array([-1, 0])) == []   # a closed RB blocks nothing
    assert not su.feasible(lp, rp, 1, np.array([0, 0]))


def test_tiny_instances_are_link_optimal_and_every_stable_matching_leaves_the_same_links_out():
    rng = np.random.default_rng(11)
    several = 0
    for i in range(150):
        if i % 2:                                                       # strict orders, full lists, the two sides wanting the opposite:
            m, r = int(rng.integers(3, 5)), 3                           # where several stable matchings live
            quota = rng.integers(1, 3, r)
            lp = rng.normal(size=(m, r)).astype(np.float32)
            rp = (-lp + 0.3 * rng.normal(size=(m, r))).astype(np.float32)
        else:
            m, r = int(rng.integers(1, 5)), int(rng.integers(1, 4))
            quota = rng.integers(0, 3, r)
            lp, rp = su.random_instance(rng, m, r, alphabet=None if i % 4 else su.ALPHABET, holes=0.1)
        got = su.sequential(lp, rp, quota)
        stable = su.all_stable_matchings(lp, rp, quota)
        assert any(np.array_equal(got.col, s) for s in stable), (lp, rp, quota)
        several += len(stable) > 1
        for s in stable:
            assert np.array_equal(s < 0, got.col < 0), (lp, rp, quota)                      # the rural-hospitals theorem
            assert all(su.link_weakly_prefers(lp, a, got.col[a], s[a]) for a in range(m)), (lp, rp, quota)
    assert several >= 10                                                 # link-optimality was a choice among several


def test_proposals_is_the_count_the_sequential_run_makes_and_the_position_sum():
    rng = np.random.default_rng(5)
    for _ in range(40):
        lp, rp = su.random_instance(rng, 7, 4)
        quota = rng.integers(0, 3, 4)
        a, b = su.sequential(lp, rp, quota), su.rounds(lp, rp, quota)   # a counts as it goes, b sums positions in the result
        assert a.proposals == b.proposals
    lp, rp, quota = su.case('rejection_chain')
    res = su.sequential(lp[0], rp[0], quota)
    assert res.proposals == 8256 == 128 * 129 // 2 and res.col.tolist() == list(range(128))
    lp, rp, quota = su.case('pure_index_order')
    assert su.sequential(lp[1], rp[1], quota).col.tolist() == [a // 2 for a in range(50)]
    assert np.signbit(lp).any() and not np.signbit(lp).all() and (lp == 0).all() and (rp == 0).all()


@pytest.mark.parametrize('name', [n for n, row in su.CASES.items() if row[4] == 'random'])
def test_the_gpu_cases_hold_what_they_are_there_for(name):
    b, m, r, _, _ = su.CASES[name]
    lp, rp, quota = su.case(name)
    assert lp.shape == rp.shape == (b, m, r) and lp.dtype == rp.dtype == np.float32 and quota.shape == (r,)
    assert np.array_equal(su.case(name)[0], lp, equal_nan=True)         # the same arrays on every call
    ok = su.acceptable(lp, rp)
    assert not ok[0, m // 2].any()                                      # a wholly unacceptable row
    assert not np.isfinite(lp).all() and not np.isfinite(rp).all()
    live = ok.reshape(b, -1).any(axis=1)
    assert live.any() and (b == 1 or (not live[b - 1] and np.isfinite(lp[b - 1]).any()))


# ------------------------------------------------------------------------------------------ exports and tables
def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_stable_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_stable_library()
    assert _native.side_library('stable') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_stable.so') == declared == {'d2d_stable_match', 'd2d_stable_last_error'}
    assert set(_native.STABLE_SIGNATURES) == declared and _native.EXTRAS['stable'] is _native.STABLE_SIGNATURES
    assert len(_native.STABLE_SIGNATURES['d2d_stable_match'][1]) == 11
    for symbol, (res, args) in _native.STABLE_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(lib.d2d_stable_last_error(), bytes)
    for const in ('MAX_LINKS', 'MAX_RBS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_STABLE_%s (\d+)' % const, header).group(1)) == getattr(_native, 'STABLE_' + const), const
    assert _native.STABLE_MAX_LINKS == _native.MAX_LINKS and _native.STABLE_MAX_LDS_BYTES == 160 * 1024
    source = SOURCE.read_text()
    assert 'static_assert(D2D_STABLE_MAX_LINKS == d2d::SAME_RB_MAX_LINKS && D2D_STABLE_MAX_RBS == d2d::SAME_RB_MAX_RBS' in source
    # the fifth table: present in the build, the digest and the headers, compiled and linked behind everything else
    assert build.EXTRAS == {'stable': ['d2d_stable.hip']} and set(build.EXTRAS) == set(_native.EXTRAS)
    assert build.ALL == {**build.TARGETS, **build.EXTRAS} and list(build.ALL) == list(build.TARGETS) + ['stable']
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and SOURCE in build.digest_files()
    assert build.CSRC / 'd2d_wave_key.h' in build.HEADERS and build.CSRC / 'd2d_wave_key.h' in build.digest_files()
    assert len(set(build.digest_files())) == len(build.digest_files())
    assert build.lib_path('stable') == LIB_DIR / 'libd2d_stable.so' == _native.side_path('stable')
    assert 'stable' in build.__doc__ and 'EXTRAS' in build.__doc__
    # the pinned tables as they were
    assert build.FAMILIES == {'balance': ['d2d_balance.hip']} and list(_native.FAMILIES) == ['balance']
    assert list(build.TARGETS) == list(build.EVERYTHING) + ['balance']
    assert len(build.LIBRARIES) == 14 and len(_native.SIDE) == 12 and set(build.SOLVERS) == set(_native.SOLVERS) == {'assign'}
    assert list(build.ADDONS) == list(_native.ADDONS) == ['assignpwr', 'color']
    for table in (build.LIBRARIES, build.SOLVERS, build.ADDONS, build.BUILT, build.EVERYTHING, build.FAMILIES, build.TARGETS,
                  _native.SIDE, _native.SOLVERS, _native.ADDONS, _native.FAMILIES):
        assert 'stable' not in table


def test_a_missing_stable_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.extras_missing() == [] and build.extras_missing(tmp_path) == ['stable']
    build.lib_path('stable', tmp_path).touch()
    assert build.extras_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'extras_missing', lambda lib_dir=build.LIB_DIR: ['stable'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built() and not build.addons_missing() \
        and not build.families_missing()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_stable\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_stable_library()


# ------------------------------------------------------------------------------------------ the LDS formula
def _header_lds(m, r):
    """The formula as include/d2d_stable.h words it."""
    r16 = lambda x: (x + 15) // 16 * 16
    return 2 * r16(8 * m) + 4 * r16(4 * m) + 4 * r16(4 * r) + 16


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, stable_matching
    assert '2 round16(8 n_links) + 4 round16(4 n_links) + 4 round16(4 n_rbs) + 16' in HEADER.read_text()
    for m, r in ((1, 1), (5, 3), (65, 63), (257, 100), (300, 7), (40, 4101), (2048, 256), (2048, 8192), (256, 8192)):
        assert stable_matching.lds_bytes(m, r) == _header_lds(m, r), (m, r)
    assert _header_lds(1, 1) == 32 + 64 + 64 + 16 and _header_lds(2048, 256) == 2048 * 32 + 256 * 16 + 16
    assert _header_lds(2048, 256) > 64 * 1024 > _header_lds(257, 100)   # the GPU case past the 64 KiB branch
    # the shapes on either side of the limit
    assert _header_lds(2048, 6140) <= _native.STABLE_MAX_LDS_BYTES < _header_lds(2048, 6141)
    assert _header_lds(1022, 8192) <= _native.STABLE_MAX_LDS_BYTES < _header_lds(1023, 8192)


# ------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(n_envs=2, n_links=5, n_rbs=3)

    def call(lp=8, rp=16, quota=24, out=(32, 40, 48, 56), **kw):
        a = dict(ok, **kw)
        _native.stable_match(lp, rp, quota, a['n_envs'], a['n_links'], a['n_rbs'], *out)
    before = _native.stable_launches
    big = 6141                                                          # the first R that 2048 links do not fit with
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.STABLE_MAX_LINKS + 1), r'n_links must be in \[1, 2048\]'),
                     (dict(n_rbs=0), 'n_rbs'), (dict(n_rbs=_native.STABLE_MAX_RBS + 1), r'n_rbs must be in \[1, 8192\]'),
                     (dict(n_envs=-1), 'n_envs'), (dict(n_envs=2 ** 31), 'n_envs'),
                     (dict(lp=0), 'null device pointer'), (dict(rp=0), 'null device pointer'), (dict(quota=0), 'null device pointer'),
                     *((dict(out=tuple(0 if i == z else 32 + 8 * i for i in range(4))), 'null device pointer') for z in range(4)),
                     (dict(out=(32, 32, 48, 56)), 'col, load, proposals and unmatched must be four arrays'),
                     (dict(out=(32, 40, 48, 48)), 'must be four arrays'), (dict(out=(32, 40, 32, 56)), 'must be four arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=big),
                      rf'n_links and n_rbs need {_header_lds(2048, big)} bytes of LDS, more than the 163840 \(D2D_STABLE_MAX_LDS_BYTES\)'),
                     (dict(n_links=2048, n_rbs=8192), 'bytes of LDS'), (dict(n_links=2048, n_rbs=big, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(n_links=2048, n_rbs=big - 1), dict(n_links=1, n_rbs=8192), dict(n_links=1, n_rbs=1)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.stable_launches == before


# ------------------------------------------------------------------------------------------ the kernel's budget
def test_register_report_shows_no_scratch_no_spills_and_integer_lds_atomics_only(tmp_path):
    """Read from the metadata as test_balance_cpu.py reads it.  The figures of the build this was written on: 60 VGPRs, no AGPRs;
    LDS is dynamic."""
    from gym_d2d_amd import build
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(SOURCE), '-save-temps', '-o', 'stable.o']
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp_path.glob('*gfx950*.s')).read_text()
    blocks = [blk for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]) if re.search(r'\.name:\s+\S*stable_kernel', blk)]
    assert len(blocks) == 1
    field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blocks[0]).group(1))
    k = {name: field(name) for name in ('vgpr_count', 'agpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                        'private_segment_fixed_size', 'group_segment_fixed_size', 'max_flat_workgroup_size')}
    print(k)
    assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, k
    assert k['group_segment_fixed_size'] == 0 and k['max_flat_workgroup_size'] == 256 and k['vgpr_count'] <= 64, k
    assert 'scratch_' not in asm
    # no global, flat or buffer atomics; the LDS atomics are the integer exchange and add of the lists; no float atomics
    assert not re.search(r'^\s*(global|flat|buffer)_\w*atomic', asm, flags=re.M)
    ds_atomics = set(re.findall(r'^\s*(ds_(?:\w*rtn\w*|add_\w+|sub_\w+|min_\w+|max_\w+|and_\w+|or_\w+|xor_\w+|cmpst_\w+|inc_\w+|dec_\w+|pk_add\w+))\s',
                                asm, flags=re.M))
    print(sorted(ds_atomics))
    assert ds_atomics and all(re.fullmatch(r'ds_(wrxchg_rtn_b32|add_rtn_u32|add_u32)', name) for name in ds_atomics), ds_atomics
    code = SOURCE.read_text().split('#include', 1)[1]
    assert set(re.findall(r'\batomic\w+', code)) == {'atomicExch', 'atomicAdd'}


def test_the_rounds_read_their_decision_from_lds_and_write_no_global_memory():
    """Between the start of the rounds and the results the source names the argument struct only for the list stride: the
    preference pointers were offset before the loop and are only read; there is no iteration cap."""
    src = SOURCE.read_text()
    loop = src[src.index('// ---- the rounds'):src.index('// ---- the results')]
    assert set(re.findall(r'\ba\.(\w+)', loop)) == {'list_stride'}
    assert 'for (int p = 0;; p ^= 1)' in loop and 'const int n = s.misc[p];' in loop and 'if (n == 0) break;' in loop
    assert loop.count('__syncthreads()') == 2 and loop.count('break') == 1


# ------------------------------------------------------------------------------------------ the host class on a stub sim
def _stub_sim(route=None, shadowing=False, num_rbs=4):
    from gym_d2d_amd.path_loss_table import NATIVE
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    law = {'a_tx_db': [30.0] * 7, 'a_rx_db': [0.0] * 7, 'exponent': [3.5] * 7, 'shadowing': shadowing}
    return SimpleNamespace(num_envs=3, handle=SimpleNamespace(num_devices=7), config=SimpleNamespace(num_rbs=num_rbs),
                           link_tx=np.asarray([1, 2, 3, 5]), link_rx=np.asarray([0, 0, 4, 6]), _dev_list=[dev] * 7,
                           path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law=law),
                           fixed_positions=lambda: (np.zeros(7, bool), np.zeros((7, 2))))


def test_refusal_texts_name_stable_rbs_and_the_pinned_rows_are_unchanged():
    from gym_d2d_amd import assignment, sensing, stable_matching
    assert stable_matching.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: stable_matching.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = stable_matching.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('stable_rbs() ') and 'assign_rbs()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where assign_rbs() is, in its words
        assert assignment.refusal(*args).replace('assign_rbs()', 'stable_rbs()') == texts[needle]
    assert stable_matching.REFUSAL == ('stable_rbs()', *sensing.REFUSALS['assign_rbs'][1:])
    assert list(sensing.REFUSALS)[-1] == 'balance_sinr' and len(sensing.REFUSALS) == 11
    # refusal_text takes a key or a row
    assert sensing.refusal_text('assign_rbs', *stubs["'channel'"]) == sensing.refusal_text(sensing.REFUSALS['assign_rbs'], *stubs["'channel'"])


def test_the_host_class_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import _native, assignment, stable_matching
    cpu = torch.device('cpu')
    sim = _stub_sim()
    agent = np.array([False, True, True, True])
    assign = assignment.Assignment(sim, 4, agent, agent, torch, cpu)
    k = stable_matching.StableMatching(sim, 4, assign, torch, cpu)
    assert k.assign is assign
    with pytest.raises(ValueError, match='does not match the env'):
        stable_matching.StableMatching(_stub_sim(), 4, assign, torch, cpu)
    # quota: an int, [R] ints, or an int32 tensor
    assert k.quota(1, 3, 4).tolist() == [1, 1, 1, 1] and k.quota(1, 3, 4).dtype == torch.int32
    assert k.quota(1, 3, 4) is k.quota(np.int64(1), 3, 4) is k.quota([1, 1, 1, 1], 3, 4)         # a repeat is not uploaded again
    assert k.quota([3, 0, 1, 2], 3, 4).tolist() == [3, 0, 1, 2] and k.quota(np.array([0, 0, 0, 0]), 3, 4).tolist() == [0] * 4
    t = torch.tensor([5, -1, 0, 2], dtype=torch.int32)                  # a tensor's values are the caller's promise
    assert k.quota(t, 3, 4) is t
    for bad in (-1, 4, True, 1.0, [1, 1, 1], [1, 1, 1, 4], [1, 1, 1, -1], [1.0, 1.0, 1.0, 1.0], np.ones(4, bool), 'one', None, [[1, 1, 1, 1]]):
        with pytest.raises(ValueError, match=r'quota must be an int or \[4\] ints \(RB\), each in \[0, 3\]'):
            k.quota(bad, 3, 4)
    for bad in (torch.ones(4, dtype=torch.int64), torch.ones(3, dtype=torch.int32), torch.ones(8, dtype=torch.int32)[::2],
                torch.ones(4, dtype=torch.int32, device='meta')):
        with pytest.raises(ValueError, match=r'quota as a tensor must be contiguous int32 \[4\]'):
            k.quota(bad, 3, 4)
    # the preference pair, out= and the limits, refused before the library is touched
    f32, i32 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    before = _native.stable_launches
    for lp, rp in ((f32(2, 3, 4), f32(2, 3, 5)), (f32(2, 3, 4), f32(2, 3, 4).double()), (f32(3, 4), f32(3, 4)), (f32(2, 3, 8)[:, :, ::2], f32(2, 3, 4)),
                   (f32(2, 0, 4), f32(2, 0, 4)), (np.zeros((2, 3, 4), np.float32), f32(2, 3, 4)), (f32(2, 3, 4), f32(2, 3, 4).to('meta'))):
        with pytest.raises(ValueError, match=r'link_pref and rb_pref must be contiguous float32 tensors of one shape \[B, M, R\]'):
            k.solve(lp, rp, 1, None, 0)
    good = (i32(2, 3), i32(2, 4), i32(2), i32(2))
    shared = i32(2)
    for out in (good[:3], (good[0], good[1], shared, shared), (good[0], i32(2, 5), good[2], good[3]), good[0],
                (good[0], good[1], f32(2), good[3]), (i32(2, 6)[:, ::2], good[1], good[2], good[3])):
        with pytest.raises(ValueError, match=r'out must be \(col, load, proposals, unmatched\)'):
            k.solve(f32(2, 3, 4), f32(2, 3, 4), 1, out, 0)
    with pytest.raises(ValueError, match=r'quota must be an int or \[4\] ints \(RB\), each in \[0, 3\]'):
        k.solve(f32(2, 3, 4), f32(2, 3, 4), 4, good, 0)
    with pytest.raises(ValueError, match=r'serves at most 2048 rows and 8192 columns \(M = 2049, R = 1\)'):
        k.solve(f32(1, 2049, 1), f32(1, 2049, 1), 1, None, 0)
    need = _header_lds(2048, 6200)
    with pytest.raises(ValueError, match=rf'2048 rows on 6200 columns need {need} bytes, more than the 163840 \(D2D_STABLE_MAX_LDS_BYTES\)'):
        k.solve(torch.empty(1, 2048, 6200), torch.empty(1, 2048, 6200), 1, None, 0)
    # stable_rbs(): rb_pref, quota against the movable links and out=, before any launch
    planes = dict(pos_x=f32(3, 7), pos_y=f32(3, 7), rb=i32(3, 4), pwr=i32(3, 4))
    with pytest.raises(ValueError, match=r"rb_pref must be 'harm' or 'total', got 'own'"):
        k.rbs(planes, None, None, 1, 'own', None, 0)
    with pytest.raises(ValueError, match=r'quota must be an int or \[4\] ints \(RB\), each in \[0, 3\]'):
        k.rbs(planes, None, None, 4, 'harm', None, 0)                   # three movable links
    with pytest.raises(ValueError, match=r'each in \[0, 2\]'):
        k.rbs(planes, np.array([False, True, True, False]), None, 3, 'harm', None, 0)
    with pytest.raises(ValueError, match='movable marks link 0, which has no action column'):
        k.rbs(planes, np.array([True, True, False, False]), None, 1, 'harm', None, 0)
    for out in ((i32(3, 4), i32(3)), (i32(3, 4), shared, shared), (i32(3, 4), i32(3), f32(3)), i32(3, 4)):
        with pytest.raises(ValueError, match=r'out must be \(rb, unmatched, proposals\)'):
            k.rbs(planes, None, None, 1, 'harm', out, 0)
    assert _native.stable_launches == before


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_stable_library', lambda: pytest.fail('libd2d_stable.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._stable is None
    for call in (lambda: env.stable_rbs(), lambda: env.stable_rbs(quota=2, rb_pref='total'), lambda: env.stable_rbs_actions(),
                 lambda: env.solve_stable_matching(None, None)):
        with pytest.raises(ValueError, match=r'stable_rbs\(\) needs the torch path'):
            call()
    assert env._stable is None and env._assign is None
    env.close()


def test_stable_rbs_actions_encode_the_matched_rbs_on_a_stubbed_handle(monkeypatch):
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
    env.stable_rbs = lambda *a: seen.append(a) or (torch.as_tensor(rb, dtype=torch.int32), None, None)
    a = env.stable_rbs_actions('mask', 'allowed', 2, 'total')
    assert seen == [('mask', 'allowed', 2, 'total')]
    assert a.dtype == torch.int32 and tuple(a.shape) == (b, dues) == (b, env.num_agents)
    got_rb, got_pwr = orc.decode_actions(a.numpy(), levels[cues:])      # the env's own decode
    assert np.array_equal(got_rb, rb[:, cues:]) and np.array_equal(got_pwr, power[:, cues:])
    env.close()

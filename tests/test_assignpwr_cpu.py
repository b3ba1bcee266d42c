"""Joint RB and power matching with SINR floors, the part that needs no GPU: the library's exported set and its place in the build,
the entry point's refusals, the kernels' register budget, the float64 reference of the per-level planes against
assign_util.weights_ref and - matched - against brute force over placements x powers on complete assignments, the reference's side of
the GPU tests' caps, and the host module on a stub sim.

The power bounds are device arrays for the kernel (d2d_power_control's convention), so the entry point cannot read them: p_min >
p_max and an alphabet past 64 levels are refused by name where they are still host arrays, joint_assignment.check_alphabet, which
JointAssignment runs before anything is uploaded - tested here at that layer."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import assign_util as asu
import assignpwr_util as apu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


# ------------------------------------------------------------------------------------------ exports and tables
def test_assignpwr_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_assignpwr_library()
    assert _native.side_library('assignpwr') is lib
    header = (ROOT / 'include' / 'd2d_assignpwr.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_assignpwr.so') == declared == {'d2d_assign_power_weights', 'd2d_assignpwr_last_error'}
    assert set(_native.ASSIGNPWR_SIGNATURES) == declared and _native.ADDONS['assignpwr'] is _native.ASSIGNPWR_SIGNATURES
    assert len(_native.ASSIGNPWR_SIGNATURES['d2d_assign_power_weights'][1]) == 23
    for symbol, (res, args) in _native.ASSIGNPWR_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(lib.d2d_assignpwr_last_error(), bytes)
    for const in ('LAW_INV_SQUARE', 'LAW_POWER', 'LAW_POW_K', 'MAX_RBS', 'MAX_LDS_BYTES', 'MAX_LEVELS', 'CHUNK'):
        assert int(re.search(r'#define D2D_ASSIGNPWR_%s (\d+)' % const, header).group(1)) == getattr(_native, 'ASSIGNPWR_' + const), const
    assert int(re.search(r'#define D2D_ASSIGNPWR_NO_POWER \((-\d+)\)', header).group(1)) == _native.ASSIGNPWR_NO_POWER == apu.NO_POWER
    assert int(re.search(r'#define D2D_ASSIGNPWR_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    assert (_native.ASSIGNPWR_MAX_LEVELS, _native.ASSIGNPWR_CHUNK) == (apu.MAX_LEVELS, apu.CHUNK) == (64, 8)
    assert (_native.ASSIGNPWR_LAW_INV_SQUARE, _native.ASSIGNPWR_LAW_POWER, _native.ASSIGNPWR_LAW_POW_K, _native.ASSIGNPWR_MAX_RBS,
            _native.ASSIGNPWR_MAX_LDS_BYTES) == (_native.ASSIGN_LAW_INV_SQUARE, _native.ASSIGN_LAW_POWER, _native.ASSIGN_LAW_POW_K,
                                                 _native.ASSIGN_MAX_RBS, _native.ASSIGN_MAX_LDS_BYTES)
    # the further table: present in the build, the digest and the headers; the tables of the other libraries as they were
    assert build.ADDONS['assignpwr'] == ['d2d_assignpwr.hip'] and set(build.ADDONS) == set(_native.ADDONS)
    assert not set(build.ADDONS) & set(build.BUILT) and list(build.EVERYTHING) == list(build.BUILT) + list(build.ADDONS)
    assert ROOT / 'include' / 'd2d_assignpwr.h' in build.HEADERS and build.CSRC / 'd2d_assignpwr.hip' in build.digest_files()
    assert ROOT / 'include' / 'd2d_assignpwr.h' in build.digest_files()
    assert build.lib_path('assignpwr') == LIB_DIR / 'libd2d_assignpwr.so' == _native.side_path('assignpwr')
    assert _exports('libd2d_assign.so') == set(_native.ASSIGN_SIGNATURES)           # the matching library keeps its three


def test_a_missing_assignpwr_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.addons_built() and not build.addons_built(tmp_path)
    build.lib_path('assignpwr', tmp_path).touch()
    assert build.addons_built(tmp_path)
    # up to date by the stamp, the twelve and the solver, the add-on missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'addons_built', lambda lib_dir=build.LIB_DIR: False)
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_assignpwr\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_assignpwr_library()


# ------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, n_movable=1)

    def call(ptr=8, links=8, allowed=0, p_min=8, p_max=8, floor=0, out=8, power=16, **kw):
        a = dict(ok, **kw)
        _native.assign_power_weights(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'],
                                     a['n_rbs'], links, a['n_movable'], allowed, p_min, p_max, floor, out, power)
    before = _native.assign_power_weights_launches
    big = apu.lds_bytes(2048, 8192, True)
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.ASSIGNPWR_MAX_RBS + 1), 'n_rbs'), (dict(n_movable=0), 'n_movable'), (dict(n_movable=3), 'n_movable'),
                     (dict(law=3), 'unknown law'), (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'),
                     (dict(n_envs=-1), 'n_envs'), (dict(n_envs=2 ** 31), 'n_envs'), (dict(n_dev=0), 'n_dev'),
                     (dict(ptr=0), 'null device pointer'), (dict(links=0), 'null device pointer'), (dict(out=0), 'null device pointer'),
                     (dict(power=0), 'null device pointer'), (dict(p_min=0), 'null device pointer'), (dict(p_max=0), 'null device pointer'),
                     (dict(power=8), 'weights and power_dbm must be two planes'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=8192, law=1), f'n_links and n_rbs need {big} bytes of LDS, more than the 163840'),
                     (dict(n_links=2048, n_rbs=8192, law=1, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(floor=8), dict(allowed=8), dict(n_links=2048, n_rbs=64, n_movable=2048, law=1)):
        call(n_envs=0, **kw)                                           # nothing to do: accepted, and no launch on a device
    assert _native.assign_power_weights_launches == before


def test_a_bad_alphabet_is_refused_by_name_where_the_bounds_are_host_arrays():
    from gym_d2d_amd import joint_assignment as ja
    lo, hi = np.zeros(5, dtype=np.int32), np.full(5, 23, dtype=np.int32)
    ja.check_alphabet(lo, hi)
    ja.check_alphabet(lo, lo)                                           # one level
    ja.check_alphabet(lo - 40, hi - 1)                                  # 64 levels, p_min negative
    bad = hi.copy()
    bad[3] = -1
    with pytest.raises(ValueError, match=r'p_min > p_max for link 3 \(0 > -1\)'):
        ja.check_alphabet(lo, bad)
    ja.check_alphabet(lo, bad, links=[0, 1, 4])                         # a link that is never movable is not read
    wide = hi.copy()
    wide[2] = 64
    with pytest.raises(ValueError, match=r'link 2 has 65 power levels, more than the 64 .*D2D_ASSIGNPWR_MAX_LEVELS'):
        ja.check_alphabet(lo, wide)
    with pytest.raises(ValueError, match=r'\|p\| < 4096'):
        ja.check_alphabet(lo + 4090, hi + 4090)
    with pytest.raises(ValueError, match='one length'):
        ja.check_alphabet(lo, hi[:4])


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, assignment, joint_assignment as ja
    for n, r in ((1, 1), (3, 4), (63, 64), (257, 259), (1000, 8), (2048, 8192), (260, 4000)):
        for power_law in (False, True):
            assert ja.lds_bytes(n, r, power_law) == apu.lds_bytes(n, r, power_law) == assignment.lds_bytes(n, r, power_law)
    header = (ROOT / 'include' / 'd2d_assignpwr.h').read_text()
    assert '48 n_links + round16(8 n4) + 3 round16(4 n_links) + round16(4 (n_rbs + 1))' in header
    sizes = sorted(apu.lds_bytes(cues + dues, r, law != 'ld2') for cues, dues, r, law in apu.EXACT_CASES)
    assert sizes[-1] > 64 * 1024 >= sizes[-2]                           # one GPU case past the 64 KiB branch
    assert apu.lds_bytes(2048, 64, True) <= _native.ASSIGNPWR_MAX_LDS_BYTES < apu.lds_bytes(2048, 8192, False)


# ------------------------------------------------------------------------------------------ the kernels' budget
@pytest.fixture(scope='module')
def kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_assignpwr')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_assignpwr.hip'), '-save-temps', '-o', 'ap.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'assign_power_weights_kernelILi\dELb[01]EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[m.group(0)] = {k: field(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size',
                                                 'group_segment_fixed_size')}
    return out, asm


def test_kernels_use_no_scratch_no_atomics_and_the_stated_registers(kernels):
    """Six kernels (law in {0, 1, 4} x floors in {0, 1}).  The figures of the build this was written on: 106 - 114 VGPRs without
    floors, 113 - 120 with; the header states at most 128, which keeps four waves per SIMD - one workgroup of 256 threads is one wave
    per SIMD, and the LDS of an env is what bounds the workgroups per CU.  LDS is dynamic."""
    found, asm = kernels
    assert len(found) == 6
    header = (ROOT / 'include' / 'd2d_assignpwr.h').read_text()
    assert 'No scratch memory; at most 128 VGPRs per kernel' in header
    for key, k in found.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0, (key, k)
        assert k['vgpr_count'] <= 128, (key, k)
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_assignpwr.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code and 'nontemporal' not in code
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'scratch_' not in asm


# ------------------------------------------------------------------------------------------ the float64 reference
@pytest.mark.parametrize('cues,dues,r,law', [(2, 3, 4, 'mixed'), (13, 50, 64, 'mixed'), (100, 200, 1, 'ld2')])
def test_one_level_at_the_planes_power_without_floors_is_weights_ref(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    own, harm, near = asu.weights_ref(c, links)
    none = np.full(c['n'], -np.inf)
    got_own, got_harm, adm, got_near = apu.level_ref(c, links, np.asarray(c['pwr'])[0, links], none)
    # the case's power plane differs per env: env 0 against env 0, then env 1 at its own powers
    assert np.array_equal(got_own[0], own[0]) and np.array_equal(got_harm[0], harm[0]) and np.array_equal(got_near[0], near[0])
    got = apu.level_ref(c, links, np.asarray(c['pwr'])[1, links], none)
    assert np.array_equal(got[0][1], own[1]) and np.array_equal(got[1][1], harm[1]) and np.array_equal(got[3][1], near[1])
    assert adm.all()
    # ... and through weights_power_ref with p_min = p_max: one level, every entry admissible
    p = np.asarray(c['pwr'])[0].astype(np.int32)
    w, valid, marks = apu.weights_power_ref(c, links, p, p)
    assert w.shape == own.shape + (1,) and valid.all() and marks[0][0].all()
    assert np.array_equal(w[0, ..., 0], (own - harm)[0])
    best, level = apu.best_power(w, valid, marks[0][0])
    assert np.array_equal(best[0], (own - harm)[0]) and (level == 0).all()


@pytest.mark.parametrize('cues,dues,r,law', apu.SMALL_CASES)
@pytest.mark.parametrize('pair', apu.SMALL_FLOORS)
def test_matching_the_best_power_weights_is_the_joint_optimum_of_brute_force(cues, dues, r, law, pair):
    """The Hungarian optimum of max over the admissible p of w[a, r, p] (assign_util.solve_ref in float64) against brute force over
    every one-to-one placement x every power vector on COMPLETE assignments through evaluate_util.evaluate_ref, admissibility judged
    there: equal to 1e-9, and infeasible together.  Measured: 0 - 3.8e-16."""
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    floor = apu.class_floors(c, cues, pair)
    powers = np.asarray(apu.SMALL_LEVELS)
    w = np.zeros((c['b'], len(links), r, len(powers)))
    adm = np.zeros(w.shape, bool)
    for l, p in enumerate(powers):
        own, harm, adm[..., l], _ = apu.level_ref(c, links, np.full(len(links), p), floor)
        w[..., l] = own - harm
    best, level = apu.best_power(w, np.ones((len(links), len(powers)), bool), adm)
    brute = apu.brute_force(c, links, powers, floor)
    worst = 0.0
    for e in range(c['b']):
        col, _, ok = asu.solve_ref(best[e])
        assert bool(ok) == (brute[e] is not None), (e, brute[e])
        if ok:
            got = float(best[e][np.arange(len(links)), col].sum())
            worst = max(worst, abs(got - brute[e]) / max(abs(brute[e]), 1.0))
    print(f'{cues} + {dues} links, {r} RBs, {law}, floors {pair}: matching against brute force {worst:.2e}; {adm.mean():.1%} admissible; '
          f'feasible {[v is not None for v in brute]}; best level inside the alphabet {((level > 0) & (level < len(powers) - 1)).mean():.1%}')
    assert worst <= 1e-9


# ------------------------------------------------------------------------------------------ the GPU cases, reference side
@pytest.mark.parametrize('cues,dues,r,law', apu.FLOOR_CASES)
def test_threshold_share_and_admissibility_of_the_gpu_cases(cues, dues, r, law):
    """The seeds of the GPU comparison, on the reference alone: at most 1 % of a case's entries carry a near-threshold mark at any
    level, under every floor setting; a floored case has admissible and inadmissible entries (the smallest has too few entries to
    promise either)."""
    w, valid, marks = apu.floor_case_ref(cues, dues, r, law)
    movable = len(apu.floor_links(asu.case(cues, dues, r, law), cues, dues, r, law))
    assert movable == (25 if r == 4000 else dues)
    assert valid.all() and w.shape == (asu.B, movable, r, 21) and np.isfinite(w).all()
    for pair, (adm, near) in zip((None,) + apu.FLOOR_SETTINGS, marks):
        share = float(near.any(axis=3).mean())
        best, level = apu.best_power(w, valid, adm)
        inside = float(((level > 0) & (level < 20)).mean())
        print(f'{cues} + {dues} links, {r} RBs, {law}, floors {pair}: near-threshold share {share:.2e}, admissible {adm.mean():.3f}, '
              f'best power strictly inside the alphabet {inside:.3f}, rows without an admissible RB {(~np.isfinite(best)).all(axis=2).mean():.2f}')
        assert share <= apu.THRESHOLD_CAP
        if pair is None:
            assert adm.all()
        elif (cues, dues, r, law) != (1, 2, 4, 'ld35'):
            assert adm.any() and not adm.all()
    if (cues, dues, r, law) == (100, 200, 1, 'ld2'):                    # the scan is tested on more than ties with p_max
        best, level = apu.best_power(w, valid, marks[0][0])
        assert ((level > 0) & (level < 20)).mean() > 0.1
    if (cues, dues, r, law) == (57, 200, 259, 'ld35'):                  # the infeasible route: rows with no admissible RB at all
        best, _ = apu.best_power(w, valid, marks[2][0])
        assert (~np.isfinite(best)).all(axis=2).mean() > 0.3


def test_threshold_share_of_the_scattered_case_stays_inside_the_cap():
    w, valid, marks = apu.scattered_floor_ref()
    assert w.shape[3] == 24 and valid[:, :18].all() and not valid.all()     # the DUE links' alphabet ends at 18 levels
    for pair, (adm, near) in zip((None,) + apu.FLOOR_SETTINGS, marks):
        share = float(near.any(axis=3).mean())
        print(f'scattered movable, floors {pair}: near-threshold share {share:.2e}, admissible {adm.any(axis=3).mean():.3f}')
        assert share <= apu.THRESHOLD_CAP and not (adm & ~valid[None, :, None, :]).any()
        assert adm.any() and (pair is None or not adm[:, :, :, :18].all())


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


def test_refusal_texts_are_assign_rbs_under_this_name():
    from gym_d2d_amd import assignment, joint_assignment as ja
    assert ja.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: ja.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = ja.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and 'assign_rbs_power()' in text and 'assign_rbs()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():
        assert texts[needle] == assignment.refusal(*args).replace('assign_rbs()', 'assign_rbs_power()')


def _kernel(p_max=(23, 23, 20, 20), num_rbs=4):
    import torch
    from gym_d2d_amd import joint_assignment as ja
    agent = np.ones(4, bool)
    due = np.array([False, False, True, True])
    return ja.JointAssignment(_stub_sim(num_rbs=num_rbs), 4, agent, due, np.zeros(4, np.int32), np.asarray(p_max, np.int32), torch,
                              torch.device('cpu'))


def test_the_floor_forms_the_bounds_and_the_links_on_a_stub_sim():
    import torch
    from gym_d2d_amd import sensing
    k = _kernel()
    assert isinstance(k, sensing.PairKernel) and hasattr(k, 'cap_cols') and len(k.ptrs) == 4
    assert k.p_min.dtype == torch.int32 and k.p_max.tolist() == [23, 23, 20, 20]
    assert k.floors(None, 2) is None
    assert k.floors(3.0, 2).tolist() == [3.0] * 4 and k.floors(3.0, 2).dtype == torch.float32
    assert k.floors({'cue': 5.0, 'due': -np.inf}, 2).tolist() == [5.0, 5.0, -np.inf, -np.inf]
    same = k.floors([1.0, 2.0, 3.0, 4.0], 2)
    assert same.tolist() == [1.0, 2.0, 3.0, 4.0] and k.floors(np.array([1.0, 2.0, 3.0, 4.0]), 2) is same      # not uploaded again
    assert k.floors(torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), 2).dtype == torch.float32
    for bad in ({'cue': 1.0}, [1.0, 2.0], float('nan'), torch.zeros(3)):
        with pytest.raises(ValueError, match='min_sinr_db'):
            k.floors(bad, 2)
    host, dev = k.links(None)
    assert host.tolist() == [2, 3] and dev.tolist() == [2, 3]           # the DUE-pair links
    assert k.links(np.array([True, False, False, True]))[0].tolist() == [0, 3]
    with pytest.raises(ValueError, match='movable marks no link'):
        k.links(np.zeros(4, bool))
    with pytest.raises(ValueError, match=r'3 movable links cannot have an RB each on 2 RBs: M = 3 must be <= R = 2'):
        _kernel(num_rbs=2).assign_power({}, np.array([True, True, True, False]), None, None, None, 0)
    with pytest.raises(ValueError, match=r'link 1 has 65 power levels'):
        _kernel(p_max=(23, 64, 20, 20))
    with pytest.raises(ValueError, match=r'p_min > p_max for link 2'):
        _kernel(p_max=(23, 23, -1, 20))
    with pytest.raises(ValueError, match=r'assign_rbs_power\(\) serves at most 8192 RBs'):
        _kernel(num_rbs=8193)


def test_the_action_encoding_puts_rb_and_power_into_the_envs_layout():
    from gym_d2d_amd import power_control
    rb = np.array([[3, 1, 0, 2], [0, 0, 1, 3]])
    power = np.array([[23, 0, 7, 20], [5, 6, 0, 1]])
    p_min, p_max = power_control.class_bounds({'cue': 24, 'due': 21}, 'cue', 2, 2)
    assert p_min.tolist() == [0] * 4 and p_max.tolist() == [23, 23, 20, 20]
    act = power_control.encode_actions(rb, power, p_min, p_max - p_min + 1)
    assert act.dtype == np.int32 and act.tolist() == [[3 * 24 + 23, 24, 7, 2 * 21 + 20], [5, 6, 21, 3 * 21 + 1]]
    assert (act // (p_max + 1) == rb).all() and (act % (p_max + 1) == power).all()
    # links on fixed actions come first and have no column
    assert power_control.encode_actions(rb, power, p_min[2:], (p_max - p_min + 1)[2:], 2).tolist() == [[7, 62], [21, 64]]


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_assignpwr_library', lambda: pytest.fail('libd2d_assignpwr.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._joint is None
    for call in (env.joint_assignment_weights, env.assign_rbs_power, env.assign_rbs_power_actions):
        with pytest.raises(ValueError, match=r'assign_rbs_power\(\) needs the torch path'):
            call()
    env.close()

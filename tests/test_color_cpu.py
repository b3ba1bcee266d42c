"""Conflict-graph RB colouring, the part that needs no GPU: the library's exported set and its place in the build, the entry point's
refusals, the kernel's register report, the known answers of DSATUR through the NumPy restatement (color_util), and the host module
on a stub sim."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import color_util as cu

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'
HEADER = ROOT / 'include' / 'd2d_color.h'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


# ------------------------------------------------------------------------------------------ exports and tables
def test_color_library_exports_exactly_its_header_and_is_built_with_the_rest():
    from gym_d2d_amd import _native, build
    lib = _native.load_color_library()
    assert _native.side_library('color') is lib
    header = HEADER.read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_color.so') == declared == {'d2d_color_graph', 'd2d_color_last_error'}
    assert set(_native.COLOR_SIGNATURES) == declared and _native.ADDONS['color'] is _native.COLOR_SIGNATURES
    assert len(_native.COLOR_SIGNATURES['d2d_color_graph'][1]) == 15
    for symbol, (res, args) in _native.COLOR_SIGNATURES.items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(lib.d2d_color_last_error(), bytes)
    for const in ('MAX_LINKS', 'MAX_RBS', 'MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_COLOR_%s (\d+)' % const, header).group(1)) == getattr(_native, 'COLOR_' + const), const
    assert _native.COLOR_MAX_LINKS == _native.MAX_LINKS and _native.COLOR_MAX_LDS_BYTES == 160 * 1024
    # the add-on table: present in the build, the digest and the headers; the other tables as they were
    assert build.ADDONS['color'] == ['d2d_color.hip'] and set(build.ADDONS) == set(_native.ADDONS)
    assert 'color' not in build.LIBRARIES and 'color' not in build.SOLVERS and 'color' not in build.BUILT
    assert 'color' not in _native.SIDE and 'color' not in _native.SOLVERS
    assert HEADER in build.HEADERS and HEADER in build.digest_files() and build.CSRC / 'd2d_color.hip' in build.digest_files()
    assert build.lib_path('color') == LIB_DIR / 'libd2d_color.so' == _native.side_path('color')


def test_a_missing_color_library_is_rebuilt_and_says_how(tmp_path, monkeypatch):
    from gym_d2d_amd import _native, build
    assert build.addons_missing() == [] and build.addons_missing(tmp_path) == list(build.ADDONS)
    build.lib_path('assignpwr', tmp_path).touch()
    assert build.addons_missing(tmp_path) == ['color']
    build.lib_path('color', tmp_path).touch()
    assert build.addons_missing(tmp_path) == []
    # up to date by the stamp and every other library, this one missing: build() reaches for the compiler
    monkeypatch.setattr(build, 'addons_missing', lambda lib_dir=build.LIB_DIR: ['color'])
    monkeypatch.setattr(build, '_hipcc', lambda: (_ for _ in ()).throw(RuntimeError('reached the compiler')))
    assert build.up_to_date(build.source_digest()) and build.solvers_built() and build.addons_built()
    with pytest.raises(RuntimeError, match='reached the compiler'):
        build.build()
    monkeypatch.setattr(_native, '_side', {})
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / 'nowhere' / f'libd2d_{n}.so')
    with pytest.raises(ImportError, match=r'libd2d_color\.so is missing - build it with `python -m gym_d2d_amd\.build`'):
        _native.load_color_library()


def test_lds_bytes_are_the_headers_formula():
    from gym_d2d_amd import _native, coloring
    header = HEADER.read_text()
    assert 'round16(4 n_links W) + (1 + has_allowed) round16(4 n_links words) + 3 round16(4 n_links) + 2 round16(4 n_rbs)' in header
    assert '+ round16(4 words) + 64' in header
    for n, r in ((1, 1), (2, 1), (37, 5), (64, 32), (65, 33), (300, 40), (800, 24), (512, 256), (2048, 8192)):
        for allowed in (False, True):
            assert coloring.lds_bytes(n, r, allowed) == cu.lds_bytes(n, r, allowed), (n, r, allowed)
    assert cu.lds_bytes(1, 1, False) == 16 + 16 + 48 + 32 + 16 + 64
    assert cu.lds_bytes(800, 24, False) > 64 * 1024 > cu.lds_bytes(300, 40, True)      # one GPU case past the 64 KiB branch
    assert cu.lds_bytes(1056, 64, False) <= _native.COLOR_MAX_LDS_BYTES < cu.lds_bytes(1088, 64, False)


# ------------------------------------------------------------------------------------------ the entry point
def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(n_envs=2, n_links=3, n_rbs=2)

    def call(score=8, bias=0, thr=8, rb=8, allowed=0, movable=0, pack=False, out=(8, 16, 24, 32), **kw):
        a = dict(ok, **kw)
        _native.color_graph(score, bias, thr, rb, a['n_envs'], a['n_links'], a['n_rbs'], allowed, movable, pack, *out)
    before = _native.color_launches
    big = cu.lds_bytes(2048, 64, False)
    assert big > _native.COLOR_MAX_LDS_BYTES
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.COLOR_MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.COLOR_MAX_RBS + 1), 'n_rbs'), (dict(n_envs=-1), 'n_envs'), (dict(n_envs=2 ** 31), 'n_envs'),
                     (dict(score=0), 'null device pointer'), (dict(thr=0), 'null device pointer'), (dict(rb=0), 'null device pointer'),
                     (dict(out=(0, 16, 24, 32)), 'null device pointer'), (dict(out=(8, 0, 24, 32)), 'null device pointer'),
                     (dict(out=(8, 16, 0, 32)), 'null device pointer'), (dict(out=(8, 16, 24, 0)), 'null device pointer'),
                     (dict(out=(8, 16, 16, 32)), 'rb_out, conflicts, rbs_used and proper must be four arrays'),
                     (dict(out=(8, 16, 24, 8)), 'must be four arrays'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, n_rbs=64), rf'n_links and n_rbs need {big} bytes of LDS, more than the 163840 \(D2D_COLOR_MAX_LDS_BYTES\)'),
                     (dict(n_links=2048, n_rbs=64, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    for kw in (dict(), dict(bias=8), dict(allowed=8, movable=8, pack=True), dict(n_links=1056, n_rbs=64), dict(n_links=1, n_rbs=1)):
        call(n_envs=0, **kw)                                            # nothing to do: accepted, and no launch on a device
    assert _native.color_launches == before


# ------------------------------------------------------------------------------------------ the kernel's budget
def test_register_report_shows_no_spills_no_private_segment_and_no_static_lds(tmp_path):
    from gym_d2d_amd import build
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_color.hip'), '-save-temps', '-o', 'color.o']
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp_path.glob('*gfx950*.s')).read_text()
    found = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        if not name or 'color_kernel' not in name.group(1):
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        found[name.group(1)] = {k: field(k) for k in ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size', 'max_flat_workgroup_size')}
    assert len(found) == 1
    header = HEADER.read_text()
    assert 'No scratch memory; at most 64 VGPRs' in header
    for key, k in found.items():
        print(key, k)
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0 and k['agpr_count'] == 0 and k['max_flat_workgroup_size'] == 256, (key, k)
        assert k['vgpr_count'] <= 64, (key, k)
    assert 'scratch_' not in asm
    # LDS atomics on integers only: no global / flat / buffer atomic, no floating-point atomic
    assert not re.search(r'^\s*(global|flat|buffer)_atomic', asm, flags=re.M)
    assert not re.search(r'^\s*ds_\w*_(f32|f64|rtn_f32|rtn_f64)\b', asm, flags=re.M)


# ------------------------------------------------------------------------------------------ the known answers, through the restatement
def _random_graph(rng, n, p):
    a = np.triu(rng.random((n, n)) < p, 1)
    return a | a.T


def _cycle(n):
    a = np.zeros((n, n), dtype=bool)
    for i in range(n):
        a[i, (i + 1) % n] = a[(i + 1) % n, i] = True
    return a


@pytest.mark.parametrize('pack', [False, True])
def test_max_degree_below_r_always_ends_proper_and_never_needs_a_forced_choice(pack):
    """A link has at most deg < R RBs among its neighbours, so a free allowed RB always exists: conflicts 0 - with a random
    precoloured background, whose own same-RB edges are not counted."""
    rng = np.random.default_rng(11 + pack)
    for trial in range(120):
        n = int(rng.integers(2, 40))
        adj = _random_graph(rng, n, rng.uniform(0.05, 0.5))
        r = int(adj.sum(axis=1).max()) + 1 + int(rng.integers(0, 3))
        movable = rng.random(n) < 0.7
        rb = rng.integers(-1, r + 2, size=n)
        col, conflicts, used, proper = cu.color_adjacency(adj, r, pack, rb=rb, movable=movable)
        assert conflicts == 0 and proper == 1, (trial, n, r)
        assert (col[~movable] == rb[~movable]).all() and ((col[movable] >= 0) & (col[movable] < r)).all()
        assert used == len(set(col[movable].tolist()))
        assert cu.same_rb_edges(adj, col, movable, r) == 0


def test_pack_colours_every_bipartite_graph_that_has_an_edge_with_exactly_two_rbs():
    rng = np.random.default_rng(5)
    done = 0
    for trial in range(150):
        n = int(rng.integers(2, 30))
        side = rng.random(n) < 0.5
        adj = _random_graph(rng, n, rng.uniform(0.05, 0.6)) & (side[:, None] != side[None, :])      # disconnected ones included
        if not adj.any():
            continue
        col, conflicts, used, proper = cu.color_adjacency(adj, 6, True)
        assert (conflicts, used, proper) == (0, 2, 1), (trial, n)
        assert set(col.tolist()) == {0, 1}
        done += 1
    assert done > 100


def test_pack_colours_even_cycles_with_two_rbs_and_odd_cycles_with_three():
    for n in (4, 6, 10, 64, 100):
        assert cu.color_adjacency(_cycle(n), 5, True)[1:] == (0, 2, 1)
    for n in (3, 5, 9, 65, 101):
        assert cu.color_adjacency(_cycle(n), 5, True)[1:] == (0, 3, 1)


@pytest.mark.parametrize('m,r,loads,conflicts', [(7, 3, [3, 2, 2], 5), (10, 4, [3, 3, 2, 2], 8), (5, 1, [5], 10)])
@pytest.mark.parametrize('pack', [False, True])
def test_the_complete_graph_on_fewer_rbs_ends_balanced(m, r, loads, conflicts, pack):
    """K_M on R < M: once every RB is taken the least-conflicting one is the least loaded, whatever pack says."""
    col, got, used, proper = cu.color_adjacency(~np.eye(m, dtype=bool), r, pack)
    assert np.bincount(col, minlength=r).tolist() == loads and got == conflicts == sum(n * (n - 1) // 2 for n in loads)
    assert used == r and proper == 0
    assert cu.same_rb_edges(~np.eye(m, dtype=bool), col, np.ones(m, bool), r) == conflicts


def test_the_empty_graph_spreads_round_robin_and_packs_onto_rb_0():
    none = np.zeros((10, 10), dtype=bool)
    col, conflicts, used, proper = cu.color_adjacency(none, 4, False, rb=np.full(10, -1))
    assert col.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1] and (conflicts, used, proper) == (0, 4, 1)
    col, conflicts, used, proper = cu.color_adjacency(none, 4, True, rb=np.full(10, -1))
    assert col.tolist() == [0] * 10 and (conflicts, used, proper) == (0, 1, 1)


def test_background_allowed_masks_and_no_turn_taker():
    adj = _cycle(4)
    # links 1 and 3 are background on RB 0 and on no RB (R + 5): link 0 and 2 see RB 0 forbidden
    col, conflicts, used, proper = cu.color_adjacency(adj, 2, True, rb=[1, 0, 1, 7], movable=np.array([True, False, True, False]))
    assert col.tolist() == [1, 0, 1, 7] and (conflicts, used, proper) == (0, 1, 1)
    # the only allowed RB is the neighbour's: a forced conflict, counted once
    allowed = np.array([[True, False], [True, True], [True, True], [True, True]])
    col, conflicts, used, proper = cu.color_adjacency(adj, 2, True, rb=[1, 0, 1, 7], movable=np.array([True, False, False, False]),
                                                      allowed=allowed)
    assert col.tolist() == [0, 0, 1, 7] and (conflicts, used, proper) == (1, 1, 0)
    # a background edge on one RB is nobody's conflict; M = 0 scores nothing
    col, conflicts, used, proper = cu.color_adjacency(adj, 2, False, rb=[0, 0, 0, 0], movable=np.zeros(4, bool))
    assert col.tolist() == [0, 0, 0, 0] and (conflicts, used, proper) == (0, 0, 1)
    # an empty allowed row makes a movable link background
    allowed = np.ones((4, 2), dtype=bool)
    allowed[2] = False
    assert cu.turn_takers(4, 2, None, allowed).tolist() == [True, True, False, True]


def test_the_conflict_graph_is_float32_one_directional_and_nan_safe():
    score = np.zeros((3, 3), dtype=np.float32)
    score[2, 0] = 1.0                                                   # only d(2<-0) holds
    thr = np.full(3, 0.5, dtype=np.float32)
    adj = cu.conflict_graph(score, None, thr)
    assert adj.tolist() == [[False, False, True], [False, False, False], [True, False, False]]
    score[:] = np.nan
    assert not cu.conflict_graph(score, None, thr).any()
    score[:] = 3.0
    assert not cu.conflict_graph(score, None, np.array([np.nan, np.inf, np.nan], dtype=np.float32)).any()
    adj = cu.conflict_graph(score, None, np.array([np.inf, -np.inf, np.inf], dtype=np.float32))
    assert adj.tolist() == [[False, True, False], [True, False, True], [False, True, False]]       # link 1 is everybody's victim
    # the sum is ONE float32 addition: 2^24 + 1 is 2^24 in float32, and does not reach the next float32
    score[:] = np.float32(2 ** 24)
    nxt = np.nextafter(np.float32(2 ** 24), np.float32(np.inf))
    bias = np.ones(3, dtype=np.float32)
    assert not cu.conflict_graph(score, bias, np.full(3, nxt, dtype=np.float32)).any()
    assert cu.conflict_graph(score, 2 * bias, np.full(3, nxt, dtype=np.float32)).sum() == 6


def test_rx_thr_is_float32_in_exactly_the_stated_association():
    from gym_d2d_amd import coloring
    rng = np.random.default_rng(2)
    c = (-90.0 + 30.0 * rng.random((40, 6, 6))).astype(np.float32)
    p = rng.integers(0, 24, size=(40, 6)).astype(np.float32)
    m = np.array([0.1, 3.3, -np.inf, 7.7, 1e-3, 12.6], dtype=np.float32)
    thr = coloring.sir_threshold(c, p, m)
    diag = np.stack([np.diag(c[e]) for e in range(40)])
    want = (diag + p) - m[None, :]
    assert thr.dtype == np.float32 and want.dtype == np.float32 and np.array_equal(thr, want)
    assert (thr[:, 2] == np.inf).all()                                  # -inf: never a victim
    other = diag + (p - m[None, :])
    assert (other[:, [0, 1, 3, 4, 5]] != want[:, [0, 1, 3, 4, 5]]).any()    # the association is not a formality
    import torch
    got = coloring.sir_threshold(torch.as_tensor(c), torch.as_tensor(p), torch.as_tensor(m))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)


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


def test_refusal_texts_name_color_rbs():
    from gym_d2d_amd import coloring, sensing
    assert coloring.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'export_actions=True': (_stub_sim(), False), "'link_table'": (_stub_sim(route='link_table'), True),
             "'per_step'": (_stub_sim(route='per_step'), True), "'channel'": (_stub_sim(route='channel'), True),
             'ShadowingPathLoss': (_stub_sim(shadowing=True), True), 'float32 cannot hold': (pinned, True)}
    texts = {needle: coloring.refusal(*args) for needle, args in stubs.items()}
    texts['torch path'] = coloring.refusal(_stub_sim(), True, use_torch=False)
    for needle, text in texts.items():
        assert needle in text and text.startswith('color_rbs() '), (needle, text)
    assert len(set(texts.values())) == len(texts)
    for needle, args in stubs.items():                                  # refused exactly where coupling() is
        assert sensing.unserved(*args) is not None


def test_the_kernel_object_checks_its_arguments_on_a_stub_sim():
    import torch
    from gym_d2d_amd import coloring, sensing
    agent = np.array([False, True, True, True])                        # link 0 is on fixed actions
    k = coloring.Coloring(_stub_sim(), 4, agent, torch, torch.device('cpu'))
    assert isinstance(k, sensing.PairKernel) and (k.b, k.n, k.r) == (3, 4, 4)
    assert k.movable(None).tolist() == [0, 1, 1, 1] and k.movable(np.array([True, True, False, False])).tolist() == [0, 1, 0, 0]
    with pytest.raises(ValueError, match=r'movable must be bool \[4\]'):
        k.movable(np.zeros(3, bool))
    assert k.margin(3.0, 2).tolist() == [3.0] * 4 and k.margin(3.0, 2).dtype == torch.float32
    assert k.margin({'cue': 5.0, 'due': -np.inf}, 2).tolist() == [5.0, 5.0, -np.inf, -np.inf]
    same = k.margin([1.0, 2.0, 3.0, 4.0], 2)
    assert k.margin(np.array([1.0, 2.0, 3.0, 4.0]), 2) is same         # not uploaded again
    for bad in (float('nan'), {'cue': 1.0}, [1.0, 2.0], torch.tensor([1.0, float('nan'), 0.0, 0.0]), torch.zeros(3)):
        with pytest.raises(ValueError, match='margin_db'):
            k.margin(bad, 2)
    score, thr, rb = torch.zeros(3, 4, 4), torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.int32)
    mov = k.movable(None)
    for kw, text in ((dict(score=torch.zeros(3, 4, 5)), r'score must be a contiguous float32 tensor \[3, 4, 4\]'),
                     (dict(score=score.double()), 'score must be'), (dict(score=torch.zeros(3, 4, 8)[:, :, ::2]), 'score must be'),
                     (dict(rx_thr=torch.zeros(3, 5)), r'rx_thr must be a contiguous float32 tensor \[3, 4\]'),
                     (dict(rx_thr=None), 'rx_thr must be'), (dict(tx_bias=torch.zeros(4)), r'tx_bias must be .* or None'),
                     (dict(pack=2), 'pack must be True or False'), (dict(pack='yes'), 'pack must be'),
                     (dict(allowed=np.ones((4, 5), bool)), r'allowed must be bool \[4, 4\]'),
                     (dict(out=(rb, thr, thr, thr)), r'out must be \(rb, conflicts, rbs_used, proper\)')):
        a = dict(dict(score=score, rx_thr=thr, tx_bias=None, pack=False, allowed=None, out=None), **kw)
        with pytest.raises(ValueError, match=text):
            k.color(rb, a['score'], a['rx_thr'], a['tx_bias'], mov, a['allowed'], a['pack'], a['out'], 0)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    shared = i32(3)
    with pytest.raises(ValueError, match='do not share memory'):
        k.outputs((i32(3, 4), shared, shared, torch.zeros(3, dtype=torch.uint8)))
    good = (i32(3, 4), i32(3), i32(3), torch.zeros(3, dtype=torch.uint8))
    assert k.outputs(good) == good and k.outputs(None) is k.outputs(None)
    with pytest.raises(ValueError, match=r'color_rbs\(\) serves at most 8192 RBs'):
        coloring.Coloring(_stub_sim(num_rbs=8193), 4, agent, torch, torch.device('cpu'))
    # past the LDS of a workgroup: refused by name with the bytes, before anything is launched
    wide = SimpleNamespace(**{**vars(_stub_sim()), 'link_tx': np.ones(2048, dtype=np.int64), 'link_rx': np.zeros(2048, dtype=np.int64)})
    kw = coloring.Coloring(wide, 2048, np.ones(2048, bool), torch, torch.device('cpu'))
    with pytest.raises(ValueError, match=rf'2048 links on 4 RBs need {cu.lds_bytes(2048, 4, False)} bytes, more than the 163840 \(D2D_COLOR_MAX_LDS_BYTES\)'):
        kw.color(i32(3, 2048), torch.zeros(3, 2048, 2048), torch.zeros(3, 2048), None, kw.movable(None), None, False, None, 0)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    monkeypatch.setattr(_native, 'load_color_library', lambda: pytest.fail('libd2d_color.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._color is None
    for call in (lambda: env.color_graph(None, None), lambda: env.color_rbs(3.0), lambda: env.color_rbs_actions(3.0)):
        with pytest.raises(ValueError, match=r'color_rbs\(\) needs the torch path'):
            call()
    assert env._color is None
    env.close()

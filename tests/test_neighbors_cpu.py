"""The neighbour graph, the part that needs no GPU: the library's exported set, refusals before any launch, the kernels' register and
LDS budgets, the observation's surface, and the GPU tests' yardstick (neighbors_util) on the oracle alone."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import neighbors_util as nbu
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_graph_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    lib = _native.load_graph_library()
    header = (ROOT / 'include' / 'd2d_graph.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_graph.so') == declared == {'d2d_graph_coupling', 'd2d_graph_neighbors', 'd2d_graph_neighbor_obs',
                                                      'd2d_graph_last_error'}
    assert set(_native.GRAPH_SIGNATURES) == declared
    # the header's parameter counts against the signature table
    for name in declared:
        params = re.search(r'^(?:int|const char\*) %s\(([^;]*)\);' % name, header, flags=re.S | re.M).group(1)
        want = 0 if params.strip() == 'void' else params.count(',') + 1
        assert len(_native.GRAPH_SIGNATURES[name][1]) == want, name
        assert getattr(lib, name).restype is not None
    assert int(re.search(r'#define D2D_GRAPH_MAX_K (\d+)', header).group(1)) == _native.GRAPH_MAX_K == 64
    assert int(re.search(r'#define D2D_GRAPH_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    assert 'receiver-major' in header and '[b][j][i]' in header                      # the index order is stated where the ABI is


def test_the_other_libraries_keep_their_symbols():
    from gym_d2d_amd import _native
    assert len(_exports('libd2d_hip.so')) == 43 == len(_native.SIGNATURES)
    assert _exports('libd2d_sense.so') == {'d2d_sense_rb', 'd2d_sense_last_error'}


def test_graph_entry_points_refuse_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=4, k=2)
    p = 8

    def coupling(ptr=p, **kw):
        a = dict(ok, **kw)
        _native.graph_coupling(ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], ptr)

    def neighbors(ptr=p, mask=0, **kw):
        a = dict(ok, **kw)
        _native.graph_neighbors(ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['k'], mask, ptr, ptr)

    def obs(ptr=p, **kw):
        a = dict(ok, **kw)
        _native.graph_neighbor_obs(ptr, ptr, ptr, ptr, ptr, ptr, a['n_envs'], a['n_links'], a['k'], ptr)
    before = dict(_native.graph_launches)
    common = ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(law=3), 'law'),
              (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'), (dict(n_dev=0), 'n_dev'),
              (dict(ptr=0), 'null device pointer'))
    for fn in (coupling, neighbors):
        for kw, text in common:
            with pytest.raises(_native.NativeError, match=text):
                fn(**kw)
    for kw in (dict(k=0), dict(k=4), dict(k=-1), dict(n_links=200, k=65), dict(n_links=1, k=1)):
        with pytest.raises(_native.NativeError, match='k must be'):
            neighbors(**kw)
    for kw, text in ((dict(k=-1), 'k must be'), (dict(k=65), 'k must be'), (dict(n_links=0), 'n_links'), (dict(n_envs=-1), 'n_envs'),
                     (dict(ptr=0), 'null device pointer')):
        with pytest.raises(_native.NativeError, match=text):
            obs(**kw)
    assert _native.graph_launches == before
    # n_envs == 0 is nothing to do, not an error - and not a launch either, though the wrapper counts the accepted call
    coupling(n_envs=0); neighbors(n_envs=0); obs(n_envs=0)


@pytest.fixture(scope='module')
def graph_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_graph')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_graph.hip'), '-save-temps', '-o', 'graph.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'\d+(coupling_kernel|neighbors_kernel|neighbor_obs_kernel)(?:ILi(\d)E(?:Lb(\d)E)?E)?', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        key = (m.group(1),) + tuple(int(x) for x in m.groups()[1:] if x is not None)
        out[key] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                          'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out, asm


def test_graph_kernels_use_no_scratch_and_spill_nothing(graph_kernels):
    """coupling_kernel<law in {0, 1, 4}, 16-byte stores or not>, neighbors_kernel<law>, neighbor_obs_kernel.  The figures of the build
    this was written on: coupling 36 / 39 VGPRs (inverse square), 50 / 52 (power), 38 / 42 (pow-k), 2 KiB of static LDS (the 128
    receivers of a workgroup); neighbors 40 / 24 / 18 VGPRs, LDS dynamic; the gather 24 VGPRs, no LDS."""
    kernels, _ = graph_kernels
    want = {('coupling_kernel', m, v) for m in (0, 1, 4) for v in (0, 1)} | {('neighbors_kernel', m) for m in (0, 1, 4)} | \
           {('neighbor_obs_kernel',)}
    assert set(kernels) == want
    budget = {('coupling_kernel', 0, 1): 36, ('coupling_kernel', 0, 0): 39, ('coupling_kernel', 1, 1): 50, ('coupling_kernel', 1, 0): 52,
              ('coupling_kernel', 4, 1): 38, ('coupling_kernel', 4, 0): 42, ('neighbors_kernel', 0): 40, ('neighbors_kernel', 1): 24,
              ('neighbors_kernel', 4): 18, ('neighbor_obs_kernel',): 24}
    for key, k in kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == (2048 if key[0] == 'coupling_kernel' else 0), (key, k)
        assert k['vgpr_count'] <= budget[key], (key, k)
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_and_no_lds_crossbar_in_the_graph_kernels(graph_kernels):
    _, asm = graph_kernels
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_graph.hip').read_text()
    assert 'atomic' not in src.split('#include', 1)[1]
    assert not re.search(r'\b(global_atomic|ds_\w*atomic|ds_add|ds_bpermute|ds_permute|scratch_)', asm)
    assert 'row_bcast:31' in asm                                     # the wave-wide maximum is DPP


def test_neighbor_obs_function_surface():
    from gym_d2d_amd import _native
    from gym_d2d_amd import envs
    from gym_d2d_amd.envs import NeighborObsFunction
    from gym_d2d_amd.envs.obs_fn import ArrayObsFunction, OwnLinkObsFunction, RbSensingObsFunction, SignalPlanesObsFunction
    assert 'NeighborObsFunction' in envs.__all__
    fn = NeighborObsFunction()
    assert isinstance(fn, ArrayObsFunction) and fn.native_mode == _native.OBS_NONE and fn.k == 8 and fn.needs_neighbors == 8
    space = fn.get_obs_space(SimpleNamespace(num_rbs=7))
    assert space.shape == (36,) and np.all(space.low == -np.inf) and np.all(space.high == np.inf)

    class K3(NeighborObsFunction):
        k = 3
    assert K3().needs_neighbors == 3 and K3().get_obs_space(SimpleNamespace()).shape == (16,)
    block = object()
    assert fn.compute(SimpleNamespace(neighbor_obs=block)) is block
    for other in (OwnLinkObsFunction, SignalPlanesObsFunction, RbSensingObsFunction):
        assert not other.needs_neighbors
    assert not fn.needs_rb_sensing


def test_k_is_checked_by_name():
    from gym_d2d_amd.graph import check_k
    assert check_k(1, 2) == 1 and check_k(64, 512) == 64 and check_k(np.int64(7), 8) == 7
    for k, n in ((0, 8), (8, 8), (65, 512), (-1, 8), (True, 8), (2.0, 8), ('3', 8), (1, 1)):
        with pytest.raises(ValueError, match=r'k must be an int in 1 \.\. min\(N - 1, 64\)'):
            check_k(k, n)


def test_the_sensing_refusals_kept_their_texts_and_share_one_predicate():
    from gym_d2d_amd import graph, sensing

    def sim(route='native', shadowing=False, pinned=None):
        mask = np.array([pinned is not None])
        xy = np.array([[pinned if pinned is not None else 0.0, 0.0]])
        return SimpleNamespace(path_loss_table=SimpleNamespace(route=route, law={'shadowing': shadowing}),
                               fixed_positions=lambda: (mask, xy))
    assert sensing.refusal(sim(), True) is None and graph.refusal(sim(), True) is None
    for args, kind, word in (((sim(), False), 'export_actions', 'export_actions=False'),
                             ((sim(route='link_table'), True), 'route', "'link_table'"),
                             ((sim(shadowing=True), True), 'shadowing', 'ShadowingPathLoss'),
                             ((sim(pinned=100.1), True), 'pinned', 'float32 cannot hold')):
        assert sensing.unserved(*args)[0] == kind
        assert sensing.refusal(*args).startswith('sense() ') and word in sensing.refusal(*args)
        assert graph.refusal(*args).startswith('the neighbour graph ') and word in graph.refusal(*args)
    assert sensing.refusal(sim(), False) == ('sense() reads the decoded (rb, tx power) planes, which export_actions=False does not '
                                             'write: build the env with export_actions=True')
    assert sensing.refusal(sim(pinned=0.5), True) is None                # float32 holds it


@pytest.mark.parametrize('cues,dues,model,down', [(8, 8, 'ld2', False), (64, 96, 'ld35', False), (24, 40, 'ld2', True), (6, 6, 'suburban', True)])
def test_oracle_ranking_rule_on_the_oracle_alone(cues, dues, model, down):
    """The yardstick's own properties: a stable descending sort without the diagonal, exact ties in ascending j (a downlink base
    station transmits every CUE link), and a left-out share under the cap for k in {1, 8, min(N - 1, 64)}."""
    spec = {'ld2': orc.PathLossSpec('log_distance', 2.1, ple=2.0), 'ld35': orc.PathLossSpec('log_distance', 2.1, ple=3.5),
            'suburban': orc.PathLossSpec('cost_hata', 2.1, area='suburban')}[model]
    rng = np.random.default_rng(cues * 100 + dues)
    pos = random_layout(rng, 2, cues, dues).astype(np.float64)
    tx, rx, _ = default_links(cues, dues)
    if down:
        tx[:cues], rx[:cues] = rx[:cues].copy(), tx[:cues].copy()
    cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    ref = nbu.coupling_ref(pos, tx, rx, cols, spec)
    n = cues + dues
    assert ref.shape == (2, n, n) and np.isfinite(ref).all()
    for k in sorted({1, 8, min(n - 1, 64)}):
        idx, vals, comparable = nbu.ranked(ref, k)
        nbu.check_sets(idx, n)
        assert (np.diff(vals, axis=2) <= 0).all()
        assert np.array_equal(vals, np.take_along_axis(ref, idx, axis=2))
        left_out, ties = nbu.check_indices(idx, ref, k)
        print(f'{model} {cues}+{dues} down={down} k={k}: {left_out:.2%} left out, {ties:.1%} exact ties')
        tie = vals[:, :, :-1] == vals[:, :, 1:]
        assert (idx[:, :, 1:][tie] > idx[:, :, :-1][tie]).all()
        if down and k > 1:
            assert ties > 0.2
    o = nbu.gather_obs(*nbu.ranked(ref, 3)[:2], np.zeros((2, n)), np.ones((2, n)), np.full((2, n), 2.0), np.full((2, n), 3.0))
    assert o.shape == (2, n, 16) and np.array_equal(o[0, 0, :4], [0, 1, 2, 3]) and np.array_equal(o[0, 0, 5:8], [0, 1, 2])

"""Best-response RB selection, the part that needs no GPU: the library's exported set, the entry point's refusals, the kernels'
register budget, the refusal texts, the host-side packing and action encoding, and the oracle's side of the GPU tests' near-tie cap."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import best_rb_util as bru

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_bestrb_library_exports_exactly_its_header():
    from gym_d2d_amd import _native, build
    lib = _native.load_bestrb_library()
    header = (ROOT / 'include' / 'd2d_bestrb.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_bestrb.so') == declared == {'d2d_best_rb', 'd2d_bestrb_last_error'}
    assert set(_native.BESTRB_SIGNATURES) == declared
    assert len(_native.BESTRB_SIGNATURES['d2d_best_rb'][1]) == 19
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('BESTRB_LAW_INV_SQUARE', 'BESTRB_LAW_POWER', 'BESTRB_LAW_POW_K', 'BESTRB_MAX_RBS'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_BESTRB_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    # the law ids and limits are the sensing kernel's: sensing.fold_columns serves both
    assert (_native.BESTRB_LAW_INV_SQUARE, _native.BESTRB_LAW_POWER, _native.BESTRB_LAW_POW_K, _native.BESTRB_MAX_RBS) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K, _native.SENSE_MAX_RBS)
    # built like the other side libraries; the step library keeps its 43 symbols
    assert build.LIBRARIES['bestrb'] == ['d2d_bestrb.hip'] and ROOT / 'include' / 'd2d_bestrb.h' in build.HEADERS
    assert build.lib_path('bestrb') == LIB_DIR / 'libd2d_bestrb.so'
    assert len(_exports('libd2d_hip.so')) == 43 == len(_native.SIGNATURES)
    assert _exports('libd2d_sense.so') == set(_native.SENSE_SIGNATURES)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3)

    def call(ptr=8, best=8, sinr=16, gain=24, **kw):
        a = dict(ok, **kw)
        _native.best_rb(ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                        0, 0, best, sinr, gain)
    before = _native.bestrb_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.BESTRB_MAX_RBS + 1), 'n_rbs'), (dict(law=3), 'law'), (dict(law=-1), 'law'),
                     (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(ptr=0), 'null device pointer'), (dict(best=0), 'null device pointer'),
                     (dict(sinr=0), 'null device pointer'), (dict(gain=0), 'null device pointer'), (dict(sinr=8), 'three planes'),
                     (dict(gain=16), 'three planes'), (dict(gain=8), 'three planes')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.bestrb_launches == before
    call(n_envs=0)                                                      # nothing to do: accepted, and still no launch on a device


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    return SimpleNamespace(path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law={'shadowing': shadowing}),
                           fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))


def test_refusal_texts_name_the_method():
    from gym_d2d_amd import best_response
    assert best_response.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True, False, False]), np.array([[100.1, -20.3], [0, 0], [0, 0]]))
    texts = {'export_actions=True': best_response.refusal(_stub_sim(), False),
             "'link_table'": best_response.refusal(_stub_sim(route='link_table'), True),
             "'per_step'": best_response.refusal(_stub_sim(route='per_step'), True),
             'ShadowingPathLoss': best_response.refusal(_stub_sim(shadowing=True), True),
             'float32 cannot hold': best_response.refusal(pinned, True),
             'torch path': best_response.refusal(_stub_sim(), True, use_torch=False)}
    for needle, text in texts.items():
        assert needle in text and 'best_rb()' in text and 'sense()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)


@pytest.fixture
def stub_handle(monkeypatch):
    from gym_d2d_amd import _native
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    opened = []
    monkeypatch.setattr(_native, 'load_bestrb_library', lambda: opened.append(1) or pytest.fail('libd2d_bestrb.so was opened'))
    return opened


def test_an_env_that_does_not_ask_never_opens_the_library(stub_handle):
    from gym_d2d_amd.envs import BestRbObsFunction, VecD2DEnv
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._bestrb is None and not env._wants_best_rb and stub_handle == []
    # asking on the NumPy path is refused by name, at the call and at construction, still without the library
    with pytest.raises(ValueError, match=r'best_rb\(\) needs the torch path'):
        env.best_rb()
    with pytest.raises(ValueError, match=r'best_rb\(\) needs the torch path'):
        env.best_response_actions()
    with pytest.raises(ValueError, match=r'best_rb\(\) needs the torch path'):
        VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2, 'obs_fn': BestRbObsFunction}, num_envs=2, use_torch=False)
    assert stub_handle == []
    env.close()


def test_obs_function_surface():
    torch = pytest.importorskip('torch')
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import BestRbObsFunction
    from gym_d2d_amd.envs.obs_fn import ArrayObsFunction, LinearObsFunction, OwnLinkObsFunction, RbSensingObsFunction
    fn = BestRbObsFunction()
    assert isinstance(fn, ArrayObsFunction) and fn.needs_best_rb is True and fn.native_mode == _native.OBS_NONE
    assert fn.get_obs_space(SimpleNamespace(num_rbs=9)).shape == (3,)
    view = SimpleNamespace(best_rb=torch.tensor([[2, -1]], dtype=torch.int32), best_sinr_db=torch.tensor([[1.5, float('nan')]]),
                           gain_db=torch.tensor([[0.0, float('nan')]]))
    obs = fn.compute(view)
    assert tuple(obs.shape) == (1, 2, 3) and obs.dtype == torch.float32
    assert obs[0, 0].tolist() == [2.0, 1.5, 0.0] and obs[0, 1, 0] == -1.0 and bool(obs[0, 1, 1:].isnan().all())
    for cls in (LinearObsFunction, OwnLinkObsFunction, RbSensingObsFunction):
        assert not getattr(cls, 'needs_best_rb', False)


@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
def test_best_response_actions_encoding_on_a_stubbed_handle(stub_handle, cue_actions):
    """6 CUEs + 4 pairs on 5 RBs: 24 CUE and 21 DUE power levels.  The planes are hand-made; best_rb() is stubbed."""
    torch = pytest.importorskip('torch')
    from gym_d2d_amd.envs import VecD2DEnv
    b, cues, dues, r = 3, 6, 4, 5
    n = cues + dues
    env = VecD2DEnv({'num_rbs': r, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b, use_torch=False, cue_actions=cue_actions)
    rng = np.random.default_rng(5)
    levels = np.array([24] * cues + [21] * dues)
    rb = rng.integers(0, r, (b, n)); pwr = rng.integers(0, levels, (b, n))
    best = rng.integers(0, r, (b, n)); gain = rng.random((b, n)).astype(np.float32) * 3.0
    gain[rng.random((b, n)) < 0.3] = 0.0
    gain[0, 7], best[0, 7] = np.nan, -1                                 # no allowed RB: stays
    gain[1, 8], rb[1, 8] = np.nan, r + 2                                # on no RB: repeats its (out of range) action
    gain[2, 9] = -1.5                                                   # own RB not allowed and better than every allowed one: stays
    env.device = torch.device('cpu')
    env._t = {'rb': torch.as_tensor(rb, dtype=torch.int32), 'pwr': torch.as_tensor(pwr, dtype=torch.int32)}
    planes = (torch.as_tensor(best, dtype=torch.int32), torch.zeros((b, n)), torch.as_tensor(gain))
    seen = []
    env.best_rb = lambda allowed=None, out=None: seen.append(allowed) or planes
    first = 0 if cue_actions == 'agent' else cues
    for min_gain in (0.0, 1.0):
        a = env.best_response_actions(allowed='mask', min_gain_db=min_gain)
        assert a.dtype == torch.int32 and tuple(a.shape) == (b, env.num_agents) == (b, n - first)
        move = gain > min_gain                                          # NaN compares false
        want = (np.where(move, best, rb) * levels + pwr)[:, first:]
        assert np.array_equal(a.numpy(), want)
        got_rb, got_lvl = np.divmod(a.numpy(), levels[first:])          # the env's own decode (d2d_env.py:94-96)
        assert np.array_equal(got_lvl, pwr[:, first:]) and np.array_equal(got_rb[move[:, first:]], best[:, first:][move[:, first:]])
        assert np.array_equal(got_rb[~move[:, first:]], rb[:, first:][~move[:, first:]])
    assert seen == ['mask', 'mask'] and move.sum() < (gain > 0.0).sum()
    for bad in (-0.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='min_gain_db'):
            env.best_response_actions(min_gain_db=bad)
    # the function behind it takes NumPy planes alike
    from gym_d2d_amd.best_response import encode_actions
    a_np = encode_actions(rb, pwr, best, gain, levels[first:], 0.0, first)
    assert a_np.dtype == np.int32 and np.array_equal(a_np, (np.where(gain > 0.0, best, rb) * levels + pwr)[:, first:])
    env.close()


def test_pack_allowed_bits():
    torch = pytest.importorskip('torch')
    from gym_d2d_amd.best_response import pack_allowed
    rng = np.random.default_rng(0)
    for n, r in ((1, 1), (5, 32), (4, 33), (7, 70)):
        mask = rng.random((n, r)) < 0.5
        mask[0] = True                                                  # bit 31 set: the int32 form wraps
        words = pack_allowed(mask)
        assert words.dtype == np.uint32 and words.shape == (n, (r + 31) // 32)
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(n, -1).astype(bool)
        assert np.array_equal(bits[:, :r], mask) and not bits[:, r:].any()
        wt = pack_allowed(torch.as_tensor(mask), torch)
        assert wt.dtype == torch.int32 and np.array_equal(wt.numpy().view(np.uint32), words)


@pytest.fixture(scope='module')
def bestrb_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_bestrb')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_bestrb.hip'), '-save-temps', '-o', 'bestrb.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'bestrb_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out, asm


def test_bestrb_kernels_use_no_scratch_and_spill_nothing(bestrb_kernels):
    """law in {inverse square 0, power 1, pow-k 4}.  The figures of the build this was written on: 42 VGPRs / 64 SGPRs for the
    inverse-square kernel, 44 / 68 and 44 / 69 for the two power-law ones; LDS is dynamic (see d2d_bestrb.hip)."""
    kernels, _ = bestrb_kernels
    assert set(kernels) == {0, 1, 4}
    for key, k in kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS (no output tile) in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_and_no_output_tile_in_the_bestrb_kernel(bestrb_kernels):
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_bestrb.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code and 'TILE' not in code and 'nontemporal' not in code
    _, asm = bestrb_kernels
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'scratch_' not in asm


@pytest.mark.parametrize('n,r,law', bru.ORACLE_CASES)
def test_oracle_near_ties_of_the_gpu_cases_stay_inside_the_cap(n, r, law):
    """The seeds of the GPU test's oracle comparison, on the oracle alone: at most 1 % of a case's links are near-ties that involve
    an occupied RB (best_rb_util.oracle_side), and the cases do hold exact ties between empty RBs and links on no RB."""
    c = bru.make_case(n, r, law, cell_radius=bru.ORACLE_CELL_M)
    ref, expect, decided = bru.oracle_side(n, r, law)
    assert ref.shape == (c['b'], n, r) and np.isfinite(ref).all()
    left_out = float((~decided).mean())
    empty = ~bru.occupied(c['rb'], r)
    ties = int(((ref == ref.max(axis=-1, keepdims=True)) & empty).sum(axis=-1).__gt__(1).sum())
    print(f'{n} links, {r} RBs, {law}: {left_out:.2%} of {decided.size} links left out as near-ties; {ties} links whose top value is '
          f'an exact tie between empty RBs; {int(c["bad"].sum())} links on no RB')
    assert left_out <= 0.01
    assert c['bad'].any() and (expect >= 0).all() and (expect < r).all()
    if r >= 33:
        assert ties > 0

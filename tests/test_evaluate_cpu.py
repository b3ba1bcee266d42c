"""What-if evaluation of candidate joint actions, the part that needs no GPU: the library's exported set, the entry point's refusals,
the kernels' register budget, the refusal texts, decode_actions against the encoders it inverts, the float64 reference against the
oracle's step, and the reference's side of the GPU tests' threshold cap."""
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import evaluate_util as evu
from oracle import d2d_oracle as orc

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_evaluate_library_exports_exactly_its_header():
    from gym_d2d_amd import _native, build
    lib = _native.load_evaluate_library()
    header = (ROOT / 'include' / 'd2d_evaluate.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_evaluate.so') == declared == {'d2d_evaluate', 'd2d_evaluate_last_error'}
    assert set(_native.EVALUATE_SIGNATURES) == declared
    assert len(_native.EVALUATE_SIGNATURES['d2d_evaluate'][1]) == 19
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('EVALUATE_LAW_INV_SQUARE', 'EVALUATE_LAW_POWER', 'EVALUATE_LAW_POW_K', 'EVALUATE_MAX_RBS', 'EVALUATE_CHUNK',
                  'EVALUATE_MAX_CANDIDATES', 'EVALUATE_MAX_LDS_BYTES'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_EVALUATE_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    assert _native.EVALUATE_MAX_CANDIDATES == 65535 * _native.EVALUATE_CHUNK and _native.EVALUATE_CHUNK == evu.CHUNK
    # the law ids and limits are the sensing kernel's: sensing.fold_columns serves both
    assert (_native.EVALUATE_LAW_INV_SQUARE, _native.EVALUATE_LAW_POWER, _native.EVALUATE_LAW_POW_K, _native.EVALUATE_MAX_RBS) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K, _native.SENSE_MAX_RBS)
    # built like the other side libraries; the step library keeps its 43 symbols
    assert build.LIBRARIES['evaluate'] == ['d2d_evaluate.hip'] and ROOT / 'include' / 'd2d_evaluate.h' in build.HEADERS
    assert build.lib_path('evaluate') == LIB_DIR / 'libd2d_evaluate.so' == _native.side_path('evaluate')
    assert len(_exports('libd2d_hip.so')) == 43 == len(_native.SIGNATURES)
    assert _exports('libd2d_marginal.so') == set(_native.MARGINAL_SIGNATURES)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_cand=3, n_dev=5, n_links=2, n_rbs=3)

    def call(ptr=8, sinr=8, cap=16, total=24, **kw):
        a = dict(ok, **kw)
        _native.evaluate(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_cand'], a['n_dev'],
                         a['n_links'], a['n_rbs'], sinr, cap, total)
    before = _native.evaluate_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.EVALUATE_MAX_RBS + 1), 'n_rbs'), (dict(n_cand=0), 'n_cand'), (dict(n_cand=-4), 'n_cand'),
                     (dict(n_cand=_native.EVALUATE_MAX_CANDIDATES + 1), 'n_cand'), (dict(law=3), 'law'), (dict(law=-1), 'law'),
                     (dict(law=2, pow_k=0), 'pow_k'), (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'),
                     (dict(n_dev=0), 'n_dev'), (dict(ptr=0), 'null device pointer'), (dict(total=0), 'null device pointer'),
                     (dict(sinr=16), 'sinr_db and capacity_mbps must be two planes'),
                     # past the 160 KiB a workgroup can have: refused by name, in bytes
                     (dict(n_links=2048, law=1), 'n_links and n_rbs need 163888 bytes of LDS, more than the 163840'),
                     (dict(n_links=2048, n_rbs=8192), 'n_links and n_rbs need 163888 bytes of LDS'),
                     (dict(n_links=2048, law=1, n_envs=0), 'bytes of LDS')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.evaluate_launches == before
    # nothing to do: accepted with either plane, both or neither absent, and still no launch on a device
    for kw in (dict(), dict(sinr=0), dict(cap=0), dict(sinr=0, cap=0), dict(n_links=2048, n_rbs=7000), dict(n_cand=_native.EVALUATE_MAX_CANDIDATES)):
        call(n_envs=0, **kw)
    assert _native.evaluate_launches == before
    assert evu.lds_bytes(2048, 8192, False) > _native.EVALUATE_MAX_LDS_BYTES >= evu.lds_bytes(2048, 7000, False)
    assert evu.lds_bytes(512, 256, True) < 48 * 1024                   # the benchmark shape fits three times into a CU's LDS


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    return SimpleNamespace(path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law={'shadowing': shadowing}),
                           fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))


def test_refusal_texts_name_the_method():
    from gym_d2d_amd import evaluate
    assert evaluate.refusal(_stub_sim(), True) is None
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True, False, False]), np.array([[100.1, -20.3], [0, 0], [0, 0]]))
    texts = {'export_actions=True': evaluate.refusal(_stub_sim(), False),
             "'link_table'": evaluate.refusal(_stub_sim(route='link_table'), True),
             "'per_step'": evaluate.refusal(_stub_sim(route='per_step'), True),
             'ShadowingPathLoss': evaluate.refusal(_stub_sim(shadowing=True), True),
             'float32 cannot hold': evaluate.refusal(pinned, True),
             'torch path': evaluate.refusal(_stub_sim(), True, use_torch=False)}
    for needle, text in texts.items():
        assert needle in text and 'evaluate()' in text and 'sense()' not in text and 'best_rb()' not in text, (needle, text)
    assert len(set(texts.values())) == len(texts)


def test_an_env_that_does_not_ask_never_opens_the_library(monkeypatch):
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import VecD2DEnv
    from test_host_env_logic import RecordingHandle
    RecordingHandle.instances.clear()
    monkeypatch.setattr(_native, 'Handle', RecordingHandle)
    opened = []
    monkeypatch.setattr(_native, 'load_evaluate_library', lambda: opened.append(1) or pytest.fail('libd2d_evaluate.so was opened'))
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 2}, num_envs=6, use_torch=False)
    env.reset(seed=1)
    env.step(np.zeros((6, 5), dtype=np.int32))
    assert env._evaluate is None and opened == []
    with pytest.raises(ValueError, match=r'evaluate\(\) needs the torch path'):
        env.evaluate(None, None)
    with pytest.raises(ValueError, match=r'evaluate\(\) needs the torch path'):
        env.evaluate_actions(None)
    assert opened == []
    env.close()


@pytest.mark.parametrize('fixed', [0, 6])
def test_decode_actions_inverts_the_encoders(fixed):
    """6 CUEs + 4 pairs on 5 RBs, 24 CUE and 21 DUE power levels; fixed = 6: the CUE links are on fixed actions and have no column."""
    torch = pytest.importorskip('torch')
    from gym_d2d_amd import best_response, power_control
    from gym_d2d_amd.evaluate import decode_actions
    b, k, cues, dues, r = 3, 4, 6, 4, 5
    n = cues + dues
    levels_all = np.array([24] * cues + [21] * dues)
    levels = levels_all[fixed:]
    rng = np.random.default_rng(9 + fixed)
    rb = rng.integers(0, r, (b, k, n)); pwr = rng.integers(0, levels_all, (b, k, n))
    rb[:, :, :fixed], pwr[:, :, :fixed] = rb[:, :1, :fixed], pwr[:, :1, :fixed]                 # fixed links: one state per env
    pwr[0, 0, fixed:], pwr[0, 1, fixed:] = 0, levels - 1                                        # both ends of the alphabet
    # the two encoders, candidate by candidate: best_response's with every link staying, power_control's at the plane's own powers
    stay = np.zeros((b, n), dtype=np.float32)
    a_br = np.stack([best_response.encode_actions(rb[:, q], pwr[:, q], rb[:, q], stay, levels, 0.0, fixed) for q in range(k)], axis=1)
    a_pc = np.stack([power_control.encode_actions(rb[:, q], pwr[:, q], np.zeros_like(levels), levels, fixed) for q in range(k)], axis=1)
    assert a_br.shape == (b, k, n - fixed) and a_br.dtype == np.int32 and np.array_equal(a_br, a_pc)
    fx = (rb[:, 0, :fixed], pwr[:, 0, :fixed]) if fixed else (None, None)
    got_rb, got_pwr = decode_actions(a_br, levels, *fx)
    assert got_rb.dtype == got_pwr.dtype == np.int32 and got_rb.flags.c_contiguous and got_pwr.flags.c_contiguous
    assert np.array_equal(got_rb, rb) and np.array_equal(got_pwr, pwr)
    # torch tensors alike, any integer dtype
    for dt in (torch.int32, torch.int64):
        fxt = tuple(torch.as_tensor(np.ascontiguousarray(f), dtype=torch.int32) for f in fx) if fixed else (None, None)
        t_rb, t_pwr = decode_actions(torch.as_tensor(a_br, dtype=dt), torch.as_tensor(levels, dtype=torch.int32), *fxt)
        assert t_rb.dtype == t_pwr.dtype == torch.int32 and t_rb.is_contiguous() and t_pwr.is_contiguous()
        assert np.array_equal(t_rb.numpy(), rb) and np.array_equal(t_pwr.numpy(), pwr)
    # a negative action decodes with floor semantics, as the step does (d2d_env.py:94-96)
    neg = np.full((1, 1, n - fixed), -1, dtype=np.int32)
    n_rb, n_pwr = decode_actions(neg, levels)
    assert (n_rb == -1).all() and np.array_equal(n_pwr[0, 0], levels - 1)
    t_rb, t_pwr = decode_actions(torch.as_tensor(neg), torch.as_tensor(levels))
    assert np.array_equal(t_rb.numpy(), n_rb) and np.array_equal(t_pwr.numpy(), n_pwr)
    for bad in (a_br[:, 0], a_br[:, :, :-1], a_br.astype(np.float32)):
        with pytest.raises(ValueError, match='actions must be'):
            decode_actions(bad, levels, *fx)


@pytest.fixture(scope='module')
def evaluate_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_evaluate')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_evaluate.hip'), '-save-temps', '-o', 'evaluate.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'evaluate_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out, asm


def test_evaluate_kernels_use_no_scratch_and_spill_nothing(evaluate_kernels):
    """law in {inverse square 0, power 1, pow-k 4}.  The figures of the build this was written on: 36 VGPRs / 71 SGPRs for the
    inverse-square kernel, 40 / 73 and 40 / 81 for the two power-law ones; LDS is dynamic (see d2d_evaluate.hip)."""
    kernels, _ = evaluate_kernels
    assert set(kernels) == {0, 1, 4}
    for key, k in kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_in_the_evaluate_kernel(evaluate_kernels):
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_evaluate.hip').read_text()
    code = src.split('#include', 1)[1]
    assert 'atomic' not in code and 'nontemporal' not in code
    _, asm = evaluate_kernels
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'scratch_' not in asm


@pytest.mark.parametrize('n,r,law,k', [(3, 1, 'ld35', 2), (65, 5, 'ld2', evu.CHUNK + 1)])
def test_reference_agrees_with_the_oracle_step(n, r, law, k):
    """Every candidate as an oracle env of its own on the env's layout: the reference's planes are the oracle's step at 1e-9."""
    c = evu.make_case(n, r, law, k)
    sinr, cap, total, _ = evu.case_ref(n, r, law, k)
    b = c['b']
    pos = np.repeat(np.asarray(c['pos'], dtype=np.float64), k, axis=0)                          # env-major, as rb.reshape below
    res = orc.step(pos, c['tx'], c['rx'], c['rb'].reshape(b * k, n), c['pwr'].reshape(b * k, n), c['ocols'], c['spec'])
    e_s = evu.rel_err(sinr.reshape(b * k, n), res['sinr_db'])
    e_c = evu.rel_err(cap.reshape(b * k, n), res['capacity_mbps'])
    print(f'{n} links, {r} RBs, {law}, K = {k}: sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e} against the oracle')
    assert e_s <= 1e-9 and e_c <= 1e-9
    assert evu.rel_err(total, res['capacity_mbps'].reshape(b, k, n).sum(axis=2)) <= 1e-9
    # the same through the pair path loss of the oracle instead of the law columns
    pl = orc.pair_path_loss_db(c['spec'], np.asarray(c['pos'], dtype=np.float64), np.asarray(c['tx']), np.asarray(c['rx']), c['ocols'])
    s2, c2, _ = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], c['rb'], c['pwr'], {'ocols': c['ocols'], 'pl': pl}, r)
    assert evu.rel_err(s2, sinr) <= 1e-9 and evu.rel_err(c2, cap) <= 1e-9


@pytest.mark.parametrize('n,r,law,k', evu.CASES)
def test_threshold_share_of_the_gpu_cases_stays_inside_the_cap(n, r, law, k):
    """The seeds of the GPU test's comparison, on the reference alone: at most 1 % of a case's links have a reference sinr_db within
    1e-4 dB of their receiver's sensitivity, where the capacity flips between 0 and its whole value."""
    c = evu.make_case(n, r, law, k)
    sinr, cap, total, decided = evu.case_ref(n, r, law, k)
    assert sinr.shape == cap.shape == decided.shape == (evu.B, k, n) and total.shape == (evu.B, k)
    assert np.isfinite(sinr).all() and np.isfinite(cap).all() and c['kind'] == evu.KIND[law]
    left_out = float((~decided).mean())
    print(f'{n} links, {r} RBs, {law}, K = {k}: {left_out:.2%} of {decided.size} links left out at the threshold; '
          f'{(cap > 0).mean():.1%} above it; LDS {evu.lds_bytes(n, r, law != "ld2")} B')
    assert left_out <= evu.THRESHOLD_CAP
    assert (c['pwr'] == evu.P_LOW).any() and (c['pwr'] == evu.P_HIGH).any()
    assert c['pwr'].min() == evu.P_LOW and c['pwr'].max() == evu.P_HIGH


def test_the_cases_cover_the_paths_they_name():
    ks = {k for _, _, _, k in evu.CASES}
    assert {1, 2, evu.CHUNK, evu.CHUNK + 1, 33} <= ks
    assert {law for _, _, law, _ in evu.CASES} == set(evu.KIND)
    big = [evu.lds_bytes(n, r, law != 'ld2') for n, r, law, _ in evu.CASES]
    assert max(big) > 64 * 1024 and sorted(big)[-2] <= 64 * 1024        # exactly one case on the far side of the 64 KiB branch
    assert {n for n, _, _, _ in evu.CASES} >= {1, 3, 63, 65, 257, 260, 300}

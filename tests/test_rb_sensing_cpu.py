"""Per-RB interference sensing, the part that needs no GPU: the library's exported set, the kernels' register budget, the host-side
folding of the columns, and the tie between the GPU tests' yardstick (the oracle-based counterfactual) and the reference."""
import re
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import rb_sensing_util as rbs
from golden_util import rel_err
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_sense_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    lib = _native.load_sense_library()
    header = (ROOT / 'include' / 'd2d_sense.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_sense.so') == declared == {'d2d_sense_rb', 'd2d_sense_last_error'}
    assert set(_native.SENSE_SIGNATURES) == declared
    assert len(_native.SENSE_SIGNATURES['d2d_sense_rb'][1]) == 16
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('SENSE_SINR_DB', 'SENSE_INTERFERENCE_MW', 'SENSE_LAW_INV_SQUARE', 'SENSE_LAW_POWER', 'SENSE_LAW_POW_K', 'SENSE_MAX_RBS'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_SENSE_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS


def test_step_library_still_exports_its_43():
    from gym_d2d_amd import _native
    assert len(_exports('libd2d_hip.so')) == 43 == len(_native.SIGNATURES)


def test_sense_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3, what=0)

    def call(ptr=8, **kw):
        a = dict(ok, **kw)
        _native.sense_rb(ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'], a['n_rbs'],
                         a['what'], ptr)
    before = _native.sense_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.SENSE_MAX_RBS + 1), 'n_rbs'), (dict(what=2), 'what'), (dict(law=3), 'law'),
                     (dict(law=2, pow_k=0), 'pow_k'), (dict(n_envs=-1), 'n_envs'), (dict(ptr=0), 'null device pointer')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.sense_launches == before


@pytest.fixture(scope='module')
def sense_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_sense')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_sense.hip'), '-save-temps', '-o', 'sense.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'sense_kernelILi(\d)ELi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[tuple(int(x) for x in m.groups())] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                                         'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out


def test_sense_kernels_use_no_scratch_and_spill_nothing(sense_kernels):
    """(law in {inverse square 0, power 1, pow-k 4}) x (what in {sinr 0, interference 1}).  The figures of the build this was
    written on: 42 VGPRs for the inverse-square pair, 44 for the four power-law ones; LDS is dynamic (see d2d_sense.hip)."""
    assert set(sense_kernels) == {(m, w) for m in (0, 1, 4) for w in (0, 1)}
    for key, k in sense_kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_floating_point_atomics_in_the_sensing_kernel(sense_kernels, tmp_path_factory):
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_sense.hip').read_text()
    assert 'atomic' not in src.split('#include', 1)[1]


@pytest.mark.parametrize('name', ['rb_sensing_case01', 'rb_sensing_case02'])
def test_oracle_counterfactual_reproduces_the_reference(name):
    """The yardstick of the GPU tests - orc.step on the N * R envs in which one link moved - against the reference's own
    Simulator.step run N * R times (tests/golden/make_rb_sensing_golden.py), and the definition written out in fp64 against both."""
    f = rbs.load_fixture(name)
    r = f['meta']['num_rbs']
    cf = rbs.counterfactual(f['pos'], f['link_tx'], f['link_rx'], f['rb'], f['pwr'], f['cols'], f['spec'], r)
    assert cf.shape == (1,) + f['sinr_db'].shape == (1, 10, 4)
    e = rel_err(cf[0], f['sinr_db'])
    print(name, 'counterfactual vs reference', e)
    assert e <= 1e-9
    ix = rbs.interference_mw(f['pos'], f['link_tx'], f['link_rx'], f['rb'], f['pwr'], f['cols'], f['spec'], r)
    s2 = rbs.sinr_from_interference(f['pos'], f['link_tx'], f['link_rx'], f['pwr'], f['cols'], f['spec'], ix)
    assert rel_err(s2[0], f['sinr_db']) <= 1e-9
    assert rel_err(cf[0][np.arange(10), f['rb'][0]], f['step_sinr_db']) <= 1e-9


def test_oracle_side_of_the_largest_gpu_case_is_quick():
    rng = np.random.default_rng(5)
    cues, dues, r = 64, 96, 24
    pos = random_layout(rng, 2, cues, dues)
    tx, rx, _ = default_links(cues, dues)
    rb = rng.integers(0, r, (2, cues + dues)); pwr = rng.integers(0, 20, (2, cues + dues))
    cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    t0 = time.perf_counter()
    cf = rbs.counterfactual(pos, tx, rx, rb, pwr, cols, orc.PathLossSpec(), r)
    dt = time.perf_counter() - t0
    print(f'oracle counterfactual of 2 x 160 x 24: {dt:.1f} s')
    ix = rbs.interference_mw(pos, tx, rx, rb, pwr, cols, orc.PathLossSpec(), r)
    assert rel_err(rbs.sinr_from_interference(pos, tx, rx, pwr, cols, orc.PathLossSpec(), ix), cf) <= 1e-12
    assert dt < 60


def test_fold_columns_chooses_the_step_s_law():
    from gym_d2d_amd import _native
    from gym_d2d_amd.sensing import fold_columns
    budget = {'eirp_off_db': np.array([1.0, -2.0, 0.5]), 'rx_off_db': np.array([3.0, 0.0, -1.0]), 'noise_dbm': np.full(3, -118.4)}
    tx = np.array([1, 2])

    def law(e):
        return {'a_tx_db': np.array([30.0, 31.0, 32.0]), 'a_rx_db': np.array([0.0, 1.0, -1.0]), 'exponent': np.asarray(e, dtype=np.float64)}
    cols, kind, k = fold_columns(budget, law([2, 2, 2]), tx)
    assert (kind, k) == (_native.SENSE_LAW_INV_SQUARE, 0) and cols.dtype == np.float32 and cols.shape == (6, 3)
    assert np.allclose(cols[0], 10 ** ((budget['eirp_off_db'] - law([2] * 3)['a_tx_db']) / 10), rtol=1e-7)
    assert np.allclose(cols[3], 10 ** (-11.84), rtol=1e-7)
    cols, kind, k = fold_columns(budget, law([2.0, 3.6, 4.375]), tx)         # COST-Hata's slopes: k = 4 by the link transmitters
    assert (kind, k) == (_native.SENSE_LAW_POW_K, 4)
    assert np.allclose(cols[4, 1:], [0.2, -0.1875]) and not cols[5].any()
    cols, kind, k = fold_columns(budget, law([2.0, 2.0, 3.5]), tx)           # 2 and 3.5 share no integer: the general split
    assert kind == _native.SENSE_LAW_POWER
    assert np.array_equal(cols[4].view(np.uint32) & 0xFFF, np.zeros(3, np.uint32))
    assert np.allclose(cols[4].astype(np.float64) + cols[5], [-1.0, -1.0, -1.75], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='float32 linear range'):
        fold_columns(dict(budget, noise_dbm=np.full(3, -400.0)), law([2, 2, 2]), tx)


def test_rb_sensing_obs_function_surface():
    from types import SimpleNamespace
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import RbSensingObsFunction
    from gym_d2d_amd.envs.obs_fn import ArrayObsFunction, OwnLinkObsFunction, SignalPlanesObsFunction
    fn = RbSensingObsFunction()
    assert isinstance(fn, ArrayObsFunction) and fn.native_mode == _native.OBS_NONE and fn.needs_rb_sensing is True
    space = fn.get_obs_space(SimpleNamespace(num_rbs=7))
    assert space.shape == (7,) and np.all(space.low == -np.inf) and np.all(space.high == np.inf)
    block = object()
    assert fn.compute(SimpleNamespace(rb_sinr_db=block)) is block
    assert not OwnLinkObsFunction.needs_rb_sensing and not SignalPlanesObsFunction.needs_rb_sensing

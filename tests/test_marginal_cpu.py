"""Difference rewards, the part that needs no GPU: the library's exported set, the kernels' register budget, the host-side folding,
the reward class's surface, and the tie between the GPU tests' yardstick (marginal_util.leave_one_out) and the reference."""
import re
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

import marginal_util as mu
import rb_sensing_util as rbs
import read_side_util as rsu
from golden_util import load_case, rel_err
from oracle import d2d_oracle as orc
from sim_util import default_links, random_layout

ROOT = Path(__file__).resolve().parent.parent
LIB_DIR = ROOT / 'gym_d2d_amd' / 'lib'


def _exports(lib):
    nm = subprocess.run(['nm', '-D', '--defined-only', str(LIB_DIR / lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}


def test_marginal_library_exports_exactly_its_header():
    from gym_d2d_amd import _native
    lib = _native.load_marginal_library()
    header = (ROOT / 'include' / 'd2d_marginal.h').read_text()
    declared = set(re.findall(r'^(?:int|const char\*) (d2d_\w+)\(', header, flags=re.M))
    assert _exports('libd2d_marginal.so') == declared == {'d2d_marginal_capacity', 'd2d_marginal_last_error'}
    assert set(_native.MARGINAL_SIGNATURES) == declared
    assert len(_native.MARGINAL_SIGNATURES['d2d_marginal_capacity'][1]) == 17
    for name in declared:
        assert getattr(lib, name).restype is not None
    for const in ('MARGINAL_LAW_INV_SQUARE', 'MARGINAL_LAW_POWER', 'MARGINAL_LAW_POW_K', 'MARGINAL_MAX_RBS'):
        assert int(re.search(r'#define D2D_%s (\d+)' % const, header).group(1)) == getattr(_native, const), const
    assert int(re.search(r'#define D2D_MARGINAL_MAX_LINKS (\d+)', header).group(1)) == _native.MAX_LINKS
    # the law ids are the sensing kernel's: sensing.fold_columns serves both
    assert (_native.MARGINAL_LAW_INV_SQUARE, _native.MARGINAL_LAW_POWER, _native.MARGINAL_LAW_POW_K) == \
        (_native.SENSE_LAW_INV_SQUARE, _native.SENSE_LAW_POWER, _native.SENSE_LAW_POW_K)


def test_step_library_still_exports_its_43():
    from gym_d2d_amd import _native
    assert len(_exports('libd2d_hip.so')) == 43 == len(_native.SIGNATURES)
    assert _exports('libd2d_sense.so') == set(_native.SENSE_SIGNATURES)
    assert _exports('libd2d_graph.so') == set(_native.GRAPH_SIGNATURES)


def test_marginal_entry_point_refuses_bad_arguments_without_a_launch():
    from gym_d2d_amd import _native
    ok = dict(law=0, pow_k=0, n_envs=2, n_dev=5, n_links=2, n_rbs=3)

    def call(ptr=8, harm=8, diff=16, **kw):
        a = dict(ok, **kw)
        _native.marginal_capacity(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, a['law'], a['pow_k'], a['n_envs'], a['n_dev'], a['n_links'],
                                  a['n_rbs'], harm, diff)
    before = _native.marginal_launches
    for kw, text in ((dict(n_links=0), 'n_links'), (dict(n_links=_native.MAX_LINKS + 1), 'n_links'), (dict(n_rbs=0), 'n_rbs'),
                     (dict(n_rbs=_native.MARGINAL_MAX_RBS + 1), 'n_rbs'), (dict(law=3), 'law'), (dict(law=2, pow_k=0), 'pow_k'),
                     (dict(law=2, pow_k=9), 'pow_k'), (dict(n_envs=-1), 'n_envs'), (dict(n_dev=0), 'n_dev'),
                     (dict(ptr=0), 'null device pointer'), (dict(harm=0), 'null device pointer'), (dict(diff=0), 'null device pointer'),
                     (dict(harm=16), 'two planes'), (dict(n_links=2048, n_rbs=8192), '160 KiB')):
        with pytest.raises(_native.NativeError, match=text):
            call(**kw)
    assert _native.marginal_launches == before


@pytest.fixture(scope='module')
def marginal_kernels(tmp_path_factory):
    from gym_d2d_amd import build
    tmp = tmp_path_factory.mktemp('isa_marginal')
    cmd = [build._hipcc(), *build.FLAGS, '-I', str(build.INCLUDE), '-c', str(build.CSRC / 'd2d_marginal.hip'), '-save-temps', '-o', 'marginal.o']
    r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = next(tmp.glob('*gfx950*.s')).read_text()
    out = {}
    for blk in re.split(r'\n  - ', asm[asm.find('amdhsa.kernels'):]):
        name = re.search(r'\.name:\s+(\S+)', blk)
        m = name and re.search(r'marginal_kernelILi(\d)EE', name.group(1))
        if not m:
            continue
        field = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        out[int(m.group(1))] = {k: field(k) for k in ('vgpr_count', 'sgpr_count', 'sgpr_spill_count', 'vgpr_spill_count',
                                                      'private_segment_fixed_size', 'group_segment_fixed_size')}
    return out, asm


def test_marginal_kernels_use_no_scratch_and_spill_nothing(marginal_kernels):
    """law in {inverse square 0, power 1, pow-k 4}.  The figures of the build this was written on: 42 VGPRs for the inverse-square
    kernel, 44 for the two power-law ones; LDS is dynamic (see d2d_marginal.hip)."""
    kernels, _ = marginal_kernels
    assert set(kernels) == {0, 1, 4}
    for key, k in kernels.items():
        print(key, k)
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0, (key, k)
        assert k['group_segment_fixed_size'] == 0, (key, k)          # no static LDS in front of the dynamic block
        assert k['vgpr_count'] <= 64, (key, k)                       # eight waves per SIMD stay possible


def test_no_atomics_in_the_marginal_kernel(marginal_kernels):
    src = (ROOT / 'gym_d2d_amd' / 'csrc' / 'd2d_marginal.hip').read_text()
    assert 'atomic' not in src.split('#include', 1)[1]
    _, asm = marginal_kernels
    assert not re.search(r'^\s*(global|flat|buffer|ds)_(atomic|add_f|add_rtn|cmpst)', asm, flags=re.M)
    assert 'scratch_' not in asm


@pytest.mark.parametrize('name', ['marginal_case01', 'marginal_case02'])
def test_oracle_leave_one_out_reproduces_the_reference(name):
    """The yardstick of the GPU tests - ONE orc.step on the N envs in which link i sits on a pseudo-RB of its own - against the
    reference's own Simulator.step run with link i's entry removed (tests/golden/make_marginal_golden.py)."""
    f = mu.load_fixture(name)
    r = f['meta']['num_rbs']
    diff, harm, cap, g_without = mu.leave_one_out(f['pos'], f['link_tx'], f['link_rx'], f['rb'], f['pwr'], f['cols'], f['spec'], r)
    assert diff.shape == harm.shape == (1, 10)
    e_cap, e_g = rel_err(cap[0], f['capacity_mbps']), rel_err(g_without[0], f['g_without'])
    ref_harm = f['g_without'] - (f['capacity_mbps'].sum() - f['capacity_mbps'])
    e_harm, e_diff = rel_err(harm[0], ref_harm), rel_err(diff[0], f['capacity_mbps'] - ref_harm)
    print(name, 'capacity', e_cap, 'g_without', e_g, 'harm', e_harm, 'difference', e_diff)
    assert max(e_cap, e_g, e_harm, e_diff) <= 1e-9
    assert (ref_harm > 1e-3).sum() >= 4 and (harm >= -1e-12).all()     # the fixtures do exercise the term


def test_oracle_leave_one_out_equals_the_step_on_the_shortened_link_list():
    rng = np.random.default_rng(3)
    cues, dues, r = 5, 7, 3
    n = cues + dues
    pos = random_layout(rng, 2, cues, dues)
    tx, rx, _ = default_links(cues, dues)
    rb = rng.integers(0, r, (2, n)); pwr = rng.integers(0, 20, (2, n))
    rb[0, 4] = -3; rb[1, 2] = r + 2                                    # on no RB
    cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    diff, harm, cap, g_without = mu.leave_one_out(pos, tx, rx, rb, pwr, cols, orc.PathLossSpec(), r)
    # (the yardstick's harm is a difference of two sums: zero up to their rounding)
    assert abs(harm[0, 4]) <= 1e-12 and abs(harm[1, 2]) <= 1e-12 and abs(diff[0, 4] - cap[0, 4]) <= 1e-12
    live = rb.copy(); live[0, 4] = r + 50; live[1, 2] = r + 51
    for i in range(n):
        keep = np.arange(n) != i
        rest = orc.step(pos, tx[keep], rx[keep], live[:, keep], pwr[:, keep], cols, orc.PathLossSpec())['capacity_mbps']
        assert np.abs(rest.sum(axis=1) - g_without[:, i]).max() <= 1e-12


def test_oracle_side_of_the_largest_gpu_case_is_quick():
    """8 envs of the full-size case: 8 x 512 links on 256 RBs."""
    rng = np.random.default_rng(5)
    cues, dues, r = 256, 256, 256
    pos = random_layout(rng, 8, cues, dues)
    tx, rx, _ = default_links(cues, dues)
    rb = rng.integers(0, r, (8, cues + dues)); pwr = rng.integers(0, 20, (8, cues + dues))
    cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
    t0 = time.perf_counter()
    diff, harm, cap, _ = mu.leave_one_out(pos, tx, rx, rb, pwr, cols, orc.PathLossSpec(), r)
    dt = time.perf_counter() - t0
    print(f'oracle leave-one-out of 8 x 512 links: {dt:.1f} s; negative difference for {(diff < 0).mean():.1%} of the links')
    assert np.isfinite(diff).all() and (harm >= -1e-9).all()
    assert dt < 60


def _rebuilt_state(name):
    """The state test_gpu_marginal.py's _build(name) reaches, rebuilt by the env's rules without a GPU: the same generator, layout
    and raw actions, decoded as the env decodes them (rb = a // P, level = a % P with 24 CUE and 21 DUE levels, d2d_env.py:93-96); under
    cue_actions='traffic' the CUEs sit on the traffic model's round-robin RBs at their maximum power, and under
    DownlinkTrafficModel their links run from the base station to the CUE.  case07 pins devices and keeps the layout its reset drew
    on the device around them: here it stands on the fixture's recorded layout instead (one env)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    cases = dict(rbs.CASES, one_rb=(2, 20, 30, 1, 'ld2', 'agent', False))
    if cases[name] is None:
        case = load_case(name)
        b0, cue_actions, down = 1, 'agent', False
        cues, dues, r = case.meta['num_cues'], case.meta['num_due_pairs'], case.meta['num_rbs']
        from sim_util import oracle_spec
        spec, cols, pos = oracle_spec(case), orc.device_columns(case.cfgs, case.is_bs), np.asarray(case.pos, dtype=np.float64)[None]
    else:
        b0, cues, dues, r, model, cue_actions, down = cases[name]
        spec = rbs._models()[model][1]
        cols = orc.device_columns(*orc.device_configs(cues, dues)[1:])
        pos = random_layout(rng, b0, cues, dues).astype(np.float64)
    tx, rx, _ = default_links(cues, dues)
    if down:
        tx[:cues], rx[:cues] = 0, np.arange(1, 1 + cues)
    levels = np.array(([24] * cues if cue_actions == 'agent' else []) + [21] * dues)
    raw = rng.integers(0, r * levels, (b0, len(levels)))
    rb, pwr = raw // levels, raw % levels
    if cue_actions == 'traffic':
        rb = np.concatenate([np.broadcast_to(np.arange(cues) % r, (b0, cues)), rb], axis=1)
        pwr = np.concatenate([np.full((b0, cues), 23), pwr], axis=1)
    return dict(b=b0, n=cues + dues, r=r, pos=pos, tx=tx, rx=rx, rb=rb, pwr=pwr, ocols=cols, spec=spec)


@pytest.mark.parametrize('name', list(rbs.CASES) + ['one_rb'])
def test_no_link_of_the_small_gpu_cases_sits_on_a_sensitivity_threshold(name):
    """test_gpu_marginal.py compares every entry.  That needs every link decided: no SINR - the link's own, or a victim's on its RB
    with or without the link - within twice the bar of the receiver's sensitivity (read_side_util.leave_one_out_direct).  On the
    float64 reference alone; the GPU test asserts the same on the state it really reached."""
    c = _rebuilt_state(name)
    pl = orc.pair_path_loss_db(c['spec'], c['pos'], c['tx'], c['rx'], c['ocols'])
    diff, harm, cap, decided = rsu.leave_one_out_direct(c, pl=pl)
    ref_diff, ref_harm, ref_cap, _ = mu.leave_one_out(c['pos'], c['tx'], c['rx'], c['rb'], c['pwr'], c['ocols'], c['spec'], c['r'])
    sinr = orc.step(c['pos'], c['tx'], c['rx'], c['rb'], c['pwr'], c['ocols'], c['spec'])['sinr_db']
    room = np.abs(sinr - c['ocols'].sens_dbm[c['rx']][None, :]).min()
    print(f'{name}: {(~decided).mean():.2%} of {decided.size} links undecided; the nearest SINR is {room:.1f} dB from its threshold')
    assert max(rel_err(harm, ref_harm), rel_err(diff, ref_diff), rel_err(cap, ref_cap)) <= 1e-9
    assert decided.all()


def test_fold_capacity_columns_follows_the_step_s_records():
    from gym_d2d_amd.marginal import fold_capacity_columns
    budget = {'bw_hz': np.array([180000.0, 360000.0, 1.0e7 / 3]), 'sens_dbm': np.array([-107.5, -6.0, 0.1])}
    cols = fold_capacity_columns(budget)
    assert cols.dtype == np.float32 and cols.shape == (2, 3)
    assert np.array_equal(cols[0], (1e-6 * budget['bw_hz']).astype(np.float32))       # one rounding, of the double product
    assert np.array_equal(cols[1], budget['sens_dbm'].astype(np.float32))


def test_difference_reward_function_surface():
    from types import SimpleNamespace
    from gym_d2d_amd import _native
    from gym_d2d_amd.envs import DifferenceRewardFunction
    from gym_d2d_amd.envs.reward_fn import (CueSinrShannonRewardFunction, RewardFunction, ShannonRewardFunction,
                                            SystemCapacityRewardFunction)
    fn = DifferenceRewardFunction()
    assert isinstance(fn, RewardFunction) and fn.native_id == _native.REWARD_NONE and fn.needs_marginal is True
    plane = object()
    assert fn.compute(SimpleNamespace(difference_mbps=plane, harm_mbps=None)) is plane
    with pytest.raises(RuntimeError, match='VecD2DEnv'):
        fn({}, {})
    for cls in (SystemCapacityRewardFunction, ShannonRewardFunction, CueSinrShannonRewardFunction):
        assert not getattr(cls, 'needs_marginal', False)


def test_refusal_texts_name_the_method():
    from types import SimpleNamespace
    from gym_d2d_amd import marginal
    from gym_d2d_amd.path_loss_table import NATIVE

    def sim(route=NATIVE, shadowing=False):
        return SimpleNamespace(path_loss_table=SimpleNamespace(route=route, law={'shadowing': shadowing}),
                               fixed_positions=lambda: (np.zeros(3, bool), np.zeros((3, 2))))
    assert marginal.refusal(sim(), True) is None
    assert 'export_actions=True' in marginal.refusal(sim(), False) and 'marginal_capacity()' in marginal.refusal(sim(), False)
    assert "'link_table'" in marginal.refusal(sim(route='link_table'), True)
    assert 'ShadowingPathLoss' in marginal.refusal(sim(shadowing=True), True)

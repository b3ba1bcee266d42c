"""What test_gpu_table_route.py stands on, without a GPU (tests/table_route_util.py): every case's plan names the kernel, launch shape and
walk the case table says; the cases together name every step_kernel<2,...> and step_kernel<5,...> of the gfx950 code object of
d2d_step.hip, so a new instantiation without a case fails here; the float64 reference on a link table equals oracle.d2d_oracle.step on
the device table it was gathered from; and the synthetic inputs have, on the reference alone, the properties the GPU tests rely on."""
import re

import numpy as np
import pytest

import table_route_util as tr
from oracle import d2d_oracle as orc
from step_plan_util import build_step_plan, kernel_names, mangled

MODES = (2, 5)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    return build_step_plan(tmp_path_factory.mktemp('plan'))


def test_every_case_is_planned_as_the_table_says(plan):
    for m in MODES:
        got = plan([c.plan_inputs(m) for c in tr.CASES])
        assert len(got) == len(tr.CASES)
        for c, p in zip(tr.CASES, got):
            assert p.get('kernel') == c.kernel.format(m=m), (c.name, m, p)
            assert tuple(p[k] for k in ('lpt', 'tpe', 'epw', 'mask_words', 'walk')) == c.geometry, (c.name, m, p)
            assert p['grid'] == -(-c.b // p['epw']) and p['block'] == p['tpe'] * p['epw'], (c.name, m, p)


def test_the_plans_the_issue_quotes(plan):
    """The LDS bytes and blocks of the rows whose plan is quoted with the case table."""
    quoted = {'n50_lists': (256, 6528), 'n64_full': (64, None), 'n130_lpt2': (256, None), 'n1100_sweep': (576, 22080),
              'n1100_lists': (576, 28096), 'n2100_strided': (1024, 58880)}
    for name, (block, lds) in quoted.items():
        c = tr.BY_NAME[name]
        inputs = c.plan_inputs(2).replace(f' n_fixed={tr.N_FIXED}', '').replace(' action_mode=1', '')
        p, = plan([inputs])
        assert p['block'] == block and (lds is None or p['lds'] == lds), (name, p)


def test_the_cases_cover_every_table_kernel_of_the_code_object(tmp_path):
    names = kernel_names(tmp_path, 'd2d_step.hip')
    built = {k for k in names if re.match(r'_ZN3d2d11step_kernelILi[25]E', k)}
    planned = {mangled(c.kernel.format(m=m)) for c in tr.CASES for m in MODES}
    assert built == planned, (sorted(built - planned), sorted(planned - built))
    assert len(built) == 36
    launched = {mangled(c.kernel.format(m=m)) for c in tr.GPU_CASES for m in MODES}
    assert launched == built            # the case that is planned only (more links than the library takes) leaves no kernel out


@pytest.mark.parametrize('name', ['n50_masks', 'n130_lpt2'])
def test_reference_equals_the_oracle_on_a_gathered_device_table(name):
    c = tr.BY_NAME[name]
    a, (tx, rx, _), cols = tr.actions(c), tr.links(c), tr.columns(c)
    pos = np.zeros((c.b, c.d, 2))
    for shared in (False, True):
        dev = tr.devices(c, shared)
        for rb in (a.rb, np.arange(c.n)[None].repeat(c.b, 0)):           # with interferers, and every link alone on its RB
            want = orc.step(pos, tx, rx, rb, a.pwr, cols, orc.PathLossSpec('table', table_db=dev))
            link = tr.gather(c, dev)
            got = tr.table_step_ref(link if link.ndim == 3 else link[None], None, rb, a.pwr, cols, tx, rx)
            for k, w in want.items():
                assert np.isfinite(w).all() and tr.rel_err(got[k], w) <= 1e-12, (name, shared, k)


def test_the_snr_row_moves_snr_db_and_nothing_else():
    c = tr.BY_NAME['n50_masks']
    inp = tr.inputs(c.name)
    moved = tr.reference(c, inp.pairs, inp.snr)
    for k, v in inp.ref_pairs.items():
        assert np.array_equal(v, moved[k]) == (k != 'snr_db'), k
    diag = np.diagonal(inp.pairs, axis1=1, axis2=2)
    assert np.allclose(moved['snr_db'] - inp.ref_pairs['snr_db'], diag - inp.snr, rtol=0, atol=1e-9)


@pytest.mark.parametrize('name', [c.name for c in tr.CASES])
def test_the_inputs_put_every_case_where_the_gpu_tests_need_it(name):
    c = tr.BY_NAME[name]
    a, (tx, rx, ty) = tr.actions(c), tr.links(c)
    overflow, oor = tr.special_envs(c)
    # actions: the overflow env has more than LIST_SLOTS links on an RB and no other env of a list case has; the out-of-range env
    # has rb == R and rb < 0 and no other env has
    most = np.array([np.bincount(a.rb[e][(a.rb[e] >= 0) & (a.rb[e] < c.rbs)], minlength=c.rbs).max() for e in range(c.b)])
    if c.lists:
        assert most[overflow] >= 12 and (np.delete(most, overflow) <= tr.LIST_SLOTS).all(), most
    out = (a.rb < 0) | (a.rb >= c.rbs)
    assert out[oor, tr.OOR_CUE] and a.rb[oor, tr.OOR_CUE] == c.rbs and a.rb[oor, c.cues + tr.OOR_DUE] == -1 and out.sum() == 2
    assert ((a.pwr >= 0) & (a.pwr < a.levels[None])).all()
    assert a.raw.shape == (c.b, c.n - (tr.N_FIXED if c.stepping == 'fixed' else 0))
    for shared in (False, True):
        t = tr.pairs(c, shared)
        t = t if t.ndim == 3 else t[None]
        ref = tr.reference(c, t, None if shared else tr.snr_row(c))
        sens = ref['sens'][None]
        for e in range(c.b):
            assert (ref['sinr_db'][e] > sens[0] + 1.0).any() and (ref['sinr_db'][e] < sens[0] - 1.0).any(), (shared, e)
        assert ref['near'].sum() <= 0.01 * c.b * c.n
        if c.reward == 1:                   # envs with and without the -1 rule, as the actions lay them out
            want = np.where(np.arange(c.b) % 2 == 1, -1.0, ref['reward'][:, 0])
            assert np.array_equal(ref['reward'][:, 0], want) and (ref['reward'][::2, 0] > 0).all()
        else:
            assert (ref['reward'] == -1.0).any() and (ref['reward'] > 0).any()
        assert np.isfinite(ref['sinr_db']).all() and np.isfinite(ref['snr_db']).all()
        for e in range(t.shape[0]):
            fin = t[e][np.isfinite(t[e])]
            assert len(np.unique(fin)) == len(fin) and np.isposinf(t[e]).sum() == tr.N_INF and not np.isinf(np.diagonal(t[e])).any()
            off = t[e][~np.eye(c.n, dtype=bool)]
            assert np.diagonal(t[e]).min() < off.min() and np.diagonal(t[e]).max() < off[np.isfinite(off)].max()
            # not derivable from a device table (two CUE columns of a row would be equal: both are received by device 0) and not symmetric
            assert (t[e][:, 0] != t[e][:, 1]).all() and ((t[e] != t[e].T) | np.isinf(t[e]))[~np.eye(c.n, dtype=bool)].all()
    if 'R1' in c.routes:
        for shared in (False, True):
            dev = tr.devices(c, shared)
            read = np.zeros((c.d, c.d), dtype=bool)
            read[np.ix_(tx, rx)] = True
            assert np.isnan(dev[..., ~read]).all() and np.isfinite(dev[..., read]).all()
            fin = dev[..., read].reshape(-1 if shared else c.b, read.sum())
            assert all(len(np.unique(row)) == len(row) for row in fin.reshape(-1, read.sum()))
    if c.xpos:
        pos = tr.positions(c)
        assert pos.dtype == np.float64 and (pos[:, 1:] != pos[:, 1:].astype(np.float32)).all()

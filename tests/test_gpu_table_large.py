"""The table read-side kernels near their stated limits on the GPU: csrc/d2d_evaltab.hip and csrc/d2d_tabmarg.hip by direct launch
at 2048 links, 8192 RBs and past 64 KiB of dynamic LDS (table_large_util.CASES; test_table_large_cpu.py asserts on the reference
alone what each case reaches).

Every output lies between guard bands over sentinels and is read behind a synchronize.  sinr_db, capacity_mbps, harm_mbps and
difference_mbps hold the project's bar |d| <= 1e-5 max(|ref|, 1) against the group-wise float64 references on the decided links;
total_mbps is table_evaluate_util.totals_in_order of the kernel's own capacity plane, difference is evaltab's capacity - harm as
float32, harm is 0.0 for a link alone or on no RB, a second launch gives the same words - all bit for bit - and domain is 0.  One
planted check per kernel in the 2048-link live layout: a NaN in an entry [j, i], j, i >= 1024, raises the flag of exactly the
candidates (the env) in which the two links share an RB, the same NaN between links on different RBs raises none, and row N, NaN
throughout, is never read.

Which case launches which instantiation past 64 KiB (launch() of csrc/d2d_addon.h sets the dynamic-LDS attribute per function):
  evaltab_kernel<double>  (2048, 8192) 106 560 B, (2047, 3) 73 776 B      evaltab_kernel<float>  (2048, 64) 74 048 B
  tabmarg_kernel<double>  (2048, 8192) 122 912 B, (2047, 3) 90 128 B      tabmarg_kernel<float>  (2048, 64) 90 400 B

Every test prints the worst error it measured.  Measured on an MI355X, in the order of table_large_util.CASES: evaltab sinr_db
rel_err 1.1e-6, 9.8e-7, 8.5e-7, 1.4e-6 and capacity_mbps 2.5e-7, 2.2e-7, 2.0e-7, 2.6e-7; tabmarg harm_mbps 9.9e-8, 1.2e-7, 2.2e-8,
1.1e-7 and difference_mbps 4.6e-7, 4.3e-7, 2.0e-7, 5.5e-7; no link left out at the threshold."""
import numpy as np
import pytest

import table_evaluate_util as teu
import table_large_util as tlu
import table_marginal_util as tmu
from guard_util import Guarded, bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

_device = {}


def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inputs(c):
    """The device tensors of a case that no launch changes - the table and the four constant arrays - uploaded once per module."""
    key = id(c['table'])
    if key not in _device:
        _device[key] = (torch.as_tensor(np.array(c['table']), device='cuda'),
                        [torch.as_tensor(np.array(c[name]), device='cuda') for name in ('tx', 'rx', 'cols', 'cap_cols')])
    return _device[key]


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    _device.clear()


def _evaltab(c, rb=None, pwr=None, table=None):
    """One d2d_evaluate_table launch, every output between guard bands: (sinr_db, capacity_mbps, total_mbps, domain) on the host."""
    from gym_d2d_amd import _native
    rb, pwr = c['rb'] if rb is None else rb, c['pwr'] if pwr is None else pwr
    tab, consts = _inputs(c)
    tab = tab if table is None else table
    b, k, n = rb.shape
    assert tuple(tab.shape) == (b, c['rows'], n) and tab.is_contiguous()
    rb_t, pwr_t = (torch.as_tensor(np.array(a, dtype=np.int32), device='cuda') for a in (rb, pwr))
    outs = (Guarded((b, k, n), torch.float32), Guarded((b, k, n), torch.float32), Guarded((b, k), torch.float32), Guarded((b, k), torch.int32))
    launches = _native.evaltab_launches
    _native.evaluate_table(tab.data_ptr(), _native.EVALTAB_F64 if tab.dtype == torch.float64 else _native.EVALTAB_F32, c['rows'],
                           rb_t.data_ptr(), pwr_t.data_ptr(), *(t.data_ptr() for t in consts), b, k, c['d'], n, c['r'],
                           *(g.array.data_ptr() for g in outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.evaltab_launches == launches + 1
    assert all(g.intact() for g in outs)
    return tuple(g.array.cpu().numpy() for g in outs)


def _tabmarg(c, table=None):
    """One d2d_table_marginal launch, every output between guard bands: (difference, harm, domain) on the host."""
    from gym_d2d_amd import _native
    tab, consts = _inputs(c)
    tab = tab if table is None else table
    b, n = c['rb'].shape
    assert tuple(tab.shape) == (b, c['rows'], n) and tab.is_contiguous()
    rb_t, pwr_t = (torch.as_tensor(np.array(a, dtype=np.int32), device='cuda') for a in (c['rb'], c['pwr']))
    g_d, g_h, g_f = Guarded((b, n), torch.float32), Guarded((b, n), torch.float32), Guarded((b,), torch.int32)
    launches = _native.tabmarg_launches
    _native.table_marginal(tab.data_ptr(), _native.TABMARG_F64 if tab.dtype == torch.float64 else _native.TABMARG_F32, c['rows'],
                           rb_t.data_ptr(), pwr_t.data_ptr(), *(t.data_ptr() for t in consts), b, c['d'], n, c['r'],
                           g_h.array.data_ptr(), g_d.array.data_ptr(), g_f.array.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.tabmarg_launches == launches + 1
    assert g_d.intact() and g_h.intact() and g_f.intact()
    return tuple(g.array.cpu().numpy() for g in (g_d, g_h, g_f))


def _same(a, m):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, m))


# ------------------------------------------------------------------------------------------ 1: evaltab
@pytest.mark.parametrize('case', tlu.CASES)
def test_evaltab_at_the_limits_against_the_groupwise_float64_reference(case):
    n, r, k, b, dtype, extra = case
    c = tlu.make_case(*case)
    ref_sinr, ref_cap, _, decided = tlu.evaluate_case_ref(*case)
    sinr, cap, total, domain = _evaltab(c)
    e_s, e_c = teu.evu.rel_err(sinr, ref_sinr), teu.evu.rel_err(cap[decided], ref_cap[decided])
    left_out = float((~decided).mean())
    print(f'evaltab {n} links, {r} RBs, K = {k}, B = {b}, {dtype} [{n + extra} rows]: sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e}; '
          f'{left_out:.2%} left out at the threshold; LDS {teu.lds_bytes(n, r)} B')
    assert (teu.lds_bytes(n, r) > tlu.LDS_64K) == (case in tlu.PAST_64K)
    assert np.isfinite(sinr).all() and np.isfinite(cap).all() and np.isfinite(total).all()
    assert (domain == 0).all()
    assert left_out <= tlu.THRESHOLD_CAP
    assert e_s <= tlu.BAR
    assert e_c <= tlu.BAR
    assert (cap > 0).sum() >= 64
    assert np.array_equal(_f32_bits(total), _f32_bits(teu.totals_in_order(cap, c['rb'], r)))
    assert _same(_evaltab(c), (sinr, cap, total, domain))


# ------------------------------------------------------------------------------------------ 2: tabmarg
@pytest.mark.parametrize('case', tlu.CASES)
def test_tabmarg_at_the_limits_against_the_groupwise_float64_leave_one_out(case):
    n, r, k, b, dtype, extra = case
    c, ref = tlu.make_marginal_case(*case), tlu.marginal_case_ref(*case)
    diff, harm, domain = _tabmarg(c)
    keep = ref['decided']
    left_out = float((~keep).mean())
    e_h, e_d = teu.evu.rel_err(harm[keep], ref['harm'][keep]), teu.evu.rel_err(diff[keep], ref['difference'][keep])
    print(f'tabmarg {n} links, {r} RBs, B = {b}, {dtype} [{n + extra} rows]: harm rel_err {e_h:.3e}, difference rel_err {e_d:.3e}; '
          f'{left_out:.2%} left out at the threshold; LDS {tmu.lds_bytes(n, r)} B')
    assert (tmu.lds_bytes(n, r) > tlu.LDS_64K) == (case in tlu.PAST_64K)
    assert np.isfinite(diff).all() and np.isfinite(harm).all() and (domain == 0).all()
    assert left_out <= tlu.THRESHOLD_CAP
    assert e_h <= tlu.BAR
    assert e_d <= tlu.BAR
    # bit for bit: the capacity is evaltab's on candidate 0's planes, the difference the float subtraction; harm exactly 0 alone
    full = tlu.make_case(*case)
    _, cap, _, dom = _evaltab(full, full['rb'][:, :1], full['pwr'][:, :1])
    cap = cap[:, 0]
    assert (dom == 0).all() and np.array_equal(_f32_bits(diff), _f32_bits(cap - harm))
    assert (harm >= 0).all() and (harm > 0).sum() >= 64
    off = (c['rb'] < 0) | (c['rb'] >= r)
    alone = off.copy()
    for e in range(b):
        sizes = tlu.group_sizes(c['rb'][e], r)
        alone[e, ~off[e]] = sizes[c['rb'][e][~off[e]]] == 1
    assert off.any() and (alone & ~off).any() == (r >= 257)             # (64 and 3 RBs leave no link alone on one)
    assert (_f32_bits(harm[alone]) == 0).all() and np.array_equal(_f32_bits(diff[alone]), _f32_bits(cap[alone]))
    assert _same(_tabmarg(c), (diff, harm, domain))


# ------------------------------------------------------------------------------------------ 3: the planted entries at 2048 links
def _with_nan(c, j, i):
    """A clone of the case's device table with entry [0, j, i] NaN."""
    tab = _inputs(c)[0].clone()
    tab[0, j, i] = float('nan')
    return tab


def test_evaltab_raises_the_flag_for_exactly_the_candidates_that_read_a_nan_past_link_1024():
    c = tlu.make_case(*tlu.PLANT)
    n, k = c['n'], c['k']
    base = _evaltab(c)
    assert c['rows'] == n + 1 and bool(torch.isnan(_inputs(c)[0][:, n]).all()) and (base[3] == 0).all()       # row N: never read
    j, i, readers = tlu.planted(c, True)
    got = _evaltab(c, table=_with_nan(c, j, i))
    print(f'evaltab: NaN at [{j}, {i}], read by candidates {np.flatnonzero(readers).tolist()}: domain {got[3][0].tolist()}')
    assert min(j, i) >= 1024 and 1 <= readers.sum() < k and np.array_equal(got[3][0] != 0, readers)
    for a, m in zip(got[:3], base[:3]):                                  # the other candidates: the same words
        assert np.array_equal(bits(a[0, ~readers]), bits(m[0, ~readers]))
    j, i, readers = tlu.planted(c, False)
    got = _evaltab(c, table=_with_nan(c, j, i))
    print(f'evaltab: NaN at [{j}, {i}], read by nobody: domain {got[3][0].tolist()}')
    assert min(j, i) >= 1024 and not readers.any() and _same(got, base)


def test_tabmarg_raises_the_flag_where_a_nan_past_link_1024_is_read_and_only_there():
    c = tlu.make_marginal_case(*tlu.PLANT)
    n = c['n']
    base = _tabmarg(c)
    assert c['rows'] == n + 1 and bool(torch.isnan(_inputs(c)[0][:, n]).all()) and (base[2] == 0).all()       # row N: never read
    j, i, readers = tlu.planted(c, True)
    got = _tabmarg(c, table=_with_nan(c, j, i))
    print(f'tabmarg: NaN at [{j}, {i}], links on one RB: domain {got[2].tolist()}')
    assert min(j, i) >= 1024 and readers.all() and got[2].tolist() == [1]
    j, i, readers = tlu.planted(c, False)
    got = _tabmarg(c, table=_with_nan(c, j, i))
    print(f'tabmarg: NaN at [{j}, {i}], links on different RBs: domain {got[2].tolist()}')
    assert min(j, i) >= 1024 and not readers.any() and _same(got, base)

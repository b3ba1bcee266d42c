"""The host side of the deviation kernels' large cases (deviation_large_util.py; test_gpu_deviation_large.py launches them).

1. The LDS figures, by deviation_util.lds_bytes and deviation.lds_bytes, and what each case claims to reach, on the case states alone.
2. The restricted oracle equals the full deviation_util.by_oracle on the existing d40_r2 and d50_r25: `near` and `open` equal, `gain`
   to 1e-12 max(|ref|, 1) - float64 on the same operands, only the order of at most 50 terms apart.
3. The float64 side of the large cases: the near-threshold marks stay under deviation_util.MARK_CAP, on the reference alone.
4. The refusals, which need no device: the largest N the formula admits on one RB is accepted and N + 1 refused by the byte count,
   2048 links are refused on every RB count, d1950_r8 with an allowed mask is refused - by the library's entry points with no env to
   launch for, and by the host class on a stub sim before the library is opened.

Every test prints what it measured."""
from types import SimpleNamespace

import numpy as np
import pytest

import deviation_large_util as dlu
import deviation_util as du
import evaluate_util as evu
from test_deviation_cpu import _best, _gains
from test_rb_ascent_cpu import _stub_sim


# ------------------------------------------------------------------------------------------ 1: the figures and the reach
def test_the_lds_figures_are_the_formulas():
    from gym_d2d_amd import _native, deviation
    assert _native.DEVIATE_MAX_LDS_BYTES == dlu.MAX_LDS_BYTES
    for name, k in dlu.CASES.items():
        n, r = k['cues'] + k['dues'], k['r']
        got = (du.lds_bytes(n, r), du.lds_bytes(n, r, True))
        assert got == dlu.LDS[name] == (deviation.lds_bytes(n, r), deviation.lds_bytes(n, r, True)), (name, got)
        assert dlu.LDS_64K < got[0] <= dlu.MAX_LDS_BYTES                 # every case goes past 64 KiB without a mask already
        assert (got[1] <= dlu.MAX_LDS_BYTES) == (name in dlu.MASKED)
    assert dlu.MAX_LDS_BYTES - dlu.LDS['d1950_r8'][0] == 672
    # evaluate(), the exact yardstick's source of planes, serves the three shapes as they stand
    own = [evu.lds_bytes(k['cues'] + k['dues'], k['r'], k['law'] != 'ld2') for k in dlu.CASES.values()]
    assert own == [124896, 88208, 28144] and max(own) <= 163840             # D2D_EVALUATE_MAX_LDS_BYTES
    assert max(du.lds_bytes(k['cues'] + k['dues'], k['r'], True) for k in du.CASES.values()) < dlu.LDS_64K      # these are the first


@pytest.mark.parametrize('name', list(dlu.CASES))
def test_what_a_large_case_reaches(name):
    c, k = dlu.make_case(name), dlu.CASES[name]
    sel = dlu.selection(name)
    words_n, levels = (c.n + 31) // 32, int((c.p_max - c.p_min + 1)[sel].max())
    chunk, groups = dlu.chunking(name)
    on = (c.rb >= 0) & (c.rb < c.r)
    sizes = np.stack([np.bincount(c.rb[e][on[e]], minlength=c.r) for e in range(c.b)])
    print(f'{name}: W = {words_n}, M = {len(sel)}, chunk {chunk} x {groups} workgroups per env, group sizes {sizes.min()} .. {sizes.max()}, '
          f'LDS {dlu.LDS[name]}')
    assert c.b == 2 and on.all() and ((c.pwr >= c.p_min) & (c.pwr <= c.p_max)).all()
    assert words_n > 32 or name == 'd300_r1024'
    assert (np.diff(sel) > 1).any() and (np.diff(sel) > 0).all() and sel[-1] == c.n - 1 or name == 'd1100_r40'
    if name == 'd1950_r8':
        assert words_n == 61 and levels == 16 and len(sel) == 40 and (sel >= 1024).sum() == 35 and sel[-1] == c.n - 1
        assert (chunk, groups) == (32, 2) and len(sel) % chunk == 8
        assert 200 <= sizes.min() and sizes.max() <= 300
        for e in range(c.b):                                             # every group has members in words below 32 and from 32 on
            for r in range(c.r):
                members = np.flatnonzero(c.rb[e] == r)
                assert (members < 1024).any() and (members >= 1024).any()
    if name == 'd1100_r40':
        assert words_n == 35 and levels == 4 and sel.tolist() == list(range(0, 1100, 97)) and groups == 1 and (sel >= 1024).any()
        assert (c.r + 31) // 32 == 2 and c.n * 2 == 2200 and du.LAWS[c.law] == 2
    if name == 'd300_r1024':
        assert c.r * levels == 4096 and (chunk, groups) == (1, 6) and 4 * words_n * c.r == 40 * 1024 and (c.r + 31) // 32 == 32
        assert du.LAWS[c.law] == 1
    if name in dlu.MASKED:
        mask = dlu.allowed_mask(name)
        assert mask.shape == (c.n, c.r) and mask.any() and not mask.all()
    if name == 'd300_r1024':
        assert not mask[:, :992].any() and mask[sel[dlu.ONLY_1023]].sum() == 1 and mask[sel[dlu.ONLY_1023], 1023]
        assert (np.bincount(c.rb[0], minlength=c.r)[992:] == 0).any()    # an empty RB in the last word: somewhere to move to
    assert {du.LAWS[k['law']] for k in dlu.CASES.values()} == {0, 1, 2}  # the table and the best kernel under each of the three laws
    if k['oracle'] is not None:
        envs, links = dlu.oracle_links(name)
        assert len(links) >= 4 and np.isin(links, sel).all() and (name != 'd1950_r8' or (links >= 1024).any())


# ------------------------------------------------------------------------------------------ 2: restricted against full
@pytest.mark.parametrize('floors', ['none', 'below'])
@pytest.mark.parametrize('case', ['d40_r2', 'd50_r25'])
def test_the_restricted_oracle_equals_the_full_one_on_the_existing_cases(case, floors):
    c = du.make_case(case)
    envs, links = du.oracle_links(case)
    full = du.oracle_side(case, floors)
    got = dlu.by_oracle_restricted(c, envs, links, None, du.FLOOR_SETTINGS[floors])
    err = np.abs(got.gain - full.gain) / np.maximum(np.abs(full.gain), 1.0)
    print(f'{case} {floors}: {full.open.sum()} open entries, {full.near.sum()} marked, gain restricted against full {err.max():.2e}')
    assert np.array_equal(got.near, full.near) and np.array_equal(got.open, full.open)
    assert err.max() <= dlu.TIE
    assert np.array_equal(got.rb_out, full.rb_out) and np.array_equal(got.pwr_out, full.pwr_out)
    assert (~np.array([[row.on for row in rows] for rows in full.rows])).any() == (case == 'd50_r25')       # a link on no RB is among them


# ------------------------------------------------------------------------------------------ 3: the float64 side of the large cases
@pytest.mark.parametrize('floors', ['none', 'below'])
@pytest.mark.parametrize('name', dlu.ORACLE_CASES)
def test_the_marks_of_the_large_cases_stay_under_the_cap(name, floors):
    c = dlu.make_case(name)
    res = dlu.oracle_side(name, floors)
    free = dlu.oracle_side(name, 'none')
    on = np.array([[row.on for row in rows] for rows in res.rows])
    print(f'{name} {floors}: {res.open.sum()} of {res.open.size} entries open, {res.near.sum()} marked ({res.near.mean():.3%}), '
          f'largest gain {np.nanmax(res.gain):.3e} Mbps, movers {(res.gain_link > 0).sum()}')
    assert on.all() and res.near.mean() <= du.MARK_CAP
    assert not (res.open & ~free.open).any() and np.isfinite(res.gain[res.open]).all()
    for e, rows in enumerate(res.rows):
        for a, row in enumerate(rows):
            assert row.open[row.held] and res.table[e, a][row.held] == 0.0 and np.isfinite(res.table[e, a]).sum() == row.open.sum()
    assert (res.gain_link > 0).any() and (np.abs(res.gain[res.open]) > 1e-3).any()           # gains of a size the bar can see


# ------------------------------------------------------------------------------------------ 4: the refusals
def _wide(n, r):
    return SimpleNamespace(**{**vars(_stub_sim(num_rbs=r)), 'num_envs': 2, 'link_tx': np.ones(n, dtype=np.int64),
                              'link_rx': np.zeros(n, dtype=np.int64)})


def _host(n, r):
    import torch
    from gym_d2d_amd.deviation import Deviation
    return Deviation(_wide(n, r), n, np.zeros(n, np.int32), np.ones(n, np.int32), np.ones(n, bool), torch, torch.device('cpu'))


def _refused(n, r, allowed, need):
    from gym_d2d_amd import _native
    for call in (_gains, _best):
        with pytest.raises(_native.NativeError, match=rf'n_links and n_rbs need {need} bytes of LDS, more than the 163840 a workgroup can have'):
            call(n_links=n, n_rbs=r, allowed=8 if allowed else 0, n_envs=0, n_sel=1)


def test_the_lds_bound_binds_before_the_link_limit():
    from gym_d2d_amd import _native
    before = _native.deviate_launches
    top = dlu.largest_links(1)
    need = du.lds_bytes(top + 1, 1)
    print(f'R = 1, no mask: {top} links need {du.lds_bytes(top, 1)} bytes, {top + 1} need {need}')
    assert top == 1979 and need == 163872 > dlu.MAX_LDS_BYTES >= du.lds_bytes(top, 1)
    _gains(n_links=top, n_rbs=1, n_envs=0, n_sel=1)
    _best(n_links=top, n_rbs=1, n_envs=0, n_sel=1)
    assert _host(top, 1).need(False) == du.lds_bytes(top, 1)
    _refused(top + 1, 1, False, need)
    with pytest.raises(ValueError, match=rf'deviation_gains\(\) .*{top + 1} links on 1 RBs need {need} bytes, more than 163840'):
        _host(top + 1, 1)
    # 2048 links never fit: 80 * 2048 is the limit itself and the tail comes on top; the formula grows with R
    assert _native.DEVIATE_MAX_LINKS == 2048 and 80 * 2048 == dlu.MAX_LDS_BYTES
    needs = [du.lds_bytes(2048, r) for r in range(1, _native.DEVIATE_MAX_RBS + 1)]
    assert min(needs) == needs[0] > dlu.MAX_LDS_BYTES and (np.diff(needs) >= 0).all()
    assert all(dlu.largest_links(r) < 2048 for r in (1, 8, 8192))
    for r in (1, 8, 64, 8192):
        _refused(2048, r, False, du.lds_bytes(2048, r))
        with pytest.raises(ValueError, match=rf'2048 links on {r} RBs need {du.lds_bytes(2048, r)} bytes, more than 163840'):
            _host(2048, r)
    # both limits at once with a mask: megabytes, where offsets in 32 bits would still hold but a narrower sum would not
    most = du.lds_bytes(2048, 8192, True)
    assert most == 80 * 2048 + 4 * 2048 * 256 + 4 * 64 * 8192 + 5216 and most > 1 << 22
    _refused(2048, 8192, True, most)
    assert _native.deviate_launches == before


def test_d1950_r8_with_an_allowed_mask_is_refused():
    from gym_d2d_amd import _native
    before = _native.deviate_launches
    k = dlu.CASES['d1950_r8']
    n, r = k['cues'] + k['dues'], k['r']
    free, masked = dlu.LDS['d1950_r8']
    assert free <= dlu.MAX_LDS_BYTES < masked
    _gains(n_links=n, n_rbs=r, n_envs=0, n_sel=40, n_levels=16)
    _best(n_links=n, n_rbs=r, n_envs=0, n_sel=40, n_levels=16)
    _refused(n, r, True, masked)
    host = _host(n, r)
    assert host.need(False) == free
    with pytest.raises(ValueError, match=rf'{n} links on {r} RBs need {masked} bytes with an allowed mask, more than 163840'):
        host.need(True)
    assert _native.deviate_launches == before

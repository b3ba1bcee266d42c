"""The host side of the table read-side kernels' large cases (table_large_util.py; test_gpu_table_large.py launches them).

1. The group-wise float64 references equal the dense ones - evaluate_util.evaluate_ref through table_evaluate_util.reference, and
   table_marginal_util.marginal_ref - on every existing case of table_evaluate_util.CASES and table_marginal_util.CASES: `decided`
   and `lifted` equal, values to 1e-12 max(|ref|, 1).  Both sides are float64 on the same operands; only the order of at most 300
   terms differs, about 300 * 2^-53 - seven orders under the project's 1e-5 bar, so the group-wise references inherit the dense
   ones' standing.
2. What each large case claims to reach, asserted on the reference alone: the LDS a launch asks for, the largest group, a group on
   both sides of link 1024, an occupied RB past 4096, links at -1 and at R, links of positive capacity and of positive harm - in the
   largest group too - and the share left out at the threshold.

Every test prints what it measured."""
import numpy as np
import pytest

import table_evaluate_util as teu
import table_large_util as tlu
import table_marginal_util as tmu


def _tie(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)).max())


# ------------------------------------------------------------------------------------------ 1: group-wise against dense
@pytest.mark.parametrize('case', teu.CASES)
def test_evaluate_groupwise_equals_the_dense_reference_on_every_existing_case(case):
    c = teu.make_case(*case)
    sinr, cap, total, decided = teu.case_ref(*case)
    g_sinr, g_cap, g_total, g_decided = tlu.evaluate_groupwise(c)
    errs = [_tie(a, m) for a, m in ((g_sinr, sinr), (g_cap, cap), (g_total, total))]
    print(f'{case}: sinr_db {errs[0]:.2e}, capacity {errs[1]:.2e}, total {errs[2]:.2e}')
    assert np.array_equal(g_decided, decided)
    assert max(errs) <= tlu.TIE


@pytest.mark.parametrize('case', tmu.CASES)
def test_marginal_groupwise_equals_the_dense_reference_on_every_existing_case(case):
    c, ref = tmu.make_case(*case), tmu.case_ref(*case)
    got = tlu.marginal_groupwise(c)
    errs = {name: _tie(got[name], ref[name]) for name in ('harm', 'difference', 'capacity', 'sinr_db')}
    print(f'{case}: ' + ', '.join(f'{name} {e:.2e}' for name, e in errs.items()))
    assert np.array_equal(got['decided'], ref['decided']) and np.array_equal(got['lifted'], ref['lifted'])
    assert max(errs.values()) <= tlu.TIE


def test_marginal_groupwise_equals_the_dense_reference_on_the_planted_lift():
    """The one existing case with a lifted victim (the existing draws have none)."""
    c, p, _ = tmu.planted_lifted()
    ref, got = tmu.marginal_ref(c), tlu.marginal_groupwise(c)
    assert got['lifted'][tmu.PLANT_ENV, p] == 1 and np.array_equal(got['lifted'], ref['lifted'])
    assert np.array_equal(got['decided'], ref['decided'])
    assert max(_tie(got[name], ref[name]) for name in ('harm', 'difference', 'capacity', 'sinr_db')) <= tlu.TIE


def test_the_two_groupwise_references_agree_on_the_large_cases():
    """capacity and sinr_db of candidate 0, two routes through the same group sums."""
    for case in tlu.CASES:
        sinr, cap, _, _ = tlu.evaluate_case_ref(*case)
        m = tlu.marginal_case_ref(*case)
        assert np.array_equal(m['sinr_db'], sinr[:, 0]) and np.array_equal(m['capacity'], cap[:, 0])


# ------------------------------------------------------------------------------------------ 2: what the large cases reach
def test_the_lds_figures_and_the_64_kib_branch():
    figures = {case: (teu.lds_bytes(case[0], case[1]), tmu.lds_bytes(case[0], case[1])) for case in tlu.CASES}
    print(figures)
    assert [figures[case] for case in tlu.CASES[:3]] == [(106560, 122912), (74048, 90400), (73776, 90128)]
    for case in tlu.CASES:
        assert all(tlu.LDS_64K < need <= tlu.MAX_LDS_BYTES for need in figures[case]) == (case in tlu.PAST_64K)
        assert all(need <= tlu.MAX_LDS_BYTES for need in figures[case])
    # no existing case of either table goes past 64 KiB: these are the first
    assert max(teu.lds_bytes(c[0], c[1]) for c in teu.CASES) < tlu.LDS_64K
    assert max(tmu.lds_bytes(c[0], c[1]) for c in tmu.CASES) < tlu.LDS_64K


@pytest.mark.parametrize('case', tlu.CASES)
def test_what_a_large_case_reaches(case):
    n, r, k, b, dtype, extra = case
    c = tlu.make_case(*case)
    sinr, cap, total, decided = tlu.evaluate_case_ref(*case)
    m = tlu.marginal_case_ref(*case)
    rb = c['rb']
    assert c['table'].shape == (b, n + extra, n) and str(c['table'].dtype) == dtype
    assert not extra or np.isnan(c['table'][:, n]).all()
    assert (rb == -1).any() and (rb == r).any() and (c['rb'][:, 0] == -1).any() and (c['rb'][:, 0] == r).any()
    sizes = np.array([tlu.group_sizes(rb[e, q], r).max() for e in range(b) for q in range(k)])
    big = tlu.largest_group(rb[0, 0], r)
    both_sides = sum(len(tlu.straddles(rb[e, q], r)) for e in range(b) for q in range(k))
    left_eval, left_marg = float((~decided).mean()), float((~m['decided']).mean())
    cap_pos, harm_pos = (cap[:, 0] > 0).sum(axis=1), (m['harm'] > 0).sum(axis=1)
    in_big = (cap[0, 0][big] > 0) & (m['harm'][0][big] > 0)
    print(f'{case}: largest group {sizes.max()}, groups on both sides of link 1024: {both_sides}, capacity > 0 on {cap_pos.tolist()} links, '
          f'harm > 0 on {harm_pos.tolist()} (largest harm {m["harm"].max():.3e} Mbps, largest capacity {cap.max():.3e}), {int(in_big.sum())} '
          f'such links in the largest group, lifted {int(m["lifted"].sum())}, left out {left_eval:.3%} / {left_marg:.3%}')
    assert both_sides >= 1
    assert (cap_pos >= 64).all() and (harm_pos >= 64).all() and in_big.any()
    assert left_eval <= tlu.THRESHOLD_CAP and left_marg <= tlu.THRESHOLD_CAP
    assert np.isfinite(sinr).all() and np.isfinite(m['harm']).all() and (m['harm'] >= 0).all()
    assert len({t.tobytes() for t in total.reshape(-1)}) == b * k                       # no two candidates alike
    if case == tlu.CASES[0]:
        assert r > n and (rb[(rb >= 0) & (rb < r)] >= 4096).any() and -(-k // teu.CHUNK) == 2 and k % teu.CHUNK == 1 and extra == 1
    if case == tlu.CASES[1]:
        assert b == 2 and 20 <= sizes.min() and sizes.max() <= 64 and extra == 0
    if case == tlu.CASES[2]:
        assert n % 4 == 3 and sizes.max() > 512 and -(-n // teu.THREADS) == 8
    if case == tlu.CASES[3]:
        assert n % 4 == 1 and n - 1 == 1024 and (rb == 256).any() and extra == 1


def test_the_planted_entries_lie_past_link_1024():
    c = tlu.make_case(*tlu.PLANT)
    j, i, readers = tlu.planted(c, True)
    assert min(j, i) >= 1024 and j != i and 1 <= readers.sum() < c['k']
    for q in range(c['k']):
        assert readers[q] == (c['rb'][0, q, j] == c['rb'][0, q, i] and 0 <= c['rb'][0, q, j] < c['r'])
    j, i, readers = tlu.planted(c, False)
    assert min(j, i) >= 1024 and j != i and not readers.any()
    assert all(c['rb'][0, q, j] != c['rb'][0, q, i] or not 0 <= c['rb'][0, q, j] < c['r'] for q in range(c['k']))
    m = tlu.make_marginal_case(*tlu.PLANT)
    j, i, readers = tlu.planted(m, True)
    assert min(j, i) >= 1024 and readers.tolist() == [True] and m['rb'][0, j] == m['rb'][0, i]
    j, i, readers = tlu.planted(m, False)
    assert min(j, i) >= 1024 and readers.tolist() == [False] and m['rb'][0, j] != m['rb'][0, i]

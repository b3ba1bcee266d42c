"""The large read-side tests, the part that needs no GPU: every float64 reference of read_side_util.py tied to the oracle where the
oracle has the law, the caps of the GPU cases (the 1 % sensitivity cap of the marginal cases, neighbors_util.CAP of the neighbour
cases) asserted on the references of the very seeds the GPU tests use, and the claims the case tables make about LDS sizes."""
import numpy as np
import pytest

import marginal_util as mu
import neighbors_util as nbu
import rb_sensing_util as rbs
import read_side_util as rsu
from golden_util import load_case, rel_err
from oracle import d2d_oracle as orc

ORACLE_LAWS = ('ld2', 'ld35', 'urban')
# (cues, due pairs, RBs, law, envs): the shapes of the eight cases of rb_sensing_util.CASES; case07's comes from its fixture
OLD_SHAPES = [(8, 8, 5, 'ld2', 3), (64, 96, 24, 'ld35', 2), (64, 64, 8, 'urban', 2), (6, 6, 40, 'suburban', 2), (24, 40, 16, 'ld2', 2),
              (8, 8, 5, 'urban', 3), (8, 8, 5, 'suburban', 3), 'case07_device_config']


def _old_shape(entry):
    if isinstance(entry, tuple):
        return entry
    meta = load_case(entry).meta
    pl = meta['path_loss']
    law = {2.0: 'ld2', 3.5: 'ld35'}[pl['ple']] if pl['kind'] == 'log_distance' else pl['area']
    return meta['num_cues'], meta['num_due_pairs'], meta['num_rbs'], law, 2


def _f64(c):
    return np.asarray(c['pos'], dtype=np.float64)


@pytest.mark.parametrize('law', ORACLE_LAWS)
def test_pair_pl_db_equals_the_oracle_s_pair_path_loss(law):
    c = rsu.make_case(41, 3, law)
    ref = orc.pair_path_loss_db(c['spec'], _f64(c), c['tx'], c['rx'], c['ocols'])
    got = rsu.pair_pl_db(c)
    e = rel_err(got, ref)
    print(f'41 links, {law}: pair_pl_db vs orc.pair_path_loss_db rel_err {e:.3e} over {ref.size} pairs, {ref.min():.1f} .. {ref.max():.1f} dB')
    assert got.shape == ref.shape == (c['b'], 41, 41) and np.isfinite(ref).all()
    assert e <= 1e-9
    assert rel_err(rsu.coupling_ref(c), nbu.coupling_ref(_f64(c), c['tx'], c['rx'], c['ocols'], c['spec'])) <= 1e-9


@pytest.mark.parametrize('law', ORACLE_LAWS + ('mixed',))
@pytest.mark.parametrize('n', [41, 2048])
def test_law_columns_are_the_ones_the_shared_cases_fold(n, law):
    """read_side_util.law_columns rebuilds what best_rb_util.make_case folded: the same float32 block, bit for bit."""
    from gym_d2d_amd.sensing import fold_columns
    c = rsu.make_case(n, 3, law)
    budget = {'eirp_off_db': c['ocols'].eirp_off_db, 'rx_off_db': c['ocols'].rx_off_db, 'noise_dbm': c['ocols'].noise_dbm}
    cols, kind, pow_k = fold_columns(budget, c['law_cols'], c['tx'])
    assert (kind, pow_k) == (c['kind'], c['pow_k']) and np.array_equal(cols.view(np.uint32), c['cols'].view(np.uint32))


@pytest.mark.parametrize('entry', OLD_SHAPES, ids=lambda e: e if isinstance(e, str) else '%dx%d_%d_%s' % e[:4])
def test_interference_per_rb_equals_the_one_hot_sum(entry):
    cues, dues, r, law, b = _old_shape(entry)
    c = rsu.build_case(cues, dues, r, law, b=b)
    ref = rbs.interference_mw(_f64(c), c['tx'], c['rx'], c['rb'], c['pwr'], c['ocols'], c['spec'], r)
    got = rsu.interference_per_rb(c)
    assert got.shape == ref.shape == (b, cues + dues, r)
    empty = ref == 0.0
    assert np.array_equal(got == 0.0, empty) and not empty.all()
    e = float(np.max(np.abs(got[~empty] - ref[~empty]) / ref[~empty]))
    print(f'{cues} + {dues} links, {r} RBs, {law}: interference_per_rb vs the one-hot einsum: {e:.3e} relative, {empty.mean():.1%} empty')
    assert e <= 1e-12
    ref_s = rbs.sinr_from_interference(_f64(c), c['tx'], c['rx'], c['pwr'], c['ocols'], c['spec'], ref)
    assert rel_err(rsu.sinr_per_rb(c, got), ref_s) <= 1e-9


@pytest.mark.parametrize('law', ORACLE_LAWS)
@pytest.mark.parametrize('n,r,cell', [(41, 3, 500.0), (41, 1, rsu.CELL_40), (131, 33, 500.0)])
def test_leave_one_out_direct_equals_the_oracle_s_leave_one_out(n, r, cell, law):
    c = rsu.make_case(n, r, law, cell_radius=cell)
    ref_diff, ref_harm, ref_cap, _ = mu.leave_one_out(_f64(c), c['tx'], c['rx'], c['rb'], c['pwr'], c['ocols'], c['spec'], r)
    diff, harm, cap, decided = rsu.leave_one_out_direct(c)
    e = [rel_err(a, b) for a, b in ((harm, ref_harm), (diff, ref_diff), (cap, ref_cap))]
    print(f'{n} links, {r} RBs, {law}, {cell:.0f} m: harm / difference / capacity vs marginal_util.leave_one_out: '
          f'{e[0]:.3e} / {e[1]:.3e} / {e[2]:.3e}; harm up to {ref_harm.max():.3f} Mbps; {(~decided).mean():.2%} undecided')
    assert max(e) <= 1e-9
    assert (ref_harm > 1e-3).any() and (harm[c['bad']] == 0.0).all()


def test_decided_marks_a_link_whose_victim_sits_on_the_threshold():
    """The rule itself, on a case bent for it: one receiver's sensitivity moved onto its own SINR undecides every link of its RB and
    no link of another RB."""
    c = rsu.make_case(41, 3, 'ld2')
    assert rsu.leave_one_out_direct(c)[3].all()
    sinr = rsu.sinr_per_rb(c, rsu.interference_per_rb(c))
    j = int(np.nonzero(~c['bad'][0] & (np.arange(41) >= 11))[0][0])         # a DUE link (a receiver of its own) on an RB, env 0
    ocols = orc.DeviceColumns(**{k: np.array(v, dtype=np.float64) for k, v in vars(c['ocols']).items()})
    ocols.sens_dbm[c['rx'][j]] = sinr[0, j, c['rb'][0, j]] + 1e-7
    decided = rsu.leave_one_out_direct(dict(c, ocols=ocols))[3]
    same_rb = c['rb'][0] == c['rb'][0, j]
    assert not decided[0, same_rb].any() and decided[0, ~same_rb].all() and decided[1:].all()


@pytest.mark.parametrize('n,r,law,b,cell', rsu.MARGINAL_CASES + ((1000, rsu.MARGINAL_WIDE_R, 'mixed', 2, 500.0),))
def test_marginal_cases_stay_inside_the_sensitivity_cap(n, r, law, b, cell):
    """On the reference alone, for the seeds test_gpu_read_side_large.py launches: at most 1 % of a case's links undecided."""
    if r == rsu.MARGINAL_WIDE_R:
        c = rsu.wide_r_case()[1]
    else:
        c = rsu.make_case(n, r, law, b=b, cell_radius=cell)
    diff, harm, cap, decided = rsu.marginal_ref(n, r, law, b, cell)
    members = np.array([(c['rb'][e][~c['bad'][e]] == q).sum() for e in range(b) for q in range(min(r, 64))])
    lds = rsu.lds_bytes('marginal', n, r, law != 'ld2')
    print(f'{n} links, {r} RBs, {law}, {cell:.0f} m: {(~decided).mean():.2%} of {decided.size} links undecided; harm up to {harm.max():.3f} Mbps, '
          f'positive on {(harm > 0).mean():.1%}; up to {members.max()} members per RB; {lds / 1024:.1f} KiB of LDS')
    assert np.isfinite(diff).all() and (harm >= 0.0).all()
    assert (~decided).mean() <= 0.01
    assert (harm[c['bad']] == 0.0).all() and c['bad'].any()
    if n == 2048:
        assert (harm[:, 1024:] > 0.0).any() and (harm[:, 1024:] > 0.0).mean() > 0.5
    if r == 1:
        assert c['bad'].mean() < 0.2 and (harm[~c['bad']] > 0.0).all()
    assert (lds > 64 * 1024) == ((n, law) in ((1000, 'mixed'), (2048, 'ld35'), (2048, 'ld2')))


def test_lds_sizes_named_in_the_case_tables():
    kib = lambda *a: rsu.lds_bytes(*a) / 1024
    assert 70 < kib('marginal', 1000, 8, True) < 71 and 62 < kib('marginal', 1000, 8, False) < 63
    assert kib('marginal', 2048, 64, True) < 145 and kib('marginal', 2048, 64, False) < 129
    assert 85 < kib('marginal', 1000, rsu.MARGINAL_WIDE_R, True) < 87
    assert kib('neighbors', 2048, 1, True) == 80 and kib('neighbors', 2048, 1, False) == 64
    assert 80 < kib('sense', 2048, 5, True) < 83 and 64 < kib('sense', 2048, 64, False) < 65


@pytest.mark.parametrize('n,law,b,down', rsu.NEIGHBOR_CASES)
def test_neighbor_cases_stay_inside_the_near_tie_cap(n, law, b, down):
    """On the reference alone, for the seeds the GPU test uses: the share of index entries left out as near ties is 0 at k = 1 and
    inside neighbors_util.CAP at k = 8 and 64 (read_side_util.NEIGHBOR_CASES records the shares: up to 0.31 % and 3.8 %); the
    downlink case holds exact ties, and the 2048-link cases select links at 1024 and above."""
    c, ref = rsu.neighbor_case(n, law, b, down)
    assert ref.shape == (b, n, n) and np.isfinite(ref).all()
    for k in rsu.KS:
        idx, vals, comparable = rsu.neighbor_ranked(n, law, b, down, k)
        left_out = 1.0 - float(comparable.mean())
        ties = float((vals[:, :, :-1] == vals[:, :, 1:]).mean()) if k > 1 else 0.0
        high = float((idx >= 1024).mean())
        print(f'{n} links, {law}, downlink {down}, k={k}: {left_out:.2%} left out as near ties, {ties:.1%} of the gaps exact ties, '
              f'{high:.1%} of the entries name a link >= 1024')
        assert left_out <= nbu.CAP
        if k == 1:
            assert left_out == 0.0
        if down and k == 8:
            assert ties > 0.2
        if n == 2048 and law == 'ld35':
            assert high > 0.25


def test_case_tables_hold_what_they_claim():
    for n, (cues, dues) in rsu.SHAPES.items():
        assert cues + dues == n
    assert 259 % 4 == 3 and 260 % 4 == 0 and 1000 % 64 != 0
    c = rsu.make_case(259, 1, 'ld2', downlink=True)
    assert (c['tx'][:59] == 0).all() and np.array_equal(c['rx'][:59], np.arange(1, 60)) and (c['tx'][59:] > 59).all()
    u = rsu.make_case(259, 1, 'ld2')
    assert (u['rx'][:59] == 0).all() and np.array_equal(u['tx'][59:], c['tx'][59:])
    for case in (c, u, rsu.make_case(1000, 8, 'mixed')):
        assert case['pos'].dtype == np.float32 and 0.05 < case['bad'].mean() < 0.2
    assert rsu.make_case(1000, 8, 'mixed')['kind'] != rsu.make_case(1000, 8, 'ld2')['kind']

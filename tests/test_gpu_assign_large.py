"""The matching kernels near their stated limits, launched directly through _native: assign_weights_kernel and assign_solve_kernel
(csrc/d2d_assign.hip) and assign_power_weights_kernel (csrc/d2d_assignpwr.hip) at 2048 links, up to 163 392 of the 163 840 bytes of
LDS a workgroup can have, `allowed` masks of 11 and 19 words with a partly filled last word, 64 power levels, and matchings in which
a thread owns up to 27 columns and has to decide between them.

The yardsticks are the existing ones, and so are the bars.  Weights and harm: assign_util.weights_ref in float64 at the project's
1e-5 (|d| <= 1e-5 max(|ref|, 1)), entries near a threshold left out, at most 1 % of a case (none on these seeds:
test_solver_large_cpu.py).  Objective 'own': evaluate()'s capacity_mbps bit for bit.  The matching: col, feasible and the bits of
value equal assign_util.solve_ref on the very float32 matrix that was launched.  Joint power without floors: the running maximum of
per-level d2d_assign_weights launches bit for bit; with floors: assignpwr_util.weights_power_ref through test_gpu_assignpwr's
_check_floors.  solver_large_util's tables name the path every case forces; test_solver_large_cpu.py asserts on the references alone
that it is reached.  Every launch writes between guard words, which the launch helpers check.  Every test prints what it measured.

Measured on an MI355X: weights rel_err 2.8e-7 - 8.6e-7, harm 1.5e-7 - 2.5e-7, own 2.6e-7 - 2.9e-7 over the four cases and the two
masked ones, nothing left out at a threshold; own equals evaluate()'s capacity on 100 % of 256 candidates per env at 2048 links and of
1320 under the power law; every matching equal to the restatement, 626 / 159 matched columns at and past 256 / 512 on the 548 x 600
planes, the highest matched column 5999 (a thread's 24th); the planes without floors equal to the per-level launches on 100 % of the
entries at 2048 links, at 64 and at 63 levels; with floors weights rel_err 2.8e-7 and 4.1e-7, the reference at the chosen power equal
to its maximum, 0.006 % and 0.020 % left out.  The slowest test takes 2.6 s, its float64 reference nearly all of it (CHANGELOG.md,
"Tests: the matching and colouring kernels at 2048 links and wide masks")."""
import numpy as np
import pytest

import assign_util as asu
import assignpwr_util as apu
import evaluate_util as evu
import solver_large_util as slu
from test_gpu_assign import _bits, _launch_solve, _launch_weights, _own_weights_are_evaluates_capacity, _planes_err
from test_gpu_assignpwr import _check_floors, _launch_power_weights, _running_maximum

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _zero_harm_where_nobody_is(c, links, harm):
    """harm is 0.0 bit for bit on the RBs that hold no background member."""
    movable = np.zeros(c['n'], bool)
    movable[links] = True
    rb = np.asarray(c['rb'])
    for e in range(c['b']):
        held = rb[e][~movable & (rb[e] >= 0) & (rb[e] < c['r'])]
        empty = np.setdiff1d(np.arange(c['r']), held)
        assert (_bits(harm[e][:, empty]) == 0).all()
    return len(empty)


def _two_roundings(w, o, h):
    """w is (own - harm) rounded once from the double sum behind the float32 harm plane: two float32 roundings apart at the most -
    the relation test_gpu_assign.py asserts."""
    o64, h64 = o.astype(np.float64), h.astype(np.float64)
    assert (np.abs(w - (o64 - h64)) <= 2.0 ** -22 * (np.abs(o64) + np.abs(h64))).all()


# ------------------------------------------------------------------------------------------------ the weights kernel
@pytest.mark.parametrize('cues,dues,r,law', list(slu.WEIGHT_CASES))
def test_weights_near_the_limits_against_the_float64_reference(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    own, harm, near = slu.weights_case_ref(cues, dues, r, law)
    w, h = _launch_weights(c, links)
    assert np.isfinite(w).all() and np.isfinite(h).all()
    e_w, e_h = _planes_err(w, h, own, harm, near)
    empty = _zero_harm_where_nobody_is(c, links, h)
    o, none = _launch_weights(c, links, objective=1, harm=False)
    assert none is None and np.isfinite(o).all()
    e_o = evu.rel_err(o[~near], own[~near])
    print(f'{cues} + {dues} links, {r} RBs, {law}: weights rel_err {e_w:.3e}, harm rel_err {e_h:.3e}, own rel_err {e_o:.3e}; '
          f'{near.mean():.3%} left out at a threshold; {(own - harm < 0).mean():.1%} of the weights negative; {empty} RBs of the last env '
          f'without a background member; LDS {slu.WEIGHT_CASES[(cues, dues, r, law)][0]} B')
    assert near.mean() <= asu.THRESHOLD_CAP
    assert e_w <= asu.BAR and e_h <= asu.BAR and e_o <= asu.BAR
    _two_roundings(w, o, h)
    if (cues, dues, r, law) == slu.RELAUNCH_CASE:                       # a second launch, and pointers moved by 4 bytes: the same bits
        for other in (_launch_weights(c, links), _launch_weights(c, links, shift=1)):
            assert np.array_equal(_bits(other[0]), _bits(w)) and np.array_equal(_bits(other[1]), _bits(h))


@pytest.mark.parametrize('cues,dues,r,law', list(slu.MASKED_CASES))
def test_scattered_movable_links_under_a_mask_of_many_words(cues, dues, r, law):
    """-inf exactly where forbidden and the reference elsewhere; harm is written where forbidden too.  links[1] may take RB R - 1
    alone, links[2] nothing; bits at and above R in the last word change nothing."""
    from gym_d2d_amd.best_response import pack_allowed
    c = asu.case(cues, dues, r, law)
    links, allowed = slu.masked_movable(c)
    own, harm, near = slu.masked_case_ref(cues, dues, r, law)
    w, h = _launch_weights(c, links, allowed=allowed)
    free = np.broadcast_to(allowed[links][None], w.shape)
    assert (w[~free] == -np.inf).all() and np.isfinite(w[free]).all() and np.isfinite(h).all()
    assert np.isfinite(w[:, 1, r - 1]).all() and (w[:, 1, :r - 1] == -np.inf).all() and (w[:, 2] == -np.inf).all()
    keep = free & ~near
    e_w, e_h = evu.rel_err(w[keep], (own - harm)[keep]), evu.rel_err(h[~near], harm[~near])
    words, tail = slu.MASKED_CASES[(cues, dues, r, law)]
    print(f'{cues} + {dues} links, {r} RBs, {law}: {len(links)} movable links ({(links < cues).sum()} CUE), {words} words with a {tail}-bit '
          f'tail, {(~free).mean():.1%} forbidden; weights rel_err {e_w:.3e}, harm rel_err {e_h:.3e}; {near.mean():.3%} left out')
    assert near.mean() <= asu.THRESHOLD_CAP and e_w <= asu.BAR and e_h <= asu.BAR
    _zero_harm_where_nobody_is(c, links, h)
    o, _ = _launch_weights(c, links, allowed=allowed, objective=1, harm=False)
    assert (o[~free] == -np.inf).all()
    _two_roundings(w[free], o[free], h[free])
    w2, h2 = _launch_weights(c, links, allowed=slu.with_tail_bits(pack_allowed(allowed), r))
    assert np.array_equal(_bits(w2), _bits(w)) and np.array_equal(_bits(h2), _bits(h))


@pytest.mark.parametrize('cues,dues,r,law', list(slu.OWN_CASES))
def test_own_weights_are_evaluates_capacity_bit_for_bit_at_2048_links_and_under_a_power_law(cues, dues, r, law):
    links = slu.OWN_CASES[(cues, dues, r, law)]
    o = _own_weights_are_evaluates_capacity(cues, dues, r, law, links=links)
    own, _, near = slu.own_case_ref(cues, dues, r, law)
    e_o = evu.rel_err(o[~near], own[~near])
    print(f'    own rel_err against the float64 reference {e_o:.3e}; {near.mean():.3%} left out')
    assert near.mean() <= asu.THRESHOLD_CAP and e_o <= asu.BAR


# ------------------------------------------------------------------------------------------------ the matching kernel
def _equals(got, want, name):
    """col, feasible and the bits of value of every env against (col, value, feasible) lists of asu.solve_ref results."""
    col, value, feasible = got
    for e, (rc, rv, rf) in enumerate(want):
        assert feasible[e] == rf, (name, e)
        assert np.array_equal(col[e], rc), (name, e, np.nonzero(col[e] != rc)[0][:8])
        assert _bits(value[e]) == _bits(rv), (name, e, value[e], rv)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('cues,dues,r,law', slu.PLANE_CASES)
def test_matching_on_the_kernels_own_weight_planes(cues, dues, r, law, masked):
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    allowed = slu.plane_allowed(c) if masked else None
    w, _ = _launch_weights(c, links, allowed=allowed, harm=False)
    if masked:
        assert np.array_equal(np.isfinite(w), np.broadcast_to(allowed[links][None], w.shape))
    got = _launch_solve(w)
    _equals(got, [asu.solve_ref(w[e]) for e in range(w.shape[0])], f'{dues} x {r}, masked {masked}')
    high, higher = slu.plane_conditions(w, got[0], got[2])
    rows = np.arange(dues)
    for e in range(w.shape[0]):
        assert len(set(got[0][e].tolist())) == dues and np.isfinite(w[e][rows, got[0][e]]).all()
    print(f'{dues} x {r} ({law}), masked {masked}: feasible {got[2].tolist()}, value {got[1].tolist()}; matched columns >= 256: {high}, '
          f'>= 512: {higher}; LDS {asu.solve_lds_bytes(dues, r)} B')


@pytest.mark.parametrize('name', list(slu.SYNTHETIC))
def test_matching_of_synthetic_matrices_with_ties_long_paths_and_many_columns_per_thread(name):
    seeds = slu.SYNTHETIC[name][2]
    refs = [slu.solved(name, seed) for seed in seeds]
    w = np.stack([x[0] for x in refs])
    got = _launch_solve(w)
    _equals(got, [x[1:] for x in refs], name)
    assert got[2].all()
    print(f'{name}: {w.shape[0]} envs, value {got[1].tolist()}, highest matched column {got[0].max(axis=1).tolist()}; LDS '
          f'{slu.SYNTHETIC[name][3]} B')
    if name == slu.WIDE:                                                # moved pointers (feasible by one byte too): the same bits
        moved = _launch_solve(w, shift=1)
        assert np.array_equal(moved[0], got[0]) and np.array_equal(_bits(moved[1]), _bits(got[1])) and np.array_equal(moved[2], got[2])


def test_an_env_that_cannot_be_matched_at_width_leaves_its_neighbours_alone():
    for name, w, bad in slu.infeasible_batches():
        want = [asu.solve_ref(w[e]) if e == bad else slu.solved(slu.WIDE, slu.WIDE_SEEDS[e])[1:] for e in range(3)]
        col, value, feasible = got = _launch_solve(w)
        _equals(got, want, name)
        print(f'{name}: feasible {feasible.tolist()}, value {value.tolist()}')
        assert feasible.tolist() == [1, 0, 1] and (col[bad] == -1).all() and _bits(value[bad]) == 0


# ------------------------------------------------------------------------------------------------ joint RB and power
def _exact(name, c, links, lo, hi, allowed=None):
    want_w, want_p = _running_maximum(c, links, lo, hi, allowed)
    w, p = _launch_power_weights(c, links, lo, hi, allowed=allowed)
    levels = sorted(set((hi - lo + 1)[links].tolist()))
    print(f'{name}: {levels} levels; weights equal {(_bits(w) == _bits(want_w)).mean():.2%}, powers equal {(p == want_p).mean():.2%}; '
          f'chosen powers {int(p[p != apu.NO_POWER].min())} .. {int(p.max())} dBm')
    assert np.array_equal(_bits(w), _bits(want_w))
    assert np.array_equal(p, want_p)
    return w, p


@pytest.mark.parametrize('case,bounds', [(case, b) for case, many in slu.EXACT_CASES.items() for b in many],
                         ids=lambda x: '-'.join(map(str, x)))
def test_without_floors_the_planes_are_the_running_maximum_at_2048_links_and_at_64_levels(case, bounds):
    cues, dues, r, law = case
    c = asu.case(*case)
    links = asu.due_links(c, cues)
    lo, hi = apu.uniform_bounds(c, *bounds)
    w, p = _exact(f'{cues} + {dues} links, {r} RBs, {law}, {bounds[0]} .. {bounds[1]} dBm', c, links, lo, hi)
    assert np.isfinite(w).all() and (p >= bounds[0]).all() and (p <= bounds[1]).all()
    if bounds[1] - bounds[0] + 1 == apu.MAX_LEVELS:                     # the eighth chunk is scanned: its levels are chosen somewhere
        assert (p >= bounds[0] + apu.MAX_LEVELS - apu.CHUNK).any()


def test_without_floors_scattered_links_by_class_alphabets_and_an_11_word_mask_bit_for_bit():
    cues, dues, r, law = slu.EXACT_SCATTERED
    c = asu.case(cues, dues, r, law)
    links, allowed = slu.masked_movable(c)
    lo, hi = apu.scattered_bounds(c, cues=cues)
    w, p = _exact(f'scattered on {cues} + {dues} links, {r} RBs', c, links, lo, hi, allowed)
    free = np.broadcast_to(allowed[links][None], w.shape)
    assert (w[~free] == -np.inf).all() and (p[~free] == apu.NO_POWER).all() and np.isfinite(w[free]).all()
    assert ((p >= lo[links][None, :, None]) & (p <= hi[links][None, :, None]))[free].all()
    assert (w[:, 2] == -np.inf).all() and np.isfinite(w[:, 1, r - 1]).all()


@pytest.mark.parametrize('cues,dues,r,law', list(slu.FLOOR_CASES))
def test_floors_near_the_limits_against_the_float64_reference(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    links = slu.floor_links(c, cues, dues, r, law)
    lo, hi = apu.uniform_bounds(c, *slu.FLOOR_CASES[(cues, dues, r, law)][1])
    ref_w, valid, marks = slu.floor_case_ref(cues, dues, r, law)
    name = f'{cues} + {dues} links, {r} RBs, {law}, M = {len(links)}'
    for q, pair in enumerate(apu.FLOOR_SETTINGS, start=1):
        w, p = _launch_power_weights(c, links, lo, hi, floor=apu.class_floors(c, cues, pair))
        _check_floors(f'{name}, floors {pair}', w, p, lo[links], ref_w, valid, *marks[q])
    # every eighth movable link under a floor no power reaches: its rows are -inf / NO_POWER, the others are judged as before
    w, p = _launch_power_weights(c, links, lo, hi, floor=slu.unreachable_floors(c, cues, dues, r, law))
    _check_floors(f'{name}, floors unreachable for every eighth row', w, p, lo[links], ref_w, valid, *marks[3])
    assert (w[:, ::8] == -np.inf).all() and (p[:, ::8] == apu.NO_POWER).all()
    # floors of -inf constrain nothing: the planes of the launch without floors, bit for bit
    none = _launch_power_weights(c, links, lo, hi)
    inf = _launch_power_weights(c, links, lo, hi, floor=np.full(c['n'], -np.inf))
    assert np.array_equal(_bits(none[0]), _bits(inf[0])) and np.array_equal(none[1], inf[1])

"""The reference's side of test_gpu_assign_large.py and test_gpu_color_large.py: every cap, feasibility and coverage condition of
solver_large_util's case tables, asserted on the float64 references and the restatements alone.  No GPU is needed.  A case that
did not reach the path its row names would make the GPU comparison pass for nothing, so each row's claim is a condition here:
the LDS bytes by the host modules' formulas, the share left out near a threshold (at most THRESHOLD_CAP), link indices on both
sides of 1024, matched columns a thread marks in a bit of `scanned` above bit 0, chosen levels on both sides of the chunk of 8,
RBs at and past 256.  Every test prints what it measured."""
import numpy as np
import pytest

import assign_util as asu
import assignpwr_util as apu
import color_util as cu
import evaluate_util as evu
import solver_large_util as slu


# ------------------------------------------------------------------------------------------ the weights
@pytest.mark.parametrize('cues,dues,r,law', list(slu.WEIGHT_CASES))
def test_weight_cases_fit_stay_under_the_threshold_cap_and_reach_what_they_name(cues, dues, r, law):
    from gym_d2d_amd import _native, assignment
    c = asu.case(cues, dues, r, law)
    n, links = c['n'], asu.due_links(c, cues)
    lds = assignment.lds_bytes(n, r, law != 'ld2')
    assert lds == asu.lds_bytes(n, r, law != 'ld2') == slu.WEIGHT_CASES[(cues, dues, r, law)][0]
    assert 64 * 1024 < lds <= _native.ASSIGN_MAX_LDS_BYTES == slu.MAX_LDS_BYTES
    own, harm, near = slu.weights_case_ref(cues, dues, r, law)
    rb = np.asarray(c['rb'])[:, :cues]
    members = np.stack([np.bincount(row[(row >= 0) & (row < r)], minlength=r) for row in rb])
    print(f'{cues} + {dues} links, {r} RBs, {law}: LDS {lds} B; {near.mean():.3%} near a threshold; {(own - harm < 0).mean():.1%} of the '
          f'weights negative; harm > 0 on {(harm > 0).mean():.1%}; members per RB {members.min()} .. {members.max()}, '
          f'{(members == 0).mean():.1%} of the RBs empty')
    assert near.mean() <= asu.THRESHOLD_CAP
    assert np.isfinite(own).all() and np.isfinite(harm).all() and (harm > 0).any() and (own > 0).any()
    if (cues, dues, r, law) == (1024, 1024, 64, 'ld35'):
        assert n == 2048 and links.min() >= 1024 and len(links) > r and members.max() >= 16 and (own - harm < 0).any()
    if (cues, dues, r, law) == (48, 2000, 256, 'mixed'):
        assert len(links) == 2000 and (members == 0).mean() > 0.5
    if (cues, dues, r, law) == (1500, 548, 600, 'ld2'):
        assert -(-r // 64) == 10 and (own - harm < 0).mean() > 0.1
    if (cues, dues, r, law) == (700, 330, 330, 'mixed'):
        assert len(links) == r


@pytest.mark.parametrize('cues,dues,r,law', list(slu.MASKED_CASES))
def test_masked_weight_cases_have_the_words_the_tail_and_the_two_special_rows(cues, dues, r, law):
    from gym_d2d_amd.best_response import pack_allowed
    c = asu.case(cues, dues, r, law)
    links, allowed = slu.masked_movable(c)
    words, tail = slu.MASKED_CASES[(cues, dues, r, law)]
    packed = pack_allowed(allowed)
    assert packed.shape == (c['n'], words) and r % 32 == tail and words > 2
    assert (links < cues).any() and (links >= cues).any()               # CUE and DUE links alike
    assert allowed[links[1]].sum() == 1 and allowed[links[1], r - 1] and not allowed[links[2]].any()
    full = slu.with_tail_bits(packed, r)
    assert (full[:, -1] >> np.uint32(tail) == (1 << (32 - tail)) - 1).all() and np.array_equal(full[:, :-1], packed[:, :-1])
    assert np.array_equal(full[:, -1] & np.uint32((1 << tail) - 1), packed[:, -1]) and not (packed[:, -1] >> np.uint32(tail)).any()
    _, _, near = slu.masked_case_ref(cues, dues, r, law)
    print(f'{cues} + {dues} links, {r} RBs, {law}: {len(links)} movable links ({(links < cues).sum()} CUE), {words} words with a {tail}-bit tail, '
          f'{allowed[links].mean():.1%} allowed; {near.mean():.3%} near a threshold')
    assert near.mean() <= asu.THRESHOLD_CAP


@pytest.mark.parametrize('cues,dues,r,law', list(slu.OWN_CASES))
def test_own_cases_fit_and_stay_under_the_threshold_cap(cues, dues, r, law):
    from gym_d2d_amd import _native, assignment
    links = slu.OWN_CASES[(cues, dues, r, law)]
    lds = assignment.lds_bytes(cues + dues, r, law != 'ld2')
    own, _, near = slu.own_case_ref(cues, dues, r, law)
    print(f"'own' on {cues} + {dues} links, {r} RBs, {law}, movable {links}: LDS {lds} B, {len(links) * r} candidates per env; "
          f'{near.mean():.3%} near a threshold; own > 0 on {(own > 0).mean():.1%}')
    assert lds == slu.OWN_LDS_BYTES[(cues, dues, r, law)] <= _native.ASSIGN_MAX_LDS_BYTES
    assert near.mean() <= asu.THRESHOLD_CAP and (own > 0).any()
    if cues + dues == 2048:
        assert max(links) == 2047 and min(links) >= 1024 and len(links) * r == 256
        # evaluate() serves 2048 links under 'ld2' only: a power law takes it past the LDS a workgroup can have
        assert evu.lds_bytes(2048, r, False) <= _native.EVALUATE_MAX_LDS_BYTES < evu.lds_bytes(2048, r, True)
        rb = np.asarray(asu.case(cues, dues, r, law)['rb'])
        on = (rb >= 0) & (rb < r)
        on[:, list(links)] = False
        assert on[:, :1024].any() and on[:, 1024:].any()                # background members on both sides of link 1024


# ------------------------------------------------------------------------------------------ the matching
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('cues,dues,r,law', slu.PLANE_CASES)
def test_matchings_on_the_reference_planes_are_feasible_and_reach_the_higher_columns(cues, dues, r, law, masked):
    w, col, value, feasible = slu.plane_ref(cues, dues, r, law, masked)
    high, higher = slu.plane_conditions(w, col, feasible)
    greedy = [slu.row_greedy(w[e]) for e in range(w.shape[0])]
    print(f'{dues} x {r} ({law}), masked {masked}: feasible {feasible.tolist()}, value {value.tolist()}; matched columns >= 256: {high}, '
          f'>= 512: {higher}; row-greedy value {[round(g[1], 3) for g in greedy]}')
    for e in range(w.shape[0]):
        rows = np.arange(dues)
        assert len(set(col[e].tolist())) == dues and np.isfinite(w[e][rows, col[e]]).all()
        assert not np.array_equal(greedy[e][0], col[e]) and float(value[e]) > greedy[e][1]      # not the trivial placement


@pytest.mark.parametrize('name', list(slu.SYNTHETIC))
def test_synthetic_matchings_are_not_greedy_and_reach_the_columns_they_name(name):
    from gym_d2d_amd import _native, assignment
    m, r, seeds, lds, q_top = slu.SYNTHETIC[name]
    assert assignment.solve_lds_bytes(m, r) == asu.solve_lds_bytes(m, r) == lds <= _native.ASSIGN_MAX_LDS_BYTES
    for seed in seeds:
        w, col, value, feasible = slu.solved(name, seed)
        g_col, g_value = slu.row_greedy(w)
        top = int(col.max()) // slu.SOLVE_THREADS
        print(f'{name}, seed {seed}: LDS {lds} B, feasible {feasible}, value {float(value):.4f} against row-greedy {g_value:.4f}; highest '
              f'matched column {int(col.max())} (q = {top}); matched columns with q >= 1: {(col >= slu.SOLVE_THREADS).sum()}')
        assert feasible == 1 and len(set(col.tolist())) == m
        assert not np.array_equal(g_col, col) and float(value) > g_value
        assert top >= 1 and (seed != seeds[0] or top == q_top)
    if name == 'low rank 300 x 2600':
        assert 64 * 1024 < lds < 64 * 1024 + 1024
    if name == 'low rank 8 x 6800':
        assert slu.MAX_LDS_BYTES - 512 < lds                             # 448 bytes under the limit
    if name == 'chain of 600':
        assert np.array_equal(slu.solved(name, 0)[1], np.r_[np.arange(1, 600), 0]) and float(slu.solved(name, 0)[2]) == 600.0


def test_the_infeasible_envs_at_width_are_infeasible_by_the_restatement():
    for name, w, bad in slu.infeasible_batches():
        assert w.shape == (3, 300, 2600) and w.dtype == np.float32
        col, value, feasible = asu.solve_ref(w[bad])
        print(f'{name}: env {bad} feasible {feasible}')
        assert feasible == 0 and (col == -1).all() and float(value) == 0.0
        for e in (0, 2):                                                # the neighbours are the synthetic case's own matrices
            assert np.array_equal(w[e], slu.solved(slu.WIDE, slu.WIDE_SEEDS[e])[0])
    two = slu.infeasible_batches()[0][1][1]
    for a in slu.WIDE_ROWS:
        assert np.isfinite(two[a]).sum() == 1 and np.isfinite(two[a, -1])
    assert (2600 - 1) // slu.SOLVE_THREADS == 10


# ------------------------------------------------------------------------------------------ joint RB and power
def test_exact_power_cases_fit_and_have_the_levels_they_name():
    from gym_d2d_amd import _native, assignment
    assert apu.MAX_LEVELS == 64 == _native.ASSIGNPWR_MAX_LEVELS and apu.CHUNK == 8
    levels = {key: [hi - lo + 1 for lo, hi in bounds] for key, bounds in slu.EXACT_CASES.items()}
    assert levels == {(1024, 1024, 256, 'mixed'): [9], (13, 50, 64, 'mixed'): [64, 63]}
    assert apu.lds_bytes(2048, 256, True) == assignment.lds_bytes(2048, 256, True) == 156688 <= _native.ASSIGNPWR_MAX_LDS_BYTES
    c = asu.case(*slu.EXACT_SCATTERED)
    links, allowed = slu.masked_movable(c)
    lo, hi = apu.scattered_bounds(c, cues=700)
    assert len(links) == 343 and sorted(set((hi - lo + 1)[links].tolist())) == [18, 24] and (allowed.shape[1] + 31) // 32 == 11


@pytest.mark.parametrize('cues,dues,r,law', list(slu.FLOOR_CASES))
def test_floor_cases_stay_under_the_cap_and_choose_levels_on_both_sides_of_the_chunk(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    links = slu.floor_links(c, cues, dues, r, law)
    lo, hi = slu.FLOOR_CASES[(cues, dues, r, law)][1]
    w, valid, marks = slu.floor_case_ref(cues, dues, r, law)
    assert valid.all() and w.shape == (asu.B, len(links), r, hi - lo + 1) and np.isfinite(w).all()
    assert len(links) == (32 if cues == 1024 else 83) and (cues != 1024 or links.min() >= 1024)
    without = []
    for pair, (adm, near) in zip((None,) + apu.FLOOR_SETTINGS + ('unreachable',), marks):
        share = float(near.any(axis=3).mean())
        best, level = apu.best_power(w, valid, adm)
        chosen = np.unique(level[level >= 0])
        no_rb = float((~np.isfinite(best)).all(axis=2).mean())
        print(f'{cues} + {dues} links, {r} RBs, {law}, M = {len(links)}, floors {pair}: {share:.3%} left out, {np.isfinite(best).mean():.1%} '
              f'admissible, rows without an admissible RB {no_rb:.1%}, chosen levels {chosen.tolist()}')
        assert share <= apu.THRESHOLD_CAP
        assert chosen.min() < apu.CHUNK <= chosen.max()                 # both sides of the chunk of 8
        if pair is None:
            assert adm.all()
        else:
            assert adm.any() and not adm.all()
        without.append(no_rb)
    # a row with no admissible RB at all: none under the two FLOOR_SETTINGS on these seeds, every eighth row under the third setting
    assert without[:3] == [0.0, 0.0, 0.0] and without[3] >= 1 / 8
    shut = np.zeros(len(links), bool)
    shut[::8] = True
    best, _ = apu.best_power(w, valid, marks[3][0])
    assert (~np.isfinite(best[:, shut])).all() and np.isfinite(best[:, ~shut]).any(axis=2).all()
    if cues == 1024:
        _, level = apu.best_power(w, valid, marks[1][0])
        assert set(range(9)) <= set(np.unique(level).tolist())          # the chosen levels cover 0 .. 8


# ------------------------------------------------------------------------------------------ the colouring
@pytest.mark.parametrize('key', list(slu.COLOR_CASES), ids=lambda s: 'x'.join(map(str, s)))
def test_colour_cases_fit_and_reach_what_they_name(key):
    from gym_d2d_amd import _native, coloring
    b, n, r = key
    how, lds, _ = slu.COLOR_CASES[key]
    c = slu.color_case(*key)
    assert coloring.lds_bytes(n, r, c.allowed is not None) == cu.lds_bytes(n, r, c.allowed is not None) == lds <= _native.COLOR_MAX_LDS_BYTES
    assert (c.allowed is not None) == how['masked'] and (c.movable is not None) == how['half'] and (c.tx_bias is not None) == how['bias']
    turn = cu.turn_takers(n, r, c.movable, c.allowed)
    refs = {pack: slu.color_ref(b, n, r, pack) for pack in (False, True)}
    for pack, out in refs.items():
        print(f'{key}, pack={pack}: LDS {lds} B, {int(turn.sum())} turns; conflicts {out[1].tolist()}, rbs_used {out[2].tolist()}, proper '
              f'{out[3].tolist()}; highest chosen RB {int(out[0][:, turn].max())}')
    slu.color_reaches(key, c, turn, refs)
    if key == (1, 1024, 33):
        assert lds / _native.COLOR_MAX_LDS_BYTES > 0.977
    if key == (1, 200, 1000):
        assert lds > 64 * 1024 and cu.lds_bytes(n, 24, True) < 64 * 1024
    if key == (1, 600, 70):
        assert [int(refs[p][1][0]) for p in (False, True)] == [690, 595]


@pytest.mark.parametrize('m,r', list(slu.COMPLETE_CASES))
def test_complete_graphs_past_256_rbs_spread_evenly(m, r):
    from gym_d2d_amd import _native, coloring
    lds, conflicts = slu.COMPLETE_CASES[(m, r)]
    assert coloring.lds_bytes(m, r, False) == lds <= _native.COLOR_MAX_LDS_BYTES and r > 256 and m > r
    for pack in (False, True):
        rb, conf, used, proper = slu.complete_ref(m, r, pack)
        load = np.bincount(rb[0], minlength=r)
        print(f'K{m} on {r} RBs, pack={pack}: conflicts {int(conf[0])}, loads {load.min()} .. {load.max()}, rbs_used {int(used[0])}')
        assert load.max() - load.min() <= 1 and int(conf[0]) == sum(int(k) * (int(k) - 1) // 2 for k in load) == conflicts
        assert int(used[0]) == r and int(proper[0]) == 0 and load[256:].all()

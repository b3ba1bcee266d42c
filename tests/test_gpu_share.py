"""Exact optimal RB sharing on the GPU (csrc/d2d_share.hip; VecD2DEnv.sharing_values, solve_sharing, share_rbs, share_rbs_actions).

The value kernel has two yardsticks.  EXACT: for every (r, S) the candidate "S on r, every other movable link on no RB, the background
as it is" goes through d2d_evaluate, whose float32 capacities of the members of r are summed on the host in ascending link index in
float64 - the block must equal that word for word.  And the float64 reference share_util.values_ref at the project's 1e-5 bar,
entries with a member within 1e-4 dB of its sensitivity left out (at most 1 % of a case).  The solver has one, no tolerance: the NumPy
restatement share_util.solve_ref, col and the bits of value.  Every direct launch writes into guarded allocations (guard_util) and
is made twice.  Then the env: share_rbs() against all 729 placements of six links on three RBs scored by evaluate()."""
import numpy as np
import pytest

import share_util as shu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _dev(a):
    return torch.as_tensor(np.array(a, order='C'), device='cuda')       # a copy: the cases' arrays are read-only


def _case_inputs(c):
    return [_dev(a) for a in (c['pos'][..., 0].astype(np.float32), c['pos'][..., 1].astype(np.float32), c['tx'], c['rx'], c['cols'], c['cap_cols'])]


def _launch_values(c, links, allowed=None, pwr=None):
    """d2d_share_values on the uploaded case; (values float64 [B, R, 2^M], closed_rb int32 [B, R]) on the host, the guards checked."""
    from guard_util import Guarded
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response import pack_allowed
    px, py, tx, rx, cols, cap_cols = _case_inputs(c)
    b, n, r, m = c['b'], c['n'], c['r'], len(links)
    rb_t, pwr_t, links_t = _dev(np.asarray(c['rb'], dtype=np.int32)), _dev(np.asarray(c['pwr'] if pwr is None else pwr, dtype=np.int32)), _dev(links)
    words = None if allowed is None else _dev(pack_allowed(allowed))
    values, closed = Guarded((b, r, 1 << m), torch.float64), Guarded((b, r), torch.int32)
    before = _native.share_values_launches
    _native.share_values(px.data_ptr(), py.data_ptr(), rb_t.data_ptr(), pwr_t.data_ptr(), tx.data_ptr(), rx.data_ptr(), cols.data_ptr(),
                         cap_cols.data_ptr(), c['kind'], c['pow_k'], b, c['d'], n, r, links_t.data_ptr(), m,
                         0 if words is None else words.data_ptr(), values.array.data_ptr(), closed.array.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.share_values_launches == before + 1
    assert values.intact() and closed.intact()
    return values.array.cpu().numpy().copy(), closed.array.cpu().numpy().copy()


def _evaluate_capacity(c, rb, pwr):
    """d2d_evaluate's float32 capacity plane [B, K, N] of candidate planes."""
    from gym_d2d_amd import _native
    px, py, tx, rx, cols, cap_cols = _case_inputs(c)
    b, k, n = rb.shape
    rb_t, pwr_t = _dev(rb), _dev(pwr)
    cap = torch.empty((b, k, n), dtype=torch.float32, device='cuda')
    total = torch.empty((b, k), dtype=torch.float32, device='cuda')
    _native.evaluate(px.data_ptr(), py.data_ptr(), rb_t.data_ptr(), pwr_t.data_ptr(), tx.data_ptr(), rx.data_ptr(), cols.data_ptr(),
                     cap_cols.data_ptr(), c['kind'], c['pow_k'], b, k, c['d'], n, c['r'], 0, cap.data_ptr(), total.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return cap.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _forbidden(links, allowed, r):
    """bool [R, 2^M]: subset S holds a link that is not allowed on r."""
    m = len(links)
    mask = np.array([sum(1 << a for a in range(m) if not allowed[links[a], layer]) for layer in range(r)])
    return (np.arange(1 << m)[None, :] & mask[:, None]) != 0


@pytest.mark.parametrize('law', shu.LAWS)
@pytest.mark.parametrize('name', list(shu.VALUE_CASES))
def test_values_equal_evaluate_word_for_word_and_the_float64_reference_at_the_bar(name, law):
    c, links, allowed, other = shu.value_case(name, law)
    b, n, r, m = c['b'], c['n'], c['r'], len(links)
    ref, ref_closed, near = shu.values_ref(c, links)
    got, closed = _launch_values(c, links)
    again, _ = _launch_values(c, links)
    assert np.array_equal(_bits(got), _bits(again))                     # two calls give the same words
    assert np.array_equal(closed, ref_closed) and set(np.unique(closed).tolist()) <= {0, 1}
    # exact: evaluate()'s capacities of the members of r, summed in ascending link index in float64
    rb_c, pwr_c = shu.candidates(c, links)
    want = shu.values_from_capacity(_evaluate_capacity(c, rb_c, pwr_c), rb_c, r, m)
    shut = np.broadcast_to((closed == 1)[:, :, None], want.shape) & (np.arange(1 << m) != 0)[None, None, :]
    want[shut] = -np.inf                                                # a closed RB: -inf rows, the true S = 0 entry
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    assert np.isfinite(got[~shut]).all() and (got[~shut] >= 0).all() and (got[:, :, 0] <= got.max(axis=2)).all()
    # the float64 reference at the bar
    fin = np.isfinite(ref) & ~near
    err = float((np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1.0)).max())
    assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and near.mean() <= shu.THRESHOLD_CAP
    # allowed, with a link allowed nowhere, and other powers for every link
    masked, _ = _launch_values(c, links, allowed, other)
    rb_c, pwr_c = shu.candidates(c, links, other)
    want = shu.values_from_capacity(_evaluate_capacity(c, rb_c, pwr_c), rb_c, r, m)
    want[shut] = -np.inf
    want[np.broadcast_to(_forbidden(links, allowed, r)[None], want.shape)] = -np.inf
    assert np.array_equal(_bits(masked), _bits(want))
    assert np.isneginf(masked[:, :, 1 << (m // 2)]).all() and np.isfinite(masked[:, :, 0]).all()
    ref2 = shu.values_ref(c, links, allowed, other)[0]
    fin2 = np.isfinite(ref2)
    err2 = float((np.abs(masked[fin2] - ref2[fin2]) / np.maximum(np.abs(ref2[fin2]), 1.0)).max())
    print(f'{name}, {law}: {b} x {n} links x {r} RBs, M = {m}: equal to evaluate(); rel_err against float64 {err:.3e} '
          f'({err2:.3e} under other powers); closed {closed.sum(axis=1).tolist()}; {near.mean():.2%} near a threshold')
    assert err <= shu.BAR
    if name == 'closed':
        assert closed.tolist() == [[0, 1, 0, 0, 0, 0, 0]] * 2 and (got[:, 2, 0] == 0.0).all() and (got[:, 1, 0] > 0).all()


# ------------------------------------------------------------------------------------------------ the solver
def _launch_solve(values, quota):
    """d2d_share_solve on an uploaded block; (col, value, feasible) on the host, the guards checked."""
    from guard_util import Guarded
    from gym_d2d_amd import _native
    b, r, nt = values.shape
    m = nt.bit_length() - 1
    v = _dev(values)
    q = None if quota is None else _dev(np.broadcast_to(np.asarray(quota, dtype=np.int32), (r,)))
    choice = Guarded((b, r, nt), torch.int16)
    col, value, feasible = Guarded((b, m), torch.int32), Guarded((b,), torch.float64), Guarded((b,), torch.int32)
    before = _native.share_solve_launches
    _native.share_solve(v.data_ptr(), 0 if q is None else q.data_ptr(), b, r, m, choice.array.data_ptr(), col.array.data_ptr(),
                        value.array.data_ptr(), feasible.array.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.share_solve_launches == before + 1
    for g, what in ((choice, 'choice'), (col, 'col'), (value, 'value'), (feasible, 'feasible')):
        assert g.intact(), f'guard bands of {what}'
    return tuple(g.array.cpu().numpy().copy() for g in (col, value, feasible))


@pytest.mark.parametrize('name', list(shu.SOLVE_CASES))
def test_solver_equals_the_restatement_word_for_word(name):
    from gym_d2d_amd import sharing
    b, r, m, kind, _ = shu.SOLVE_CASES[name]
    values, quota = shu.solve_case(name)
    want = shu.solve_case_ref(name)
    got = _launch_solve(values, quota)
    again = _launch_solve(values, quota)
    print(f'{name}: {b} x {r} RBs x 2^{m}, {kind}, quota {quota}: feasible {int(want[2].sum())} of {b}, value {want[1][:3].tolist()}; '
          f'LDS {sharing.solve_lds_bytes(m)} bytes')
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[2], want[2])
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))       # two calls give the same words
    if name == 'limit':
        assert sharing.solve_lds_bytes(m) > 64 * 1024                   # the dynamic-LDS attribute was needed
    if name == 'dead_between':
        assert got[2].tolist() == [1, 0, 1] and (got[0][1] == -1).all() and _bits(got[1][1]) == 0


# ------------------------------------------------------------------------------------------------ through the env
def _env(cues, dues, rbs, b=4, seed=3, step=True, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': rbs, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b, **kw)
    env.reset(seed=seed)
    if step:
        env.step(_random_actions(env, np.random.default_rng(seed)))
    return env


def _random_actions(env, rng):
    return torch.as_tensor(np.stack([rng.integers(0, h, env.num_envs) for h in env._initial_action_highs()], axis=1).astype(np.int32),
                           device=env.device)


def _totals(env, rb):
    """evaluate()'s float32 totals of candidate planes rb [B, K, N] at the current powers."""
    b, k, n = rb.shape
    pwr = env._t['pwr'].unsqueeze(1).expand(b, k, n).contiguous()
    return env.evaluate(rb.contiguous(), pwr, planes=())['total_mbps'].cpu().numpy()


def _within_one_ulp(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def test_share_rbs_reaches_the_best_of_all_729_placements():
    import itertools
    from gym_d2d_amd import _native
    env = _env(8, 6, 3)
    try:
        b, n, r, m = env.num_envs, env.num_links, env.config.num_rbs, 6
        cur = env._t['rb'].clone()
        launches = _native.share_values_launches, _native.share_solve_launches
        res = env.share_rbs()
        assert (_native.share_values_launches, _native.share_solve_launches) == (launches[0] + 1, launches[1] + 1)
        assert res._fields == ('rb', 'value_mbps', 'feasible', 'closed')
        assert [x.dtype for x in res] == [torch.int32, torch.float32, torch.int32, torch.int32]
        rb, value, feasible, closed = (x.clone() for x in res)
        assert torch.equal(env._t['rb'], cur) and env.status_flags() == 0                      # the env is untouched
        assert feasible.tolist() == [1] * b and closed.tolist() == [0] * b and torch.equal(rb[:, :8], cur[:, :8])
        links = np.arange(8, 14)
        placements = np.array(list(itertools.product(range(r), repeat=m)), dtype=np.int32)      # [729, 6]
        cand = cur.cpu().numpy()[:, None, :].repeat(len(placements), axis=1)
        cand[:, :, links] = placements[None]
        scores = _totals(env, torch.as_tensor(cand, device=env.device))
        reached = _totals(env, rb.unsqueeze(1))[:, 0]
        print(f'optimum {value.tolist()} Mbps; evaluate(rb) {reached.tolist()}; best of 729 {scores.max(axis=1).tolist()}; '
              f'median placement {np.median(scores, axis=1).tolist()}')
        # the two double sums differ only in association, and each is rounded once to float32
        assert _within_one_ulp(reached, scores.max(axis=1)).all()
        assert _within_one_ulp(value.cpu().numpy(), reached).all()
        # the two launches alone, with out=, give the same words
        block = env.sharing_values()
        assert block._fields == ('values', 'links', 'closed') and block.links.tolist() == links.tolist()
        assert tuple(block.values.shape) == (b, r, 64) and block.values.dtype == torch.float64
        out = (torch.empty((b, m), dtype=torch.int32, device=env.device), torch.empty(b, dtype=torch.float64, device=env.device),
               torch.empty(b, dtype=torch.int32, device=env.device))
        solved = env.solve_sharing(block.values, out=out)
        assert solved._fields == ('col', 'value', 'feasible') and all(x is y for x, y in zip(solved, out))
        assert torch.equal(out[0], rb[:, 8:]) and torch.equal(out[1].float(), value)
        want = shu.solve_ref(block.values.cpu().numpy())
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(_bits(out[1].cpu().numpy()), _bits(want[1]))
        # quota 2: at most two links per RB, still the best of the placements that keep it
        rb2, value2 = (x.clone() for x in env.share_rbs(quota=2)[:2])
        keeps = np.array([np.bincount(p, minlength=r).max() <= 2 for p in placements])
        assert all(np.bincount(row, minlength=r).max() <= 2 for row in rb2[:, 8:].cpu().numpy())
        assert _within_one_ulp(_totals(env, rb2.unsqueeze(1))[:, 0], scores[:, keeps].max(axis=1)).all()
        assert (value2 <= value).all()
        # an allowed mask that leaves a movable link no RB: every env keeps its row
        shutout = np.ones((n, r), bool)
        shutout[9] = False
        kept = env.share_rbs(allowed=shutout)
        assert kept.feasible.tolist() == [0] * b and torch.equal(kept.rb, cur) and (kept.value_mbps == 0).all()
        # the actions put the step on the solved RBs at the current powers
        keep = env._t['pwr'].clone()
        _, _, _, info = env.step(env.share_rbs_actions())
        assert torch.equal(info['rb'], rb) and torch.equal(env._t['pwr'], keep)
    finally:
        env.close()


def test_quota_one_agrees_with_the_one_to_one_matching():
    env = _env(5, 4, 6, seed=7)
    try:
        shared = env.share_rbs(quota=1)
        rb_s, value = shared.rb.clone(), shared.value_mbps.clone()
        rb_a = env.assign_rbs().rb.clone()
        t_s, t_a = _totals(env, rb_s.unsqueeze(1))[:, 0].astype(np.float64), _totals(env, rb_a.unsqueeze(1))[:, 0].astype(np.float64)
        print(f'share_rbs(quota=1) {t_s.tolist()} Mbps, assign_rbs() {t_a.tolist()} Mbps')
        assert all(len(set(row)) == 4 for row in rb_s[:, 5:].tolist())
        assert (np.abs(t_s - t_a) <= 1e-5 * np.maximum(np.abs(t_a), 1.0)).all()
        assert _within_one_ulp(value.cpu().numpy(), t_s).all()
        assert (env.share_rbs().value_mbps >= value).all()              # sharing allowed can only do better
    finally:
        env.close()


def test_an_infeasible_env_between_two_feasible_ones_keeps_its_row():
    """132 CUEs and 4 pairs on 3 RBs, RB 2 closed to movable links by its quota: envs 0 and 2 have 44 CUEs per RB; env 1 has 66 on
    RB 0 and 66 on RB 1, past the 64 background members an RB may have and take movable links."""
    env = _env(132, 4, 3, b=3, step=False)
    try:
        highs = np.asarray(env._initial_action_highs())
        levels = highs // 3
        want = np.zeros((3, 136), dtype=np.int64)
        want[:, :132] = np.arange(132) % 3
        want[1, :132] = np.arange(132) % 2
        want[:, 132:] = 2
        env.step(torch.as_tensor((want * levels[None, :]).astype(np.int32), device=env.device))
        cur = env._t['rb'].clone()
        assert np.array_equal(cur.cpu().numpy(), want)
        res = env.share_rbs(quota=[4, 4, 0])
        assert res.feasible.tolist() == [1, 0, 1] and res.closed.tolist() == [0, 2, 0]
        assert torch.equal(res.rb[1], cur[1]) and float(res.value_mbps[1]) == 0.0 and (res.rb[[0, 2], 132:] < 2).all()
        assert torch.equal(res.rb[:, :132], cur[:, :132])
        assert _within_one_ulp(res.value_mbps.cpu().numpy()[[0, 2]], _totals(env, res.rb.clone().unsqueeze(1))[[0, 2], 0]).all()
        values = env.sharing_values().values
        assert torch.isneginf(values[1, :2, 1:]).all() and torch.isfinite(values[1, :, 0]).all() and torch.isfinite(values[[0, 2]]).all()
    finally:
        env.close()


@pytest.mark.parametrize('autoreset', [False, True])
def test_in_lockstep_and_after_autoreset_steps_the_result_is_the_optimum_of_the_current_planes(autoreset):
    import itertools
    from gym_d2d_amd.mobility import GaussMarkovMobility
    kw = dict(autoreset=True, mobility=GaussMarkovMobility(speed_std_mps=8.0, memory=0.7)) if autoreset else {}
    env = _env(4, 4, 3, b=5, step=False, **kw)
    try:
        b, n, r, m = 5, 8, 3, 4
        rng = np.random.default_rng(6)
        if autoreset:
            env.reset(seed=21, elapsed=np.arange(b) % 10)
        placements = np.array(list(itertools.product(range(r), repeat=m)), dtype=np.int32)
        resets = 0
        for _ in range(12 if autoreset else 3):
            _, _, _, info = env.step(_random_actions(env, rng))
            resets += int(info['reset'].sum()) if autoreset else 0
            res = env.share_rbs()
            rb, value = res.rb.clone(), res.value_mbps.clone()
            cand = env._t['rb'].cpu().numpy()[:, None, :].repeat(len(placements), axis=1)
            cand[:, :, 4:] = placements[None]
            best = _totals(env, torch.as_tensor(cand, device=env.device)).max(axis=1)
            assert _within_one_ulp(_totals(env, rb.unsqueeze(1))[:, 0], best).all() and _within_one_ulp(value.cpu().numpy(), best).all()
        print(f'autoreset {autoreset}: {resets} env resets')
        assert resets >= b or not autoreset
    finally:
        env.close()

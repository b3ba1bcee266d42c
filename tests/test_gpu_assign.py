"""Optimal one-to-one RB matching on the GPU (VecD2DEnv.assignment_weights / solve_assignment / assign_rbs, csrc/d2d_assign.hip).

Direct launches of the weights kernel against assign_util.weights_ref, the float64 reference test_assign_cpu.py ties to
evaluate_util.evaluate_ref through the separability identity; the bar is the project's 1e-5 (|d| <= 1e-5 max(|ref|, 1)) on weights
and harm (Mbps), entries near a threshold left out, at most 1 % of a case (asserted on the reference alone in test_assign_cpu.py:
none in any case here).  Under objective 'own' the plane is evaluate()'s capacity_mbps bit for bit.  Direct launches of the matching
kernel against assign_util.solve_ref: col, feasible and the bits of value are equal.  Then the env: the placement, the identity
against evaluate(), optimality against the float64 optimum, and the refusals.  Every test prints what it measured.

Measured on an MI355X: weights rel_err 1.0e-8 - 5.8e-7, harm 4.1e-10 - 1.7e-7, own 1.0e-8 - 2.6e-7 over the eight cases; own equals
evaluate()'s capacity on 100 % of 35 and 3200 candidates per env; evaluate(rb) = background + value_mbps to 3.5e-8; no shortfall against
the float64 optimum (CHANGELOG.md)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest

import assign_util as asu
import evaluate_util as evu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
GUARD, PAD = 0x5AFEC0DE, 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev():
    return torch.device('cuda', 0)


_inputs = {}


def _device_inputs(c):
    """The device tensors of a case, uploaded once per case."""
    key = id(c['pos'])
    if c.get('fresh') or key not in _inputs:                            # fresh: the state of a live env, never cached
        _inputs[key] = [torch.as_tensor(np.ascontiguousarray(a), device=_dev()) for a in
                        (c['pos'][..., 0].astype(np.float32), c['pos'][..., 1].astype(np.float32), c['rb'], c['pwr'], c['tx'], c['rx'],
                         c['cols'], c['cap_cols'])]
    return _inputs[key]


def _launch_weights(c, links, allowed=None, objective=0, harm=True, shift=0):
    """One d2d_assign_weights launch with both planes inside guard words; shift: words (4 bytes each) by which the output pointers
    are moved off their 256-byte alignment; allowed: bool [N, R], or the packed uint32 words [N, ceil(R / 32)] themselves.  Returns
    (weights, harm) [B, M, R] as host arrays, harm None if not asked for."""
    from gym_d2d_amd import _native
    from gym_d2d_amd.best_response import pack_allowed
    px, py, rb, pwr, tx, rx, cols, cap_cols = _device_inputs(c)
    b, n, r, m = c['b'], c['n'], c['r'], len(links)
    links_t = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32), device=_dev())
    packed = None if allowed is None else allowed if allowed.dtype == np.uint32 else pack_allowed(allowed)
    assert packed is None or packed.shape == (n, (r + 31) // 32)
    words_t = None if packed is None else torch.as_tensor(np.ascontiguousarray(packed).view(np.int32), device=_dev())
    words = b * m * r
    o_w, o_h = PAD + shift, 2 * PAD + words + shift
    arena = torch.full((2 * words + 3 * PAD + shift,), GUARD, dtype=torch.int32, device=_dev())
    base = arena.data_ptr()
    _native.assign_weights(px.data_ptr(), py.data_ptr(), rb.data_ptr(), pwr.data_ptr(), tx.data_ptr(), rx.data_ptr(), cols.data_ptr(),
                           cap_cols.data_ptr(), c['kind'], c['pow_k'], b, c['d'], n, r, links_t.data_ptr(), m,
                           0 if words_t is None else words_t.data_ptr(), objective, base + 4 * o_w, base + 4 * o_h if harm else 0,
                           torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    host = arena.cpu().numpy()
    live = np.zeros(host.shape, bool)
    live[o_w:o_w + words] = True
    if harm:
        live[o_h:o_h + words] = True
    assert (host[~live] == GUARD).all()                                 # the guard words, and a plane that was not asked for, untouched
    f = host.view(np.float32)
    return f[o_w:o_w + words].reshape(b, m, r).copy(), f[o_h:o_h + words].reshape(b, m, r).copy() if harm else None


def _launch_solve(w, shift=0):
    """One d2d_assign_solve launch on host weights [B, M, R] with the three outputs inside guard words (feasible: guard BYTES).
    Returns (col int32 [B, M], value float32 [B], feasible uint8 [B])."""
    from gym_d2d_amd import _native
    w = np.ascontiguousarray(w, dtype=np.float32)
    b, m, r = w.shape
    w_t = torch.as_tensor(w, device=_dev())
    o_c, o_v, o_f = PAD + shift, 2 * PAD + b * m + shift, 3 * PAD + b * m + b + shift
    arena = torch.full((4 * PAD + b * m + b + (b + 3) // 4 + shift,), GUARD, dtype=torch.int32, device=_dev())
    base = arena.data_ptr()
    _native.assign_solve(w_t.data_ptr(), b, m, r, base + 4 * o_c, base + 4 * o_v, base + 4 * o_f + shift,      # feasible: odd bytes too
                         torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    raw = host.view(np.uint8)
    live = np.zeros(raw.shape, bool)
    live[4 * o_c:4 * (o_c + b * m)] = True
    live[4 * o_v:4 * (o_v + b)] = True
    live[4 * o_f + shift:4 * o_f + shift + b] = True
    assert np.array_equal(raw[~live], np.full(host.shape, GUARD, dtype=np.int32).view(np.uint8)[~live])
    return (host[o_c:o_c + b * m].reshape(b, m).copy(), host.view(np.float32)[o_v:o_v + b].copy(),
            raw[4 * o_f + shift:4 * o_f + shift + b].copy())


def _planes_err(got_w, got_h, own, harm, near):
    keep = ~near
    return asu.evu.rel_err(got_w[keep], (own - harm)[keep]), asu.evu.rel_err(got_h[keep], harm[keep])


# ------------------------------------------------------------------------------------------------ the weights kernel
@pytest.mark.parametrize('cues,dues,r,law', asu.WEIGHT_CASES)
def test_weights_against_the_float64_reference(cues, dues, r, law):
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    own, harm, near = asu.case_ref(cues, dues, r, law)
    w, h = _launch_weights(c, links)
    assert np.isfinite(w).all() and np.isfinite(h).all()
    e_w, e_h = _planes_err(w, h, own, harm, near)
    left_out = float(near.mean())
    print(f'{cues} + {dues} links, {r} RBs, {law}: weights rel_err {e_w:.3e}, harm rel_err {e_h:.3e}; {left_out:.2%} left out at a '
          f'threshold; {(own - harm < 0).mean():.1%} of the weights negative; LDS {asu.lds_bytes(cues + dues, r, law != "ld2")} B')
    assert left_out <= asu.THRESHOLD_CAP
    assert e_w <= asu.BAR
    assert e_h <= asu.BAR
    rb = np.asarray(c['rb'])[:, :cues]
    for e in range(c['b']):                                             # 0.0 exactly on the RBs without background members
        empty = np.setdiff1d(np.arange(r), rb[e][(rb[e] >= 0) & (rb[e] < r)])
        assert (_bits(h[e][:, empty]) == 0).all()
    # the own plane: the same launch under objective 'own', no harm plane; weights = own - harm rounded once
    o, none = _launch_weights(c, links, objective=1, harm=False)
    assert none is None
    e_o = evu.rel_err(o[~near], own[~near])
    print(f'    own rel_err {e_o:.3e}')
    assert e_o <= asu.BAR
    # w is (own - harm) rounded once from the double sum behind the float32 harm plane: two float32 roundings apart at the most
    o64, h64 = o.astype(np.float64), h.astype(np.float64)
    assert (np.abs(w - (o64 - h64)) <= 2.0 ** -22 * (np.abs(o64) + np.abs(h64))).all()


def test_a_second_launch_and_a_moved_pointer_give_the_same_bits():
    cues, dues, r, law = 57, 200, 259, 'ld35'
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues)
    first = _launch_weights(c, links)
    for other in (_launch_weights(c, links), _launch_weights(c, links, shift=1)):
        for a, m in zip(first, other):
            assert np.array_equal(_bits(a), _bits(m))
    total_only = _launch_weights(c, links, harm=False)                  # a null harm plane: the weights do not change
    assert total_only[1] is None and np.array_equal(_bits(total_only[0]), _bits(first[0]))


def test_scattered_movable_links_and_allowed():
    """Movable links that mix CUE and DUE links, about 30 % of the entries forbidden: -inf exactly there, the reference elsewhere;
    harm is written where forbidden too."""
    c = asu.case(*asu.SCATTERED)
    links, allowed = asu.scattered_movable(c)
    own, harm, near = asu.scattered_ref()
    w, h = _launch_weights(c, links, allowed=allowed)
    free = np.broadcast_to(allowed[links][None], w.shape)
    assert (w[~free] == -np.inf).all() and np.isfinite(w[free]).all() and np.isfinite(h).all()
    keep = free & ~near
    e_w, e_h = evu.rel_err(w[keep], (own - harm)[keep]), evu.rel_err(h[~near], harm[~near])
    print(f'scattered: {len(links)} movable links ({(links < 13).sum()} CUE), {(~free).mean():.1%} forbidden; weights rel_err {e_w:.3e}, '
          f'harm rel_err {e_h:.3e}; {near.mean():.2%} left out')
    assert near.mean() <= asu.THRESHOLD_CAP and e_w <= asu.BAR and e_h <= asu.BAR
    # a link index outside [0, N): a row of -inf, harm 0.0, nothing else touched (the guards are checked by the launch)
    odd = np.r_[links[:3], c['n'], -1].astype(np.int32)
    w2, h2 = _launch_weights(c, odd, allowed=allowed)
    w3, h3 = _launch_weights(c, links[:3], allowed=allowed)              # the same three movable links, the rest background
    assert np.array_equal(_bits(w2[:, :3]), _bits(w3)) and np.array_equal(_bits(h2[:, :3]), _bits(h3)) and (w2[:, 3:] == -np.inf).all() and (_bits(h2[:, 3:]) == 0).all()


def _own_weights_are_evaluates_capacity(cues, dues, r, law, links=None):
    """Candidate (a, r): link a on r, the background where it is, every other movable link on rb -1.  links: the movable links,
    ascending (None: the DUE links)."""
    from gym_d2d_amd import _native
    c = asu.case(cues, dues, r, law)
    links = asu.due_links(c, cues) if links is None else np.asarray(links, dtype=np.int32)
    m, b, n = len(links), c['b'], c['n']
    own, _ = _launch_weights(c, links, objective=1, harm=False)
    rb = np.repeat(asu.background_candidate(c, links)[:, None, :], m * r, axis=1)            # [B, M R, N]
    a_idx, r_idx = np.divmod(np.arange(m * r), r)
    rb[:, np.arange(m * r), links[a_idx]] = r_idx
    pwr = np.repeat(np.asarray(c['pwr'], dtype=np.int32)[:, None, :], m * r, axis=1)
    px, py, _, _, tx, rx, cols, cap_cols = _device_inputs(c)
    rb_t, pwr_t = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=_dev()) for a in (rb, pwr))
    cap = torch.empty((b, m * r, n), dtype=torch.float32, device=_dev())
    total = torch.empty((b, m * r), dtype=torch.float32, device=_dev())
    _native.evaluate(px.data_ptr(), py.data_ptr(), rb_t.data_ptr(), pwr_t.data_ptr(), tx.data_ptr(), rx.data_ptr(), cols.data_ptr(),
                     cap_cols.data_ptr(), c['kind'], c['pow_k'], b, m * r, c['d'], n, r, 0, cap.data_ptr(), total.data_ptr(),
                     torch.cuda.current_stream(_dev()).cuda_stream)
    torch.cuda.synchronize()
    want = cap.cpu().numpy()[:, np.arange(m * r), links[a_idx]].reshape(b, m, r)
    same = _bits(own) == _bits(want)
    print(f'{cues} + {dues} links, {r} RBs, {law}: {m * r} candidates per env, {same.mean():.2%} of the own weights equal '
          f"evaluate()'s capacity bit for bit; {(want > 0).mean():.1%} above the sensitivity")
    assert same.all()
    return own


@pytest.mark.parametrize('cues,dues,r,law', asu.TIE_CASES)
def test_own_weights_are_evaluates_capacity_bit_for_bit(cues, dues, r, law):
    _own_weights_are_evaluates_capacity(cues, dues, r, law)


# ------------------------------------------------------------------------------------------------ the matching kernel
def _check_solve(w, name):
    """col, feasible and the bits of value of every env equal solve_ref's."""
    col, value, feasible = _launch_solve(w)
    steps = 0
    for e in range(w.shape[0]):
        rc, rv, rf = asu.solve_ref(w[e])
        assert feasible[e] == rf, (name, e)
        assert np.array_equal(col[e], rc), (name, e, np.nonzero(col[e] != rc)[0][:8])
        assert _bits(value[e]) == _bits(rv), (name, e, value[e], rv)
        steps += 1
    print(f'{name}: {w.shape[0]} envs x {w.shape[1]} x {w.shape[2]}, feasible {feasible.tolist()}, value {value.tolist()[:3]}')
    return col, value, feasible


@pytest.mark.parametrize('m,r', asu.SOLVE_SHAPES)
def test_matching_equals_the_restatement(m, r):
    w = np.stack([asu.solve_case_ref(m, r)[0], asu.solve_matrix(m, r, seed=1)])
    col, value, feasible = _check_solve(w, f'{m} x {r}')
    assert feasible.all() and all(len(set(row)) == m for row in col.tolist())
    if (m, r) == (64, 65):                                              # moved pointers (feasible by one byte too): the same bits
        moved = _launch_solve(w, shift=1)
        assert np.array_equal(moved[0], col) and np.array_equal(_bits(moved[1]), _bits(value)) and np.array_equal(moved[2], feasible)


def test_matching_with_ties_a_chain_and_what_cannot_be_matched():
    rng = np.random.default_rng(2)
    _check_solve(rng.integers(0, 4, (2, 100, 100)).astype(np.float32), 'integer weights in 0 .. 3')
    col, value, _ = _check_solve(asu.chain_matrix(65)[None], 'the chain')
    assert np.array_equal(col[0], np.r_[np.arange(1, 65), 0]) and value[0] == 65.0
    # B = 3 with the middle env infeasible: two rows that can only take the same column
    w = np.stack([asu.solve_matrix(6, 9, seed=s) for s in range(3)])
    w[1, 2], w[1, 4] = -np.inf, -np.inf
    w[1, 2, 5], w[1, 4, 5] = 1.0, 2.0
    col, value, feasible = _check_solve(w, 'the middle env infeasible')
    assert feasible.tolist() == [1, 0, 1] and (col[1] == -1).all() and _bits(value[1]) == 0
    # a row of all -inf
    w = asu.solve_matrix(5, 70, seed=3)[None].copy()
    w[0, 3] = -np.inf
    col, value, feasible = _check_solve(w, 'a row of -inf')
    assert feasible.tolist() == [0] and (col == -1).all()
    # NaN entries are never matched; a matrix of NaN is infeasible
    w = np.stack([asu.solve_matrix(40, 70, seed=4), np.full((40, 70), np.nan, dtype=np.float32)])
    w[0][rng.random((40, 70)) < 0.3] = np.nan
    col, value, feasible = _check_solve(w, 'NaN entries')
    assert feasible.tolist() == [1, 0] and np.isfinite(w[0][np.arange(40), col[0]]).all()


# ------------------------------------------------------------------------------------------------ through the env
ENVS = {'small': ({'num_rbs': 8, 'num_cues': 4, 'num_due_pairs': 6}, 5), 'config2': ({'num_rbs': 25, 'num_cues': 25, 'num_due_pairs': 25}, 3),
        # 280 movable links on 300 RBs: a matching thread owns two columns, and the host packs a 10-word `allowed` with a 12-bit tail
        'wide': ({'num_rbs': 300, 'num_cues': 150, 'num_due_pairs': 280}, 2)}


def _env(name, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    cfg, b = ENVS[name]
    return VecD2DEnv(dict(cfg), num_envs=b, **kw)


def _env_case(env):
    """The env's current state as a case of read_side_util: float64 references on the positions and planes the kernels read."""
    from gym_d2d_amd.device import link_budget_columns
    sim = env.simulator
    torch.cuda.synchronize()
    law = sim.path_loss_table.law
    pos = np.stack([env._t['pos_x'].cpu().numpy(), env._t['pos_y'].cpu().numpy()], axis=-1).astype(np.float64)
    return dict(b=env.num_envs, n=env.num_links, r=env.config.num_rbs, pos=pos, tx=np.asarray(sim.link_tx), rx=np.asarray(sim.link_rx),
                rb=env._t['rb'].cpu().numpy(), pwr=env._t['pwr'].cpu().numpy(),
                ocols=SimpleNamespace(**link_budget_columns(sim._dev_list)),
                law_cols={k: np.asarray(law[k], dtype=np.float64) for k in ('a_tx_db', 'a_rx_db', 'exponent')})


def _snapshot(env):
    t = env._t
    names = [k for k in ('rb', 'pwr', 'pos_x', 'pos_y', 'reward', 'sinr_db', 'capacity_mbps', 'elapsed', 'env_flags') if t.get(k) is not None]
    torch.cuda.synchronize()
    return {k: t[k].clone() for k in names}, env.num_steps


def _random_placement(rng, links, r, allowed):
    """A random one-to-one placement of the links inside allowed (None: anywhere): links in random order, each on a random free RB
    it may take; the rotated diagonal the masked tests keep allowed if that gets stuck."""
    if allowed is None:
        return rng.permutation(r)[:len(links)]
    cols, free = np.full(len(links), -1), np.ones(r, bool)
    for a in rng.permutation(len(links)):
        options = np.nonzero(free & allowed[links[a]])[0]
        if not len(options):
            return links % r
        cols[a] = rng.choice(options)
        free[cols[a]] = False
    return cols


def _background_mbps(env, rb, links):
    """evaluate() of the background state: the movable links on rb -1, the capacities of the background links summed in double."""
    off = rb.clone()
    off[:, links] = -1
    cap = env.evaluate(off.unsqueeze(1).contiguous(), env._t['pwr'].unsqueeze(1).contiguous(), planes=('capacity_mbps',))['capacity_mbps']
    cap = cap[:, 0].cpu().numpy().astype(np.float64)
    return np.delete(cap, links.cpu().numpy(), axis=1).sum(axis=1)


@pytest.mark.parametrize('name', list(ENVS))
@pytest.mark.parametrize('masked', [False, True])
def test_assign_rbs_is_the_optimal_one_to_one_placement(name, masked):
    from gym_d2d_amd import _native
    env = _env(name)
    try:
        b, n, r = env.num_envs, env.num_links, env.config.num_rbs
        rng = np.random.default_rng(5 + masked)
        env.reset(seed=3)
        env.step(torch.as_tensor(np.stack([rng.integers(0, h, b) for h in env._initial_action_highs()], axis=1).astype(np.int32),
                                 device=env.device))
        allowed = None
        if masked:
            allowed = rng.random((n, r)) < 0.6
            allowed[np.arange(n), np.arange(n) % r] = True               # a complete matching stays
        before, steps = _snapshot(env)
        launches = _native.assign_weights_launches, _native.assign_solve_launches
        res = env.assign_rbs(allowed=allowed)
        assert (_native.assign_weights_launches, _native.assign_solve_launches) == (launches[0] + 1, launches[1] + 1)
        assert res._fields == ('rb', 'value_mbps', 'feasible')
        rb, value, feasible = (x.clone() for x in res)
        after, steps_after = _snapshot(env)
        assert steps_after == steps and set(after) == set(before)
        for key in before:                                              # the env is untouched
            assert torch.equal(before[key], after[key]), key
        assert env.status_flags() == 0
        links = np.arange(env.num_cues, n)
        rb_h, cur = rb.cpu().numpy(), before['rb'].cpu().numpy()
        assert feasible.cpu().numpy().tolist() == [1] * b
        assert np.array_equal(rb_h[:, :env.num_cues], cur[:, :env.num_cues])                   # the background stays
        cols = rb_h[:, links]
        assert ((cols >= 0) & (cols < r)).all() and all(len(set(row)) == len(links) for row in cols.tolist())
        if masked:
            assert allowed[links[None, :], cols].all()
        # the identity against evaluate(): total(rb) = background + value_mbps
        pwr = env._t['pwr'].unsqueeze(1).contiguous()
        total = env.evaluate(rb.unsqueeze(1).contiguous(), pwr, planes=())['total_mbps'][:, 0].cpu().numpy().astype(np.float64)
        background = _background_mbps(env, before['rb'], torch.as_tensor(links, device=env.device))
        e_id = float(np.abs((background + value.cpu().numpy().astype(np.float64)) / total - 1.0).max())
        # optimality against the float64 reference of the same state
        c = _env_case(env)
        own, harm, near = asu.weights_ref(c, links)
        w_ref = np.where(np.broadcast_to(allowed[links][None], own.shape), own - harm, -np.inf) if masked else own - harm
        delta = asu.BAR * np.maximum(np.abs(own - harm), 1.0)
        slack_used = []
        for e in range(b):
            best = asu.solve_ref(w_ref[e])[0]
            rows = np.arange(len(links))
            got64, best64 = w_ref[e][rows, cols[e]].sum(), w_ref[e][rows, best].sum()
            slack = (delta[e][rows, cols[e]] + delta[e][rows, best]).sum()
            slack_used.append((best64 - got64) / slack)
            if not near[e].any():
                assert got64 >= best64 - slack, (e, got64, best64, slack)
        # no worse than 32 random one-to-one placements scored by evaluate()
        cand = np.repeat(cur[:, None, :], 32, axis=1)
        for e in range(b):
            for q in range(32):
                cand[e, q, links] = _random_placement(rng, links, r, allowed)
                assert len(set(cand[e, q, links].tolist())) == len(links)
        scores = env.evaluate(torch.as_tensor(cand.astype(np.int32), device=env.device), pwr.expand(b, 32, n).contiguous(),
                              planes=())['total_mbps'].cpu().numpy().astype(np.float64)
        print(f'{name}, allowed {masked}: identity against evaluate() {e_id:.3e}; value {value.cpu().numpy().tolist()}; shortfall against '
              f'the float64 optimum / allowed slack {max(slack_used):.3e}; {near.mean():.2%} near a threshold; total {total.min():.3f} .. '
              f'{total.max():.3f} Mbps against the best of 32 random placements {scores.max(axis=1).min():.3f} .. {scores.max(axis=1).max():.3f}')
        assert e_id <= 1e-6
        assert (total >= scores.max(axis=1) * (1.0 - 1e-6)).all()
        # the weights and the matching alone give the same result; an infeasible env keeps its row
        w, lk = env.assignment_weights(allowed=allowed)
        assert np.array_equal(lk.cpu().numpy(), links) and tuple(w.shape) == (b, len(links), r)
        col, val, ok = env.solve_assignment(w)
        assert torch.equal(col, rb[:, links].to(torch.int32)) and torch.equal(val, value) and torch.equal(ok, feasible)
        shut = np.ones((n, r), bool) if allowed is None else allowed.copy()
        shut[links[0]] = False
        kept = env.assign_rbs(allowed=shut)
        assert kept.feasible.cpu().numpy().tolist() == [0] * b and torch.equal(kept.rb, before['rb']) and (kept.value_mbps == 0).all()
    finally:
        env.close()


def test_actions_put_the_step_on_the_matched_rbs_and_compose_with_power_control():
    env = _env('small')
    try:
        env.reset(seed=8)
        for _ in range(2):
            rb = env.assign_rbs().rb.clone()
            pwr = env._t['pwr'].clone()
            act = env.assign_rbs_actions()
            assert tuple(act.shape) == (5, env.num_agents) and act.dtype == torch.int32
            _, _, _, info = env.step(act)
            assert torch.equal(info['rb'], rb) and torch.equal(env._t['pwr'], pwr)
        # one call picks RBs, the other picks powers
        levels = env._action_levels
        mixed = (env.assign_rbs_actions() // levels) * levels + env.power_control_actions({'cue': -4.0, 'due': 9.0}) % levels
        rb = env.assign_rbs().rb.clone()
        _, _, _, info = env.step(mixed.to(torch.int32))
        assert torch.equal(info['rb'], rb)
        # a movable subset and out=
        movable = np.zeros(10, bool)
        movable[[1, 5, 9]] = True
        out = (torch.empty((5, 10), dtype=torch.int32, device=env.device), torch.empty(5, device=env.device),
               torch.empty(5, dtype=torch.uint8, device=env.device))
        got = env.assign_rbs(movable=movable, out=out)
        assert got.rb is out[0] and got.value_mbps is out[1] and got.feasible is out[2]
        fixed = ~movable
        assert torch.equal(out[0][:, fixed], env._t['rb'][:, fixed]) and out[2].cpu().numpy().tolist() == [1] * 5
        w, lk, harm = env.assignment_weights(movable=movable, harm=True)
        own = env.assignment_weights(movable=movable, objective='own', out=torch.empty_like(w))[0]
        assert lk.cpu().numpy().tolist() == [1, 5, 9] and tuple(harm.shape) == (5, 3, 8) and (harm >= 0).all()
        assert (own.double() - harm.double() - w.double()).abs().max() <= 1e-5 * max(float(own.max()), 1.0)
        for bad, text in ((dict(objective='sum'), 'objective must be'), (dict(movable=np.ones(9, bool)), 'movable must be'),
                          (dict(movable=np.zeros(10, bool)), 'movable marks no link'), (dict(allowed=np.ones((10, 7), bool)), 'allowed must be'),
                          (dict(out=torch.empty((5, 3, 8), device=env.device)), 'out must be')):
            with pytest.raises(ValueError, match=text):
                env.assignment_weights(**bad)
        with pytest.raises(ValueError, match='weights must be'):
            env.solve_assignment(w.double())
        with pytest.raises(ValueError, match=r'M = 9 must be <= R = 8'):
            env.solve_assignment(torch.zeros((2, 9, 8), device=env.device))
    finally:
        env.close()


def test_after_an_autoreset_step_the_result_is_a_direct_launch_on_the_current_planes():
    from gym_d2d_amd.mobility import GaussMarkovMobility
    env = _env('small', autoreset=True, mobility=GaussMarkovMobility(speed_std_mps=8.0, memory=0.7))
    try:
        b = env.num_envs
        rng = np.random.default_rng(6)
        env.reset(seed=21, elapsed=np.arange(b) % 10)
        resets = 0
        for _ in range(12):
            a = torch.as_tensor(np.stack([rng.integers(0, h, b) for h in env._initial_action_highs()], axis=1).astype(np.int32),
                                device=env.device)
            _, _, _, info = env.step(a)
            resets += int(info['reset'].sum())
            res = env.assign_rbs()
            w = env.assignment_weights()[0].cpu().numpy()
            k = env._assignment_kernel()
            c = dict(_env_case(env), fresh=True, cols=k.cols.cpu().numpy(), cap_cols=k.cap_cols.cpu().numpy(), kind=k.law, pow_k=k.pow_k, d=k.d)
            c['pos'] = c['pos'].astype(np.float32)
            c['tx'], c['rx'] = c['tx'].astype(np.int32), c['rx'].astype(np.int32)
            links = np.arange(env.num_cues, env.num_links, dtype=np.int32)
            direct, _ = _launch_weights(c, links, harm=False)
            assert np.array_equal(_bits(direct), _bits(w))
            col, value, feasible = _launch_solve(direct)
            assert np.array_equal(col, res.rb.cpu().numpy()[:, links]) and np.array_equal(_bits(value), _bits(res.value_mbps.cpu().numpy()))
        print(f'{resets} env resets inside 12 steps')
        assert resets >= b
    finally:
        env.close()


def test_what_cannot_be_served_is_refused_by_name(tmp_path):
    from gym_d2d_amd.envs import VecD2DEnv
    from gym_d2d_amd.path_loss import ArrayPathLoss, PathLoss, ShadowingPathLoss
    small = {'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}

    class Foo(PathLoss):
        def __call__(self, tx, rx):
            return 20 * np.log10(tx.position.distance(rx.position)) + 40.0

    class Arr(ArrayPathLoss):
        def compute(self, view):
            return 20 * view.xp.log10(view.distance()) + 40.0

    class PerStep(Arr):
        per_step = True

    def refused(text, cfg=None, **kw):
        env = VecD2DEnv(dict(small, **(cfg or {})), num_envs=2, **kw)
        try:
            env.reset(seed=1)
            for call in (env.assign_rbs, env.assign_rbs_actions, env.assignment_weights,
                         lambda: env.solve_assignment(torch.zeros((2, 3, 4), device=getattr(env, 'device', None)))):
                with pytest.raises(ValueError, match=text):
                    call()
        finally:
            env.close()
    refused(r'assign_rbs\(\).*export_actions', export_actions=False)
    refused(r'assign_rbs\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"assign_rbs\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"assign_rbs\(\).*'array'", {'path_loss_model': Arr})
    refused(r"assign_rbs\(\).*'per_step'", {'path_loss_model': PerStep})
    refused(r'assign_rbs\(\).*torch path', use_torch=False)
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'assign_rbs\(\).*float32 cannot hold', {'device_config_file': pinned})
    # more movable links than RBs names both numbers; a link on fixed actions cannot be moved
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 5}, num_envs=2)
    try:
        env.reset(seed=1)
        with pytest.raises(ValueError, match=r'5 movable links .* 4 RBs: M = 5 must be <= R = 4'):
            env.assign_rbs()
        with pytest.raises(ValueError, match=r'M = 5 must be <= R = 4'):
            env.assign_rbs_actions()
        w, links = env.assignment_weights()                              # the weights alone are served
        assert tuple(w.shape) == (2, 5, 4) and links.cpu().numpy().tolist() == [3, 4, 5, 6, 7]
    finally:
        env.close()
    env = VecD2DEnv({'num_rbs': 4, 'num_cues': 3, 'num_due_pairs': 3}, num_envs=2, cue_actions='traffic')
    try:
        env.reset(seed=1)
        movable = np.zeros(6, bool)
        movable[[1, 4]] = True
        with pytest.raises(ValueError, match='movable marks link 1, which has no action column'):
            env.assign_rbs(movable=movable)
        assert env.assign_rbs().feasible.cpu().numpy().tolist() == [1, 1]
    finally:
        env.close()


def test_the_example_runs_and_the_matching_beats_the_random_placements():
    import runpy
    from pathlib import Path
    res = runpy.run_path(str(Path(__file__).resolve().parent.parent / 'examples' / 'rb_matching.py'), run_name='__main__')['results']
    print(res)
    best_random = res['the best of 32 random one-to-one placements']
    assert res["assign_rbs(objective='total')"] >= best_random >= res['random actions']
    assert res["assign_rbs(objective='total')"] >= res["assign_rbs(objective='own')"] * (1.0 - 1e-6)
    assert abs(res['the step that takes assign_rbs_actions()'] / res["assign_rbs(objective='total')"] - 1.0) <= 1e-6

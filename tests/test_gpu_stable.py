"""Stable RB matching on the GPU (csrc/d2d_stable.hip; VecD2DEnv.solve_stable_matching, stable_rbs, stable_rbs_actions).

One yardstick, no tolerance: the sequential NumPy restatement (stable_util) fed the same tensors.  The link-proposing result and its
count of proposals do not depend on the order of the proposals, so the kernel's parallel rounds must give the restatement's words:
all four outputs are compared for equality.  Every direct launch writes into guarded allocations whose guard words are checked, and
is made twice.

The common content of the random cases (stable_util.case): entries that are not finite in both tensors, a wholly unacceptable row,
and - where the case has more than one env - a wholly unacceptable env among live ones; a case of ONE env launches such an env on
its own at the same shape instead.

On an MI355X the 14 tests take 3.3 s in all, the restatement of 2048 x 256 (119 864 proposals) most of it; every case was equal."""
import numpy as np
import pytest

import stable_util as su

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

NAMES = ('col', 'load', 'proposals', 'unmatched')
GUARD = 64                                          # guard words on either side of an output
SENTINEL = -1234567


def _guarded(shape):
    """(the whole allocation, the output inside it): GUARD sentinel words before and behind."""
    total = int(np.prod(shape))
    whole = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda')
    return whole, whole[GUARD:GUARD + total].view(shape)


def _launch(lp, rp, quota):
    """d2d_stable_match on the uploaded tensors; the four outputs on the host, the guards checked."""
    from gym_d2d_amd import _native
    b, m, r = lp.shape
    lp_d, rp_d, q_d = (torch.as_tensor(np.ascontiguousarray(x), device='cuda') for x in (lp, rp, quota))
    bufs = [_guarded(s) for s in ((b, m), (b, r), (b,), (b,))]
    before = _native.stable_launches
    _native.stable_match(lp_d.data_ptr(), rp_d.data_ptr(), q_d.data_ptr(), b, m, r, *(o.data_ptr() for _, o in bufs),
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    assert _native.stable_launches == before + 1
    for (whole, _), name in zip(bufs, NAMES):
        assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), f'guard words of {name}'
    return tuple(o.cpu().numpy().copy() for _, o in bufs)


_REFS = {}


def _ref(name):
    """The restatement's four outputs of a case, computed once."""
    if name not in _REFS:
        _REFS[name] = su.solve_batch(*su.case(name))
    return _REFS[name]


def _same(got, want, what):
    for x, y, name in zip(got, want, NAMES):
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), f'{what}: {name}'


@pytest.mark.parametrize('name', list(su.CASES))
def test_direct_launch_equals_the_restatement(name):
    from gym_d2d_amd import stable_matching
    b, m, r, _, what = su.CASES[name]
    lp, rp, quota = su.case(name)
    want = _ref(name)
    got = _launch(lp, rp, quota)
    print(f'{name}: {b} x {m} x {r}, quota {sorted(set(quota.tolist()))}; proposals {want[2].tolist()}, unmatched {want[3].tolist()}; '
          f'LDS {stable_matching.lds_bytes(m, r)} bytes')
    _same(got, want, name)
    _same(_launch(lp, rp, quota), got, name + ', the second call')
    assert (got[1] <= quota[None, :]).all() and np.array_equal(got[3], (got[0] < 0).sum(axis=1))
    if what == 'random':
        assert (got[0][0, m // 2] == -1)                                # the wholly unacceptable row
        if b >= 2:
            assert (got[0][b - 1] == -1).all() and got[2][b - 1] == 0 and got[3][b - 1] == m and (got[1][b - 1] == 0).all()
            assert got[2][:b - 1].sum() > 0                             # beside live ones
        else:
            rng = np.random.default_rng(1)
            dead = tuple(x[None] for x in su.dead_env(rng, m, r))
            alone = _launch(*dead, quota)
            assert (alone[0] == -1).all() and (alone[1] == 0).all() and alone[2].tolist() == [0] and alone[3].tolist() == [m]
    if name == 'row_limit':
        assert stable_matching.lds_bytes(m, r) > 64 * 1024              # the dynamic-LDS attribute was needed
    if name == 'rejection_chain':
        assert got[2].tolist() == [8256, 8256] and got[0].tolist() == [list(range(128))] * 2
    if name == 'pure_index_order':
        assert got[0].tolist() == [[a // 2 for a in range(50)]] * 2 and got[3].tolist() == [0, 0]
    if name == 'closed_rb':
        assert (got[1][:, 2] == 0).all() and (got[0] != 2).all() and got[3][0] >= 2


def test_no_blocking_pair_by_brute_force_on_the_kernels_own_words():
    for name in ('closed_rb', 'wave_edge_odd', 'many_per_rb'):
        lp, rp, quota = su.case(name)
        got = _launch(lp, rp, quota)
        for e in range(lp.shape[0]):
            assert su.feasible(lp[e], rp[e], quota, got[0][e]) and su.blocking_pairs(lp[e], rp[e], quota, got[0][e]) == [], (name, e)


# ------------------------------------------------------------------------------------------------ through the env
def _env(cues, dues, rbs, b=4, seed=3):
    from gym_d2d_amd.envs import VecD2DEnv
    env = VecD2DEnv({'num_rbs': rbs, 'num_cues': cues, 'num_due_pairs': dues}, num_envs=b)
    rng = np.random.default_rng(seed)
    env.reset(seed=seed)
    env.step(torch.as_tensor(np.stack([rng.integers(0, h, b) for h in env._initial_action_highs()], axis=1).astype(np.int32),
                             device=env.device))
    return env


def _prefs(env, rb_pref):
    """The downloaded assignment_weights(objective='own', harm=True) planes as (link_pref, rb_pref), float32 on the host."""
    own, links, harm = env.assignment_weights(objective='own', harm=True)
    own, harm = own.cpu().numpy().copy(), harm.cpu().numpy().copy()
    return own, (-harm if rb_pref == 'harm' else own - harm), harm, links.cpu().numpy().copy()


@pytest.mark.parametrize('rb_pref', ['harm', 'total'])
def test_stable_rbs_on_16_and_16_links_and_32_rbs(rb_pref):
    from gym_d2d_amd import _native
    env = _env(16, 16, 32)
    try:
        b, n, r = env.num_envs, env.num_links, env.config.num_rbs
        cur = env._t['rb'].clone()
        launches = _native.assign_weights_launches, _native.stable_launches
        res = env.stable_rbs(rb_pref=rb_pref)
        assert (_native.assign_weights_launches, _native.stable_launches) == (launches[0] + 1, launches[1] + 1)
        assert res._fields == ('rb', 'unmatched', 'proposals') and all(x.dtype == torch.int32 for x in res)
        rb, unmatched, proposals = (x.clone() for x in res)
        assert torch.equal(env._t['rb'], cur) and env.status_flags() == 0                      # the env is untouched
        lp, rp, harm, links = _prefs(env, rb_pref)
        assert links.tolist() == list(range(16, 32)) and lp.shape == (b, 16, r)
        want = su.solve_batch(lp, rp, 1)
        rb_h = rb.cpu().numpy()
        assert np.array_equal(rb_h[:, links], want[0]) and np.array_equal(proposals.cpu().numpy(), want[2])
        assert unmatched.cpu().numpy().tolist() == want[3].tolist() == [0] * b
        assert np.array_equal(rb_h[:, :16], cur.cpu().numpy()[:, :16])                          # background rows are unchanged
        assert all(len(set(row)) == 16 for row in rb_h[:, links].tolist())                      # matched RBs are distinct
        for e in range(b):
            assert su.blocking_pairs(lp[e], rp[e], 1, rb_h[e, links]) == []
        # quota 1: the preferences are the true capacities - evaluate(rb) = evaluate(background) + the matched 'total' weights
        pwr = env._t['pwr'].unsqueeze(1).contiguous()
        total = env.evaluate(rb.unsqueeze(1).contiguous(), pwr, planes=())['total_mbps'][:, 0].cpu().numpy().astype(np.float64)
        off = cur.clone()
        off[:, 16:] = -1
        cap = env.evaluate(off.unsqueeze(1).contiguous(), pwr, planes=('capacity_mbps',))['capacity_mbps'][:, 0].cpu().numpy()
        background = cap[:, :16].astype(np.float64).sum(axis=1)
        rows = np.arange(16)
        matched = np.array([(lp[e].astype(np.float64) - harm[e].astype(np.float64))[rows, rb_h[e, links]].sum() for e in range(b)])
        err = float(np.abs(background + matched - total).max() / max(float(np.abs(total).max()), 1.0))
        print(f'rb_pref {rb_pref}: proposals {want[2].tolist()}; total {total.tolist()} Mbps; identity against evaluate() {err:.3e}')
        assert (np.abs(background + matched - total) <= 1e-5 * np.maximum(np.abs(total), 1.0)).all()
        # the matching alone on the same planes, with out=; and the actions
        own_t, _, harm_t = env.assignment_weights(objective='own', harm=True)
        pref_t = torch.neg(harm_t) if rb_pref == 'harm' else own_t - harm_t
        out = (torch.empty((b, 16), dtype=torch.int32, device=env.device), torch.empty((b, r), dtype=torch.int32, device=env.device),
               torch.empty(b, dtype=torch.int32, device=env.device), torch.empty(b, dtype=torch.int32, device=env.device))
        solved = env.solve_stable_matching(own_t, pref_t, out=out)
        assert solved._fields == ('col', 'load', 'proposals', 'unmatched') and all(x is y for x, y in zip(solved, out))
        assert np.array_equal(out[0].cpu().numpy(), want[0]) and np.array_equal(out[1].cpu().numpy(), want[1])
        act = env.stable_rbs_actions(rb_pref=rb_pref)
        keep = env._t['pwr'].clone()
        _, _, _, info = env.step(act)
        assert torch.equal(info['rb'], rb) and torch.equal(env._t['pwr'], keep)
    finally:
        env.close()


def test_quotas_on_6_and_24_links_and_8_rbs_and_allowed():
    env = _env(6, 24, 8, seed=5)
    try:
        b, n, r = env.num_envs, env.num_links, env.config.num_rbs
        cur = env._t['rb'].cpu().numpy().copy()
        lp, rp, _, links = _prefs(env, 'harm')
        assert links.tolist() == list(range(6, 30)) and np.isfinite(lp).all() and np.isfinite(rp).all()
        for quota, left in ((3, 0), (2, 8), ([3, 3, 3, 3, 3, 3, 3, 0], 3)):
            rb, unmatched, proposals = (x.cpu().numpy().copy() for x in env.stable_rbs(quota=quota))
            want = su.solve_batch(lp, rp, quota)
            assert unmatched.tolist() == want[3].tolist() == [left] * b and np.array_equal(proposals, want[2])
            assert np.array_equal(rb[:, links], np.where(want[0] >= 0, want[0], cur[:, links]))     # an unmatched link keeps its RB
            assert np.array_equal(rb[:, :6], cur[:, :6])
            print(f'quota {quota}: {left} of 24 unmatched per env, proposals {proposals.tolist()}')
        # allowed arrives as -inf: forbidden pairs are unacceptable
        allowed = np.ones((n, r), bool)
        allowed[links[::2], :4] = False
        allowed[links[1]] = False                                        # a movable link with nothing allowed stays where it is
        rb, unmatched, proposals = (x.cpu().numpy().copy() for x in env.stable_rbs(allowed=allowed, quota=3))
        own = env.assignment_weights(allowed=allowed, objective='own', harm=True)[0].cpu().numpy()
        assert np.isneginf(own[:, ::2, :4]).all() and np.isneginf(own[:, 1]).all()
        want = su.solve_batch(np.where(allowed[links][None], lp, -np.inf).astype(np.float32), rp, 3)
        assert np.array_equal(rb[:, links], np.where(want[0] >= 0, want[0], cur[:, links])) and np.array_equal(proposals, want[2])
        assert (want[0][:, 1] == -1).all() and ((want[0][:, ::2] >= 4) | (want[0][:, ::2] == -1)).all() and (unmatched >= 1).all()
        # quota as a device tensor, twice: the same words
        q = torch.tensor([1, 2, 3, 0, 1, 2, 3, 0], dtype=torch.int32, device=env.device)
        first = tuple(x.clone() for x in env.stable_rbs(quota=q))
        again = env.stable_rbs(quota=q)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        assert np.array_equal(first[0].cpu().numpy()[:, links], np.where((w := su.solve_batch(lp, rp, q.cpu().numpy()))[0] >= 0, w[0], cur[:, links]))
        with pytest.raises(ValueError, match=r'quota must be an int or \[8\] ints \(RB\), each in \[0, 24\]'):
            env.stable_rbs(quota=25)
        with pytest.raises(ValueError, match="rb_pref must be 'harm' or 'total'"):
            env.stable_rbs(rb_pref='own')
    finally:
        env.close()

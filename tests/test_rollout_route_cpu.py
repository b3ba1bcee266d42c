"""What test_gpu_rollout_route.py stands on, without a GPU (tests/rollout_route_util.py): every row of the case table plans to the
rollout_kernel instantiation it names, in the launch shape it states; the rows together name exactly the 48 rollout kernels of the
gfx950 code object of d2d_rollout.hip, so a new instantiation without a row fails here; and, on the float64 reference alone, every
case holds a link in every arm of the kernel - clear of the arm's boundary by a factor of 4 -, no link within 1e-4 dB of a
threshold that decides an output, and both outcomes of its reward."""
import re

import numpy as np
import pytest

import rollout_route_util as rr
from oracle import d2d_oracle as orc
from step_plan_util import build_step_plan, kernel_names, mangled

LDS_HEAD_BYTES = 80


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    return build_step_plan(tmp_path_factory.mktemp('plan'))


def test_every_row_plans_to_the_kernel_it_names(plan):
    for mode in rr.MODELS:
        got = plan([r.plan_inputs(mode) for r in rr.ROWS])
        assert len(got) == len(rr.ROWS)
        for r, p in zip(rr.ROWS, got):
            assert p.get('kernel') == r.kernel(mode), (r.name, mode, p)
            assert (p['rollout'], p['lpt'], p['tpe'], p['epw'], p['grid'], p['block'], p['mask_words'], p['walk']) == \
                (1, r.lpt, r.threads(), 1, rr.B, r.threads(), 0, 2), (r.name, mode, p)
            assert (p['rec_uniform'], p['nt_results']) == (int(r.opt & 2 != 0), int(r.opt & 4 != 0)), (r.name, mode, p)
            assert p['obs_expand'] == int(r.obs == 'linear') and p['fuse_obs'] == 0, (r.name, mode, p)
            assert p['lds'] == p['env_bytes'] <= 64 * 1024
            # rollout_lds_layout: 16 (N + 1) + 8 N bytes of tuples and pool before anything else, so the env's LDS always holds its
            # table image and the direct 48-byte store arm of the two-links-per-thread table rows is never taken
            assert p['env_bytes'] - LDS_HEAD_BYTES >= 24 * r.n, (r.name, mode, p)


def test_pass_0_takes_further_rounds_only_in_the_rows_with_300_rbs():
    for r in rr.ROWS:
        assert (rr.pass0_rounds(r) > 2) == (r.rbs == 300), r.name
    assert (rr.pass0_rounds(rr.BY_NAME['r300_l2']), rr.pass0_rounds(rr.BY_NAME['r300_l1'])) == (6, 3)


def test_the_rows_cover_every_rollout_kernel_of_the_code_object(tmp_path):
    built = {k for k in kernel_names(tmp_path, 'd2d_rollout.hip') if re.match(r'_ZN3d2d14rollout_kernelI', k)}
    planned = {mangled(r.kernel(mode)) for r in rr.ROWS for mode in rr.MODELS}
    assert built == planned, (sorted(built - planned), sorted(planned - built))
    assert len(built) == 48
    assert len({(r.opt, r.lpt) for r in rr.ROWS}) == 16 and len(rr.ROWS) == 18          # the two rows with 300 RBs repeat names


def test_the_settings_are_spread_over_both_link_counts_per_thread():
    def rows(**kw):
        return {r.lpt for r in rr.ROWS if all(getattr(r, k) == v for k, v in kw.items())}
    assert rows(reward=1, per_env=False) == rows(reward=1, per_env=True) == rows(reward=2) == {1, 2}
    assert rows(obs='table') == rows(obs='none') == rows(obs='linear') == rows(export=True) == rows(export=False) == {1, 2}
    for picked in (rows(reward=3), rows(fixed=True)):
        assert picked == {1}                                        # the planner gives both one link per thread
    for what in ('reward', 'fixed'):                                # ... on a plain, a padded and an exact-position row each
        opts = {r.opt & 24 for r in rr.ROWS if (r.reward == 3 if what == 'reward' else r.fixed)}
        assert opts >= {0, 8, 16}, (what, opts)
    assert all(not (r.opt & 2) for r in rr.ROWS if r.fixed)         # no scalar records beside a fixed prefix


@pytest.mark.parametrize('name,model', rr.CASES)
def test_every_case_holds_a_link_in_every_arm(name, model):
    inp = rr.inputs(name, model)
    row, c = inp.row, inp.row.cues
    arm, clear, divided = rr.classify(inp)
    counts = rr.arm_counts(inp)
    print(name, model, 'attempt', inp.attempt, counts)
    for a in rr.ARMS:
        assert counts[a] >= 1, (a, counts)
    victim = c + rr.VICTIM_DUE
    for env, want in ((0, 're_sorted'), (1, 'pool_selection'), (2, 'pool_sweep')):
        assert arm[env, victim] == want and clear[env, victim], (env, arm[env, victim])
    members = np.bincount(inp.ref['rb'][1][inp.ref['rb'][1] >= 0], minlength=row.rbs)
    assert (members[row.rbs - 1], np.bincount(inp.ref['rb'][2], minlength=row.rbs)[44]) == (12, 40)
    # env 3: rb == R twice and rb == -1, all by division; no action beyond the multiply-high bound decodes inside [0, R) - the bound
    # is R P - 1 at every shape of the table -, so inside the range only a fixed link is decoded by division
    rb = inp.ref['rb']
    assert (rb[3, rr.OOR_CUE], rb[3, c + rr.OOR_DUE], rb[3, rr.NEG_CUE]) == (row.rbs, row.rbs, -1)
    out = (rb < 0) | (rb >= row.rbs)
    assert out.sum() == 3 and out[3].sum() == 3 and (arm[out] == 'oor_sweep').all() and divided[out].all()
    assert np.array_equal(rr.decode_bound(row, inp.levels), row.rbs * inp.levels - 1)
    assert np.array_equal(divided & ~out, np.broadcast_to(np.arange(row.n) < (rr.N_FIXED if row.fixed else 0), out.shape))
    # env 4: the nine on the ring - the pool, order-free, every term well inside the window
    nine = [c + p for p in rr.ENV4_DUES]
    assert (arm[4, nine] == 'pool_order_free').all() and clear[4, nine].all()
    assert np.bincount(rb[4], minlength=row.rbs)[row.rbs - 2] == 9
    assert (np.bincount(rb[4], minlength=row.rbs) > rr.SLOTS).sum() >= 2          # two RBs' entries in one pool
    # env 6: the row's edge links sit on an RB with a pool
    crowded = np.bincount(rb[6], minlength=row.rbs)[rb[6]] > rr.SLOTS
    if row.n % 64:
        assert crowded[[row.n - 1, row.n - 2]].all() and rb[6, row.n - 1] == rb[6, row.n - 2]
    elif row.lpt == 2:
        pair = [c + rr.ENV6_DUES[0], c + rr.ENV6_DUES[1]]
        assert pair[0] % 2 == 0 and crowded[pair].all() and rb[6, pair[0]] == rb[6, pair[1]]
    if row.lpt == 2:                 # (env 3) a thread with one link out of range and the other ordinary, twice
        assert rr.OOR_CUE % 2 == 1 and not out[3, rr.OOR_CUE - 1] and (c + rr.OOR_DUE) % 2 == 0 and not out[3, c + rr.OOR_DUE + 1]
    if row.fixed:
        assert crowded[rr.ENV6_FIXED_LINK] and divided[6, rr.ENV6_FIXED_LINK]
        assert inp.fixed is not None and np.array_equal(rb[:, :rr.N_FIXED], np.broadcast_to(inp.fixed[1], (rr.B, rr.N_FIXED)))
    # env 7: untouched.  Under 1 / d^2 every link is exact and clear.  Under the steeper laws random links leave the window by
    # themselves (3 % at an exponent of 3, half of them under COST-Hata at four links per RB: further witnesses of the sorted
    # sum), so there the env only has to hold the common arm in a quarter of its links
    exact7 = np.isin(arm[7], ('common', 'pool_order_free')) & clear[7]
    if model == 'inv2':
        assert exact7.all()
    else:
        assert exact7.mean() >= 0.25 and not out[7].any()
    assert not divided[7, (rr.N_FIXED if row.fixed else 0):].any()


@pytest.mark.parametrize('name,model', rr.CASES)
def test_no_link_lies_at_a_threshold_and_both_reward_outcomes_occur(name, model):
    inp = rr.inputs(name, model)
    row, ref, ty = inp.row, inp.ref, inp.ty
    side = ty == orc.SIDELINK
    for step_ref, param in [(ref, inp.param)] + [(s.ref, s.param) for s in inp.roles]:
        sinr = step_ref['sinr_db']
        assert np.isfinite(sinr).all() and np.isfinite(step_ref['snr_db']).all()
        assert (np.abs(sinr - step_ref['sens'][None]) > rr.THRESHOLD_DB).all()
        if row.reward == 1:
            assert (np.abs(sinr - rr.capacity_threshold_db(row, model, param)[None]) > rr.THRESHOLD_DB)[:, ~side].all()
        else:
            assert (np.abs(sinr - param) > rr.THRESHOLD_DB).all()
        assert rr.near(row, model, step_ref, param) == 0
    c = row.cues
    if row.reward == 1:
        assert ref['reward'].shape == (rr.B,)
        minus = ref['reward'] == -1.0
        assert minus.sum() >= 2 and (~minus).sum() >= 2 and (ref['reward'][~minus] > 0).all(), ref['reward']
        # envs 5 and 6: eleven CUE links and exactly one sidelink on RB 51, the weak one's capacity positive and below MIN_CAPACITY;
        # envs 5 and 4: the same on RB 53 without a sidelink, and env 4 stays at the mean
        rb, cap = ref['rb'], ref['capacity_mbps']
        for env in (5, 6):
            on = rb[env] == 51
            assert (on & ~side).sum() == 11 and (on & side).sum() == 1 and on[c + rr.CROWD_A_DUE[env]] and minus[env]
            assert 0.0 < cap[env, rr.CROWD_A[0]] <= inp.param == rr.MIN_CAPACITY
        for env in (5, 4):
            on = rb[env] == 53
            assert (on & ~side).sum() == 11 and (on & side).sum() == 0 and 0.0 < cap[env, rr.CROWD_B[0]] <= inp.param
        assert not minus[4]
    else:
        minus = ref['reward'] == -1.0
        assert 0.1 <= minus.mean() <= 0.9, minus.mean()
    if row.reward == 3:
        # twelve role steps: the twelve of env 5's RB 51, each in turn the one non-D2D link below the threshold - the other eleven
        # get -1 through whichever of row and pool holds it, the low one its own value
        assert len(inp.roles) == 12 and (ref['rb'][5] == 51).sum() == 12
        twelve = list(rr.ROLE_CUES)
        for k, s in enumerate(inp.roles):
            changed = s.raw != inp.raw
            assert changed.sum() == 1 and changed[5, twelve[k]] and s.ref['pwr'][5, twelve[k]] == 0
            low = (s.ref['sinr_db'][5, twelve] < s.param)
            assert low.sum() == 1 and low[k]
            r5 = s.ref['reward'][5, twelve]
            assert (np.delete(r5, k) == -1.0).all() and r5[k] > 0.0


@pytest.mark.parametrize('name,model', [(n, m) for n, m in rr.CASES if n in ('o6_l2', 'o12_l1', 'o20_l1')])
def test_the_zero_distance_batch_and_the_exact_positions(name, model):
    inp = rr.inputs(name, model)
    row, c = inp.row, inp.row.cues
    pos, raw = inp.zero_pos, inp.zero_raw
    tx, rx = inp.tx, inp.rx
    d = np.hypot(*(pos[:, tx][:, :, None, :] - pos[:, rx][:, None, :, :]).transpose(3, 0, 1, 2))          # [B, j, i]
    rb, _ = orc.decode_actions(raw, inp.levels[None, :])
    same = rb[:, :, None] == rb[:, None, :]
    zero = np.argwhere((d == 0.0) & same)
    assert sorted(map(tuple, zero)) == [(0, c + 7, c + 7), (1, c + 7, c + 7), (2, c + 11, c + 3)], zero
    assert [(e, c + p) for e, p in rr.ZERO_LINKS] == [(0, c + 7), (1, c + 7), (2, c + 3)]
    assert [(rb[e] == rb[e, c + p]).sum() for e, p in rr.ZERO_LINKS] == [1, 3, 2]
    assert ((rb >= 0) & (rb < row.rbs)).all()
    for p in (inp.pos, pos):
        if row.xpos:
            assert p.dtype == np.float64 and (p[:, 1:] != p[:, 1:].astype(np.float32)).all() and (p[:, 0] == 0).all()
        else:
            assert p.dtype == np.float32

"""What-if evaluation of candidate joint actions on the GPU (VecD2DEnv.evaluate / evaluate_actions, csrc/d2d_evaluate.hip).

Direct launches against evaluate_util.evaluate_ref, the float64 reference test_evaluate_cpu.py ties to the oracle's step at 1e-9; the
bar is the project's 1e-5 (|d| <= 1e-5 max(|ref|, 1)) on sinr_db (dB) and capacity_mbps (Mbps).  Links whose reference sinr_db lies
within 1e-4 dB of their receiver's sensitivity are left out of the capacity comparison, at most 1 % of a case (asserted on the
reference alone in test_evaluate_cpu.py: none in any case here).  Then candidate independence, null planes and the env's own step,
all bit for bit.  Every test prints what it measured.

Measured on an MI355X: sinr_db rel_err 8.9e-8 - 2.2e-6, capacity_mbps 1.8e-8 - 2.5e-7, total_mbps within 5.4e-8 of the float64 sum of
its plane over the eight cases and the two contrast runs (CHANGELOG.md)."""
import json

import numpy as np
import pytest

import evaluate_util as evu
from rb_sensing_util import _models

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
GUARD, PAD = 0x5AFEC0DE, 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_inputs = {}


def _device_inputs(c):
    """The candidate-independent device tensors of a case, uploaded once per case."""
    key = id(c['pos'])
    if key not in _inputs:
        dev = torch.device('cuda', 0)
        _inputs[key] = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in
                        (c['pos'][..., 0].astype(np.float32), c['pos'][..., 1].astype(np.float32), c['tx'], c['rx'], c['cols'], c['cap_cols'])]
    return _inputs[key]


def _launch(c, rb, pwr, sinr=True, cap=True, shift=0):
    """One d2d_evaluate launch with every output inside guard words; shift: words (4 bytes each) by which every output pointer is
    moved off its 256-byte alignment.  Returns (sinr_db, capacity_mbps, total_mbps) as host arrays, None for a plane not asked for."""
    from gym_d2d_amd import _native
    dev = torch.device('cuda', 0)
    px, py, tx, rx, cols, cap_cols = _device_inputs(c)
    b, k, n = rb.shape
    rb_t, pwr_t = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev) for a in (rb, pwr))
    words, tw = b * k * n, b * k
    o_s, o_c, o_t = PAD + shift, 2 * PAD + words + shift, 3 * PAD + 2 * words + shift
    arena = torch.full((2 * words + tw + 4 * PAD + shift,), GUARD, dtype=torch.int32, device=dev)
    base = arena.data_ptr()
    _native.evaluate(px.data_ptr(), py.data_ptr(), rb_t.data_ptr(), pwr_t.data_ptr(), tx.data_ptr(), rx.data_ptr(), cols.data_ptr(),
                     cap_cols.data_ptr(), c['kind'], c['pow_k'], b, k, c['d'], n, c['r'], base + 4 * o_s if sinr else 0,
                     base + 4 * o_c if cap else 0, base + 4 * o_t, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()                                            # raises if the device faulted
    host = arena.cpu().numpy()
    live = np.zeros(host.shape, bool)
    for on, o, w in ((sinr, o_s, words), (cap, o_c, words), (True, o_t, tw)):
        if on:
            live[o:o + w] = True
    assert (host[~live] == GUARD).all()                                 # the guard words, and a plane that was not asked for, untouched
    f = host.view(np.float32)
    return (f[o_s:o_s + words].reshape(b, k, n).copy() if sinr else None, f[o_c:o_c + words].reshape(b, k, n).copy() if cap else None,
            f[o_t:o_t + tw].reshape(b, k).copy())


@pytest.mark.parametrize('n,r,law,k', evu.CASES)
def test_direct_launch_against_the_float64_reference(n, r, law, k):
    c = evu.make_case(n, r, law, k)
    ref_sinr, ref_cap, ref_total, decided = evu.case_ref(n, r, law, k)
    sinr, cap, total = _launch(c, c['rb'], c['pwr'])
    assert np.isfinite(sinr).all() and np.isfinite(cap).all() and np.isfinite(total).all()
    e_s, e_c = evu.rel_err(sinr, ref_sinr), evu.rel_err(cap[decided], ref_cap[decided])
    e_t = float(np.abs(total.astype(np.float64) / cap.astype(np.float64).sum(axis=2) - 1.0).max())
    left_out = float((~decided).mean())
    print(f'{n} links, {r} RBs, {law}, K = {k}: sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e}, total against the float64 sum '
          f'of its plane {e_t:.3e}; {left_out:.2%} left out at the threshold; LDS {evu.lds_bytes(n, r, law != "ld2")} B')
    assert left_out <= evu.THRESHOLD_CAP
    assert e_s <= evu.BAR
    assert e_c <= evu.BAR
    assert e_t <= 1e-6
    assert (ref_cap > 0).any()


def test_output_pointers_offset_by_four_bytes():
    n, r, law, k = 65, 5, 'ld2', evu.CHUNK + 1
    c = evu.make_case(n, r, law, k)
    ref_sinr, ref_cap, _, decided = evu.case_ref(n, r, law, k)
    aligned = _launch(c, c['rb'], c['pwr'])
    moved = _launch(c, c['rb'], c['pwr'], shift=1)
    for a, m in zip(aligned, moved):
        assert np.array_equal(_bits(a), _bits(m))
    assert evu.rel_err(moved[0], ref_sinr) <= evu.BAR and evu.rel_err(moved[1][decided], ref_cap[decided]) <= evu.BAR


@pytest.mark.parametrize('n,r,law', [(257, 7, 'ld35'), (63, 5, 'mixed')])
def test_candidates_do_not_depend_on_their_neighbours(n, r, law):
    """33 candidates that alternate between everyone on one RB and everyone spread out: each equals, bit for bit, a K = 1 launch of
    that candidate alone - nothing of candidate k's sort, start[] or sums reaches candidate k + 1 - and a second launch of all
    gives identical bits."""
    c = evu.make_case(n, r, law, 33)
    rb, pwr = evu.contrast_planes(c, 33)
    first = _launch(c, rb, pwr)
    again = _launch(c, rb, pwr)
    for a, m in zip(first, again):
        assert np.array_equal(_bits(a), _bits(m))
    ref_sinr, ref_cap, _ = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rb, pwr, c, r)
    e_s, e_c = evu.rel_err(first[0], ref_sinr), evu.rel_err(first[1], ref_cap)
    print(f'{n} links, {r} RBs, {law}: 33 contrasting candidates, sinr_db rel_err {e_s:.3e}, capacity rel_err {e_c:.3e}')
    decided = np.abs(ref_sinr - c['ocols'].sens_dbm[np.asarray(c['rx'])][None, None, :]) > evu.THRESHOLD_DB
    assert e_s <= evu.BAR and decided.mean() >= 1.0 - evu.THRESHOLD_CAP
    assert evu.rel_err(first[1][decided], ref_cap[decided]) <= evu.BAR
    for q in range(33):
        alone = _launch(c, rb[:, q:q + 1], pwr[:, q:q + 1])
        for a, m in zip(first, alone):
            assert np.array_equal(_bits(a[:, q:q + 1]), _bits(m)), q
    assert len({_bits(first[2][:, q]).tobytes() for q in range(33)}) > 2          # the candidates do differ


def test_null_planes_leave_the_other_outputs_and_the_guards_alone():
    n, r, law, k = 65, 5, 'ld2', evu.CHUNK + 1
    c = evu.make_case(n, r, law, k)
    sinr, cap, total = _launch(c, c['rb'], c['pwr'])
    for want_s, want_c in ((True, False), (False, True), (False, False)):
        s, p, t = _launch(c, c['rb'], c['pwr'], sinr=want_s, cap=want_c)      # _launch checks the guards and the absent planes' words
        assert (s is None) == (not want_s) and (p is None) == (not want_c)
        assert np.array_equal(_bits(t), _bits(total))
        assert s is None or np.array_equal(_bits(s), _bits(sinr))
        assert p is None or np.array_equal(_bits(p), _bits(cap))


def test_rb_outside_the_range_is_on_no_rb_and_writes_nothing_out_of_bounds():
    """Outside the contract, documented: such a link shares with nobody, as a link that has a real RB of its own."""
    n, r, law, k = 63, 5, 'mixed', evu.CHUNK
    c = evu.make_case(n, r, law, k)
    rng = np.random.default_rng(4)
    rb = c['rb'].copy()
    bad = rng.random(rb.shape) < 0.2
    rb[bad] = rng.choice([-1, -7, r, r + 1, 2 ** 31 - 1, -2 ** 31], int(bad.sum()))
    got = _launch(c, rb, c['pwr'])
    own = rb.copy()
    own[bad] = np.broadcast_to(r + np.arange(n, dtype=np.int32), rb.shape)[bad]
    want = _launch(dict(c, r=r + n), own, c['pwr'])
    for a, m in zip(got, want):
        assert np.array_equal(_bits(a), _bits(m))
    ref_sinr, _, _ = evu.evaluate_ref(c['pos'], c['tx'], c['rx'], rb, c['pwr'], c, r)
    assert evu.rel_err(got[0], ref_sinr) <= evu.BAR


# ------------------------------------------------------------------------------------------------ through the env
def _env(cue_actions, model, **kw):
    from gym_d2d_amd.envs import VecD2DEnv
    cfg = {'num_rbs': 7, 'num_cues': 5, 'num_due_pairs': 20}
    if model != 'default':
        cfg['path_loss_model'] = _models()[model][0]
    return VecD2DEnv(cfg, num_envs=4, cue_actions=cue_actions, **kw)


def _snapshot(env):
    t = env._t
    names = [k for k in ('rb', 'pwr', 'pos_x', 'pos_y', 'reward', 'sinr_db', 'capacity_mbps', 'elapsed', 'env_flags') if t.get(k) is not None]
    torch.cuda.synchronize()
    return {k: t[k].clone() for k in names}, env.num_steps


@pytest.mark.parametrize('cue_actions', ['agent', 'traffic'])
@pytest.mark.parametrize('model', ['default', 'ld35'])
def test_candidates_are_the_planes_of_the_step_that_takes_them(cue_actions, model):
    from gym_d2d_amd import _native
    env = _env(cue_actions, model)
    try:
        b, n, r, k = 4, 25, 7, 6
        rng = np.random.default_rng(31 + len(model))
        env.reset(seed=6)
        p = env.num_pwr_actions
        highs = ([r * p[env._cue_kind]] * 5 if cue_actions == 'agent' else []) + [r * p['due']] * 20
        assert env.num_agents == len(highs)
        actions = torch.as_tensor(rng.integers(0, highs, (b, k, len(highs))).astype(np.int32), device=env.device)
        before, steps = _snapshot(env)
        launches = _native.evaluate_launches
        res = env.evaluate_actions(actions)                              # first: right after reset()
        assert _native.evaluate_launches == launches + 1
        assert set(res) == {'total_mbps', 'sinr_db', 'capacity_mbps'}
        assert tuple(res['total_mbps'].shape) == (b, k) and tuple(res['sinr_db'].shape) == tuple(res['capacity_mbps'].shape) == (b, k, n)
        got = {name: v.cpu().numpy() for name, v in res.items()}
        after, steps_after = _snapshot(env)
        assert steps_after == steps and set(after) == set(before)
        for name in before:                                              # the env is untouched
            assert torch.equal(before[name], after[name]), name
        for q in range(k):
            _, _, _, info = env.step(actions[:, q].contiguous())
            assert np.array_equal(_bits(info['sinr_db'].cpu().numpy()), _bits(got['sinr_db'][:, q])), q
            assert np.array_equal(_bits(info['capacity_mbps'].cpu().numpy()), _bits(got['capacity_mbps'][:, q])), q
        total64 = got['capacity_mbps'].astype(np.float64).sum(axis=2)
        assert np.abs(got['total_mbps'] / total64 - 1.0).max() <= 1e-6 and (total64 > 0).all()
        # the env's own current planes, K = 1: the last step's planes
        cur = env.evaluate(env._t['rb'].unsqueeze(1).contiguous(), env._t['pwr'].unsqueeze(1).contiguous())
        assert tuple(cur['sinr_db'].shape) == (b, 1, n)
        assert np.array_equal(_bits(cur['sinr_db'][:, 0].cpu().numpy()), _bits(info['sinr_db'].cpu().numpy()))
        assert np.array_equal(_bits(cur['capacity_mbps'][:, 0].cpu().numpy()), _bits(info['capacity_mbps'].cpu().numpy()))
        # totals only: no [B, K, N] block; the env's tensors are reused while K stays and replaced when it changes
        tot = env.evaluate_actions(actions, planes=())
        assert set(tot) == {'total_mbps'} and tot['total_mbps'] is not res['total_mbps']          # K went 6 -> 1 -> 6
        tot2 = env.evaluate_actions(actions, planes=('capacity_mbps',))
        assert set(tot2) == {'total_mbps', 'capacity_mbps'} and tot2['total_mbps'] is tot['total_mbps']
        assert env.status_flags() == 0
    finally:
        env.close()


def test_out_is_honoured_and_bad_arguments_are_refused_by_name():
    env = _env('agent', 'default')
    try:
        env.reset(seed=2)
        b, n, k = 4, 25, 3
        rng = np.random.default_rng(8)
        rb = torch.as_tensor(rng.integers(0, 7, (b, k, n)).astype(np.int32), device=env.device)
        pwr = torch.as_tensor(rng.integers(0, 20, (b, k, n)).astype(np.int32), device=env.device)
        own = {name: v.clone() for name, v in env.evaluate(rb, pwr).items()}
        out = {'total_mbps': torch.empty((b, k), device=env.device), 'sinr_db': torch.empty((b, k, n), device=env.device)}
        got = env.evaluate(rb, pwr, planes=('sinr_db',), out=out)
        assert got['total_mbps'] is out['total_mbps'] and got['sinr_db'] is out['sinr_db'] and set(got) == set(out)
        assert torch.equal(out['sinr_db'], own['sinr_db']) and torch.equal(out['total_mbps'], own['total_mbps'])
        for bad_rb, bad_pwr, text in ((rb.long(), pwr, 'rb must be'), (rb[:, :, :-1].contiguous(), pwr, 'rb must be'),
                                      (rb.transpose(0, 1), pwr, 'rb must be'), (rb[:, 0], pwr, 'rb must be'), (rb.cpu(), pwr, 'rb must be'),
                                      (rb, pwr.float(), 'power_dbm must be'), (rb, pwr[:, :2].contiguous(), 'one shape'),
                                      (rb[:, :0].contiguous(), pwr[:, :0].contiguous(), 'rb must be')):
            with pytest.raises(ValueError, match=text):
                env.evaluate(bad_rb, bad_pwr)
        for bad in (out['total_mbps'], {'total_mbps': out['total_mbps']}, dict(out, sinr_db=out['sinr_db'].double()),
                    dict(out, capacity_mbps=torch.empty((b, k, n), device=env.device)), dict(out, total_mbps=out['total_mbps'][:, :2]),
                    dict(out, sinr_db=out['sinr_db'].cpu())):
            with pytest.raises(ValueError, match='out must be'):
                env.evaluate(rb, pwr, planes=('sinr_db',), out=bad)
        with pytest.raises(ValueError, match='planes must be'):
            env.evaluate(rb, pwr, planes=('snr_db',))
        with pytest.raises(ValueError, match='actions must be'):
            env.evaluate_actions(torch.zeros((b, k, n + 1), dtype=torch.int32, device=env.device))
        with pytest.raises(ValueError, match='actions must be'):
            env.evaluate_actions(torch.zeros((b, k, n), device=env.device))
    finally:
        env.close()


def test_unsupported_routes_are_refused_by_name(tmp_path):
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
            planes = torch.zeros((2, 1, 6), dtype=torch.int32, device=env.device)
            with pytest.raises(ValueError, match=text):
                env.evaluate(planes, planes.clone())
            with pytest.raises(ValueError, match=text):
                env.evaluate_actions(torch.zeros((2, 1, 6), dtype=torch.int32, device=env.device))
        finally:
            env.close()
    refused(r'evaluate\(\).*export_actions', export_actions=False)
    refused(r'evaluate\(\).*ShadowingPathLoss', {'path_loss_model': ShadowingPathLoss})
    refused(r"evaluate\(\).*'link_table'", {'path_loss_model': Foo})
    refused(r"evaluate\(\).*'array'", {'path_loss_model': Arr})
    refused(r"evaluate\(\).*'per_step'", {'path_loss_model': PerStep})
    pinned = tmp_path / 'pinned.json'
    pinned.write_text(json.dumps({'cue00': {'position': [100.1, -20.3], 'config': {'max_tx_power_dBm': 23}}}))
    refused(r'evaluate\(\).*float32 cannot hold', {'device_config_file': pinned})

"""Every enqueue-only API of VecD2DEnv on a side stream behind a sleeping GPU (tests/stream_order_util.py has the harness).

"Enqueued on torch's current stream, nothing is synchronised" is checked two ways per case: the host returns from the whole round
while the GPU has not yet finished the sleep queued in front of it (`gate` still pending), and the results equal, byte for byte,
those of a twin env that made the same calls one at a time on the null stream with a device synchronise after each.  Three kinds
of mistake show here and nowhere else in the suite: a launch that does not carry the stream (it runs early and reads the state of
the step before), a temporary freed while its reader is still queued on another stream, and a hidden host synchronisation.

The argument forms that do synchronise, by design, are the cases marked xfail(strict=True): a `movable` TENSOR of the calls whose
output shapes depend on the number of movable links, and a `margin_db` TENSOR of color_rbs(), whose NaN refusal reads it.
"""
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def so(native):
    import torch
    import stream_order_util as u
    harness = u.Harness(torch.device('cuda', torch.cuda.current_device()))
    twins = u.Twins()
    yield u, harness, twins
    twins.close()
    rows = [row[:4] for row in harness.log if row[4]]                # the cases that did not wait for the GPU
    if rows:
        case, slept, warm, test = min(rows, key=lambda row: row[1] / max(row[2], row[3]))
        print(f'\nsmallest sleep / host-time ratio of the enqueue-only cases: {slept / max(warm, test):.0f} ({case}: slept {slept:.1f} ms, round '
              f'{max(warm, test):.3f} ms); {harness.cycles_per_ms:.0f} sleep cycles per ms')


def run_case(so, case: str, feature: str, fn=None, steps: int = 1):
    """One case on the twins of `feature`; a case that does not reach its end leaves them to be rebuilt."""
    u, harness, twins = so
    pair = twins.get(feature)
    twins.dirty.add(feature)
    res = harness.run(case, pair, fn, steps)
    twins.dirty.discard(feature)
    return res


def check(so, res) -> None:
    u = so[0]
    assert res.pending, 'the host waited for the GPU: the sleep queued before the round had ended when the round returned'
    assert res.slept_ms >= u.MIN_SLEEP_MS and res.slept_ms >= u.MIN_RATIO * max(res.host_ms, res.test_ms), \
        f'the sleep was too short to tell: {res.slept_ms:.1f} ms for a round of {max(res.host_ms, res.test_ms):.3f} ms'
    diff = u.mismatches(res.got, res.want)
    assert not diff, f'differs from the twin on the null stream: {diff}'


# ---------------------------------------------------------------------------------------------------------------- the steps
STEP_CASES = ['linear', 'autoreset', 'mobility', 'traffic', 'channel', 'per_step', 'neighbor_obs']


def _extras(feature: str):
    """What a feature set shows beyond step()'s own return: its planes, read right behind the last step."""
    if feature == 'mobility':
        return lambda env, a: (env.link_positions(), env.velocities(), env.neighbors(1))
    if feature == 'traffic':
        return lambda env, a: env.queues()
    if feature == 'channel':
        return lambda env, a: (env.path_loss_db(), env.link_positions(), env.velocities())
    return None


@pytest.mark.parametrize('feature', STEP_CASES)
def test_three_steps_behind_a_sleep(so, feature):
    """step() alone (LinearObs), with autoreset and staggered episodes - some envs reset behind the sleep: masked reset, merge,
    advance - with mobility, packet queues, the spatial channel and a per-step ArrayPathLoss, and under a neighbour obs function
    with autoreset (the reset-time reselection and the gather of _observe)."""
    u, harness, twins = so
    res = run_case(so, f'step[{feature}]', feature, _extras(feature), steps=3)
    if feature == 'per_step':
        table = twins.get(feature)[1].env.simulator.path_loss_table
        assert table.live_bound and table.stream == harness.side.cuda_stream    # before_step took its `same` branch: no synchronise
    if feature in ('autoreset', 'neighbor_obs'):
        reset = twins.get(feature)[1].env._t['reset']
        resets = [int(t.sum()) for name, t in res.want.items() if t.dtype == reset.dtype and t.shape == reset.shape]
        assert any(0 < k < u.B for k in resets), f'no step of the round reset a part of the envs: {resets}'
    check(so, res)


# ---------------------------------------------------------------------------------------------------------------- the APIs
def _subset(form: str, host, tensor):
    return tensor if form == 'tensor' else host


def _api_cases():
    """name -> fn(u, env, a, form): the call under test with device arguments made behind the sleep."""
    c = {}
    c['sense[sinr_db]'] = lambda u, env, a, f: env.sense('sinr_db')
    c['sense[interference_mw]'] = lambda u, env, a, f: env.sense('interference_mw')
    c['coupling'] = lambda u, env, a, f: env.coupling()
    c['neighbors'] = lambda u, env, a, f: env.neighbors(u.K)
    c['marginal_capacity'] = lambda u, env, a, f: env.marginal_capacity()
    c['best_rb'] = lambda u, env, a, f: env.best_rb(a.allowed)
    # env_mask: the rows of an env that is masked out are kept, so an unmasked call with other arguments comes first - every row is
    # then a value of this round, and a mask that was not honoured shows
    def power_control(u, env, a, f):
        env.power_control(a.floor, _subset(f, u.ADJUSTABLE, a.adjustable), 16)
        return env.power_control(a.target, _subset(f, u.ADJUSTABLE, a.adjustable), 16, env_mask=a.env_mask)

    def balance_sinr(u, env, a, f):
        env.balance_sinr(a.floor, None, None, _subset(f, u.ADJUSTABLE, a.adjustable), 16)
        return env.balance_sinr(a.target, None, a.floor, _subset(f, u.ADJUSTABLE, a.adjustable), 16, env_mask=a.env_mask)

    def power_ascent(u, env, a, f):
        env.power_ascent(_subset(f, u.ADJUSTABLE, a.adjustable), None, start='min')
        return env.power_ascent(_subset(f, u.ADJUSTABLE, a.adjustable), a.floor, env_mask=a.env_mask)

    def best_response_dynamics(u, env, a, f):
        env.best_response_dynamics(None, _subset(f, u.MOVABLE, a.movable), min_gain_db=9.0)
        return env.best_response_dynamics(a.allowed, _subset(f, u.MOVABLE, a.movable), env_mask=a.env_mask)
    c.update(power_control=power_control, balance_sinr=balance_sinr, power_ascent=power_ascent, best_response_dynamics=best_response_dynamics)
    c['evaluate'] = lambda u, env, a, f: env.evaluate(a.rb_cand, a.pw_cand)
    c['evaluate_actions'] = lambda u, env, a, f: env.evaluate_actions(a.act_cand)
    c['assignment_weights'] = lambda u, env, a, f: env.assignment_weights(_subset(f, u.MOVABLE5, a.movable), a.allowed, harm=True)
    c['solve_assignment'] = lambda u, env, a, f: env.solve_assignment(a.weights)
    c['assign_rbs'] = lambda u, env, a, f: env.assign_rbs(u.MOVABLE5, a.allowed)
    c['solve_stable_matching'] = lambda u, env, a, f: env.solve_stable_matching(a.link_pref, a.rb_pref, a.quota)
    c['stable_rbs'] = lambda u, env, a, f: env.stable_rbs(None, a.allowed, a.quota)
    c['sharing_values'] = lambda u, env, a, f: env.sharing_values(u.MOVABLE4, a.allowed, a.power)
    c['solve_sharing'] = lambda u, env, a, f: env.solve_sharing(a.values, a.quota)
    c['share_rbs'] = lambda u, env, a, f: env.share_rbs(u.MOVABLE4, a.allowed, a.quota, a.power)
    c['joint_assignment_weights'] = lambda u, env, a, f: env.joint_assignment_weights(u.MOVABLE5, a.allowed, a.floor)
    c['assign_rbs_power'] = lambda u, env, a, f: env.assign_rbs_power(u.MOVABLE5, a.allowed, a.floor)
    c['color_graph'] = lambda u, env, a, f: env.color_graph(a.score, a.rx_thr, None, _subset(f, u.MOVABLE, a.movable), a.allowed)
    c['color_rbs'] = lambda u, env, a, f: env.color_rbs(a.target if f == 'margin_tensor' else 5.0, _subset(f, u.MOVABLE, a.movable),
                                                        a.allowed, a.power)
    c['link_positions'] = lambda u, env, a, f: env.link_positions()
    return c


API_CASES = _api_cases()
# the calls that take `adjustable` / `movable` through PairKernel.agent_subset: a tensor is combined with the agent links on the device
TENSOR_SUBSETS = ['power_control', 'balance_sinr', 'power_ascent', 'best_response_dynamics', 'color_graph', 'color_rbs']
SYNCHRONISES = [
    pytest.param('assignment_weights', 'tensor', marks=pytest.mark.xfail(strict=True, reason=(
        'a movable TENSOR is read on the host (Assignment.links): the number of movable links shapes every output of the assignment, '
        'stable-matching, sharing and joint-assignment calls'))),
    pytest.param('color_rbs', 'margin_tensor', marks=pytest.mark.xfail(strict=True, reason=(
        'a margin_db TENSOR is read on the host (Coloring.margin): NaN is refused by value'))),
]


@pytest.mark.parametrize('name,form', [(name, 'host') for name in API_CASES] + [(name, 'tensor') for name in TENSOR_SUBSETS] + SYNCHRONISES)
def test_api_behind_a_step_and_a_sleep(so, name, form):
    """A fresh step and then the call, `allowed`, `env_mask`, targets, floors, candidates, weights, preference planes, quotas and
    powers as device tensors written behind the sleep; `adjustable` / `movable` as host arrays (cached by the warm rounds) and, for
    the calls that take them through agent_subset, as device tensors too."""
    u = so[0]
    fn = API_CASES[name]
    check(so, run_case(so, f'{name}[{form}]', 'plain', lambda env, a: fn(u, env, a, form)))


# ---------------------------------------------------------------------------------------------------------------- *_actions
ACTION_CASES = {
    'best_response_actions': lambda u, env, a: env.best_response_actions(a.allowed),
    'power_control_actions': lambda u, env, a: env.power_control_actions(a.target, u.ADJUSTABLE, 16),
    'balance_sinr_actions': lambda u, env, a: env.balance_sinr_actions(a.target, None, a.floor, u.ADJUSTABLE, 16),
    'power_ascent_actions': lambda u, env, a: env.power_ascent_actions(a.adjustable, a.floor),
    'best_response_dynamics_actions': lambda u, env, a: env.best_response_dynamics_actions(a.allowed, a.movable),
    'assign_rbs_actions': lambda u, env, a: env.assign_rbs_actions(u.MOVABLE5, a.allowed),
    'stable_rbs_actions': lambda u, env, a: env.stable_rbs_actions(None, a.allowed, a.quota),
    'share_rbs_actions': lambda u, env, a: env.share_rbs_actions(u.MOVABLE4, a.allowed, a.quota, a.power),
    'assign_rbs_power_actions': lambda u, env, a: env.assign_rbs_power_actions(u.MOVABLE5, a.allowed, a.floor),
    'color_rbs_actions': lambda u, env, a: env.color_rbs_actions(5.0, u.MOVABLE, a.allowed, a.power),
}


@pytest.mark.parametrize('name', list(ACTION_CASES))
def test_actions_form_feeds_the_next_step(so, name):
    """The composition users write: a step, the *_actions call - two or three launches and torch ops - and its tensor straight into
    the next step(), all behind one sleep; the actions and the next step's rb, tx_pwr_dbm and sinr_db planes equal the twin's."""
    u = so[0]

    def fn(env, a):
        actions = ACTION_CASES[name](u, env, a)
        info = env.step(actions)[3]
        return actions, info['rb'], info['tx_pwr_dbm'], info['sinr_db']
    check(so, run_case(so, name, 'plain', fn))


# ---------------------------------------------------------------------------------------------------------------- stream switches
def test_stream_switch_in_mid_episode(so):
    """null stream -> side stream A -> side stream B -> null stream, ordered by wait_stream alone, no device synchronise before the
    end.  On every stream a sleep comes first, then fresh arguments, then power_control() and best_rb() - in turn the first call
    behind the switch, so each of them has to follow the stream itself - then the step.  The trajectory equals the twin's."""
    import torch
    u, harness, twins = so
    ref, sub = twins.get('plain')
    twins.dirty.add('plain')

    def segment(env, side, k, sync=False):
        side.args.refresh(side.gen)
        if sync:
            torch.cuda.synchronize()
        calls = [lambda: env.power_control(side.args.target, u.ADJUSTABLE, 16, env_mask=side.args.env_mask),
                 lambda: env.best_rb(side.args.allowed)]
        out = []
        for call in calls[::-1] if k % 2 else calls:
            out += [t.clone() for t in u.flatten(call())]
        out += [t.clone() for t in u.flatten(env.step(side.args.actions))]
        return out

    synced = u.Synced(ref.env)
    want = [segment(synced, ref, k, sync=True) for k in range(4)]
    null = torch.cuda.default_stream(harness.device)
    streams = [null, torch.cuda.Stream(device=harness.device), torch.cuda.Stream(device=harness.device), null]
    got, prev = [], None
    for k, stream in enumerate(streams):
        if prev is not None:
            stream.wait_stream(prev)
        with torch.cuda.stream(stream):
            harness.sleep(u.MIN_SLEEP_MS)
            got.append(segment(sub.env, sub, k))
        prev = stream
    torch.cuda.synchronize()
    twins.dirty.discard('plain')
    diff = [(k, j) for k in range(4) for j in range(len(want[k])) if not u.same_bytes(got[k][j], want[k][j])]
    assert not diff, f'(segment, tensor) that differ from the twin on the null stream: {diff}'

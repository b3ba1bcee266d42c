"""Every refusal text and every out= ValueError text of the stateless pair kernels' host modules, against
tests/golden/pair_kernel_messages.json: the texts `collect` gave on the commit before the host plumbing was stated once.  Stub sim,
kernel objects on torch.device('cpu'), the _native wrappers replaced by no-ops: nothing is loaded or launched."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'pair_kernel_messages.json'
MODULES = ('sensing', 'graph', 'marginal', 'best_response', 'power_control', 'best_response_dynamics', 'evaluate', 'assignment',
           'joint_assignment', 'coloring')
TORCH_ONLY = MODULES[3:]
LAUNCHES = ('sense_rb', 'graph_coupling', 'graph_neighbors', 'marginal_capacity', 'best_rb', 'power_control', 'best_response_dynamics',
            'evaluate', 'assign_weights', 'assign_solve', 'assign_power_weights', 'color_graph')
B, N, R = 3, 4, 4                                   # the stub's own: 3 envs, 4 links, 4 RBs


def _stub_sim(route=None, shadowing=False):
    from gym_d2d_amd.path_loss_table import NATIVE
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    law = {'a_tx_db': [30.0] * 7, 'a_rx_db': [0.0] * 7, 'exponent': [3.5] * 7, 'shadowing': shadowing}
    return SimpleNamespace(num_envs=B, handle=SimpleNamespace(num_devices=7), config=SimpleNamespace(num_rbs=R),
                           link_tx=np.asarray([1, 2, 3, 5]), link_rx=np.asarray([0, 0, 4, 6]), _dev_list=[dev] * 7,
                           path_loss_table=SimpleNamespace(route=NATIVE if route is None else route, law=law),
                           fixed_positions=lambda: (np.zeros(7, bool), np.zeros((7, 2))))


def _refusals():
    import importlib
    pinned = _stub_sim()
    pinned.fixed_positions = lambda: (np.array([True] + [False] * 6), np.array([[100.1, -20.3]] + [[0, 0]] * 6))
    stubs = {'served': (_stub_sim(), True), 'export_actions': (_stub_sim(), False), 'link_table': (_stub_sim(route='link_table'), True),
             'per_step': (_stub_sim(route='per_step'), True), 'channel': (_stub_sim(route='channel'), True),
             'shadowing': (_stub_sim(shadowing=True), True), 'pinned': (pinned, True)}
    texts = {}
    for name in MODULES:
        module = importlib.import_module(f'gym_d2d_amd.{name}')
        for case, args in stubs.items():
            texts[f'{name}.refusal/{case}'] = module.refusal(*args)
        if name in TORCH_ONLY:
            texts[f'{name}.refusal/numpy_path'] = module.refusal(_stub_sim(), True, use_torch=False)
    return texts


def _text(call):
    """The ValueError's text, or None where the call passes."""
    try:
        call()
    except ValueError as e:
        return str(e)
    return None


def _noncontiguous(torch, shape, dtype):
    return torch.zeros(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]


def _bad_tuples(torch, shapes, dtypes):
    """The fixed set of bad out= tuples for a result of these shapes and dtypes, by case name."""
    good = lambda: [torch.zeros(s, dtype=dt) for s, dt in zip(shapes, dtypes)]
    swap = lambda i, t: tuple(t if j == i else o for j, o in enumerate(good()))
    last = len(shapes) - 1
    other = torch.float64 if dtypes[last] != torch.float64 else torch.int32
    cases = {'wrong_length': tuple(good()[:-1]) if last else (),
             'wrong_shape_first': swap(0, torch.zeros(*shapes[0][:-1], shapes[0][-1] + 1, dtype=dtypes[0])),
             'wrong_dtype_last': swap(last, torch.zeros(shapes[last], dtype=other)),
             'noncontiguous': swap(0, _noncontiguous(torch, shapes[0], dtypes[0])),
             'not_a_sequence': good()[0] if last else 'out',
             'not_tensors': tuple(np.zeros(s) for s in shapes)}
    if last:
        # the last two slots as views of one buffer: the same data_ptr under their own shapes and dtypes
        buf = torch.zeros(max(int(np.prod(s)) * dt.itemsize for s, dt in zip(shapes[-2:], dtypes[-2:])), dtype=torch.uint8)
        views = [buf[:int(np.prod(s)) * dt.itemsize].view(dt).view(s) for s, dt in zip(shapes[-2:], dtypes[-2:])]
        cases['shared_memory'] = (*good()[:-2], *views)
    return cases


def _bad_tensors(torch, shape, dtype):
    """The fixed set of bad single out= tensors of this shape and dtype, by case name."""
    return {'wrong_shape': torch.zeros(*shape[:-1], shape[-1] + 1, dtype=dtype),
            'wrong_dtype': torch.zeros(shape, dtype=torch.float64),
            'noncontiguous': _noncontiguous(torch, shape, dtype),
            'not_a_tensor': np.zeros(shape, dtype=np.float32)}


def _out_checks():
    import torch
    from gym_d2d_amd import (assignment, best_response, best_response_dynamics, coloring, evaluate, graph, joint_assignment, marginal,
                             power_control, sensing)
    cpu, sim = torch.device('cpu'), _stub_sim()
    i32, f32, u8 = torch.int32, torch.float32, torch.uint8
    agent, due = np.array([False, True, True, True]), np.array([False, False, True, True])      # link 0 is on fixed actions
    p_min, p_max = np.zeros(N, dtype=np.int32), np.full(N, 3, dtype=np.int32)
    t = {'pos_x': torch.zeros(B, 7), 'pos_y': torch.zeros(B, 7), 'rb': torch.zeros(B, N, dtype=i32), 'pwr': torch.zeros(B, N, dtype=i32)}
    m = int(due.sum())
    texts = {}

    def tuples(name, shapes, dtypes, call):
        for case, out in _bad_tuples(torch, shapes, dtypes).items():
            texts[f'{name}/{case}'] = _text(lambda: call(out))

    def tensors(name, shape, dtype, call):
        for case, out in _bad_tensors(torch, shape, dtype).items():
            texts[f'{name}/{case}'] = _text(lambda: call(out))

    k = best_response.BestRb(sim, N, torch, cpu)
    tuples('BestRb.planes', ((B, N),) * 3, (i32, f32, f32), lambda out: k.planes(t, None, out, 0))

    k = power_control.PowerControl(sim, N, p_min, p_max, agent, torch, cpu)
    shapes, dtypes = ((B, N), (B, N), (B,), (B,)), (i32, f32, i32, u8)
    tuples('PowerControl.outputs', shapes, dtypes, k.outputs)
    target, adjustable = k.target(3.0, 2), k.adjustable(None)
    tuples('PowerControl.solve', shapes, dtypes, lambda out: k.solve(t, target, adjustable, 4, out, 0))

    k = best_response_dynamics.BestResponseDynamics(sim, N, agent, torch, cpu)
    shapes, dtypes = ((B, N), (B, N), (B,), (B,), (B,)), (i32, f32, i32, i32, u8)
    tuples('BestResponseDynamics.outputs', shapes, dtypes, k.outputs)
    movable = k.movable(None)
    tuples('BestResponseDynamics.solve', shapes, dtypes, lambda out: k.solve(t, None, movable, 3.0, 4, out, 0))

    k = coloring.Coloring(sim, N, agent, torch, cpu)
    shapes, dtypes = ((B, N), (B,), (B,), (B,)), (i32, i32, i32, u8)
    tuples('Coloring.outputs', shapes, dtypes, k.outputs)
    score, thr, movable = torch.zeros(B, N, N), torch.zeros(B, N), k.movable(None)
    tuples('Coloring.color', shapes, dtypes, lambda out: k.color(t['rb'], score, thr, None, movable, None, False, out, 0))
    tensors('Coloring.plane(score)', (B, N, N), f32, lambda v: k.plane(v, 'score', (B, N, N)))
    tensors('Coloring.plane(tx_bias)', (B, N), f32, lambda v: k.plane(v, 'tx_bias', (B, N), optional=True))
    texts['Coloring.plane(rx_thr)/none'] = _text(lambda: k.plane(None, 'rx_thr', (B, N)))
    texts['Coloring.plane(tx_bias)/none'] = _text(lambda: k.plane(None, 'tx_bias', (B, N), optional=True))

    for name, k in (('Assignment', assignment.Assignment(sim, N, agent, due, torch, cpu)),
                    ('JointAssignment', joint_assignment.JointAssignment(sim, N, agent, due, p_min, p_max, torch, cpu))):
        tuples(f'{name}.weights(harm)', ((B, m, R),) * 2, (f32, f32), lambda out: k.weights(t, None, None, 'total', True, out, 0))
        tuples(f'{name}.weights', ((B, m, R),), (f32,), lambda out: k.weights(t, None, None, 'total', False, out, 0))
        tensors(f'{name}.weights(tensor)', (B, m, R), f32, lambda out: k.weights(t, None, None, 'own', False, out, 0))
        w = torch.zeros(B, m, R)
        tuples(f'{name}.solve', ((B, m), (B,), (B,)), (i32, f32, u8), lambda out: k.solve(w, out, 0))
        tuples(f'{name}.assign', ((B, N), (B,), (B,)), (i32, f32, u8), lambda out: k.assign(t, None, None, 'total', out, 0))
    tuples('JointAssignment.power_weights', ((B, m, R),) * 2, (f32, i32), lambda out: k.power_weights(t, None, None, None, out, 0))
    tuples('JointAssignment.assign_power', ((B, N), (B, N), (B,), (B,)), (i32, i32, f32, u8),
           lambda out: k.assign_power(t, None, None, None, out, 0))

    k = marginal.MarginalCapacity(sim, N, torch, cpu)
    tuples('MarginalCapacity.torch_planes', ((B, N),) * 2, (f32, f32), lambda out: k.torch_planes(t, out, 0))
    one = torch.zeros(B, N)
    texts['MarginalCapacity.torch_planes/same_tensor_twice'] = _text(lambda: k.torch_planes(t, (one, one), 0))

    k = evaluate.Evaluate(sim, N, torch, cpu)
    rb = pwr = torch.zeros(B, 2, N, dtype=i32)
    names, shapes = ('total_mbps', 'sinr_db', 'capacity_mbps'), ((B, 2), (B, 2, N), (B, 2, N))
    for case, out in _bad_tuples(torch, shapes, (f32,) * 3).items():
        out = dict(zip(names, out)) if isinstance(out, tuple) else out
        texts[f'Evaluate.planes/{case}'] = _text(lambda: k.planes(t, rb, pwr, evaluate.PLANES, out, 0))
    wrong_key = {'total': torch.zeros(B, 2), 'sinr_db': torch.zeros(B, 2, N), 'capacity_mbps': torch.zeros(B, 2, N)}
    texts['Evaluate.planes/wrong_key'] = _text(lambda: k.planes(t, rb, pwr, evaluate.PLANES, wrong_key, 0))
    extra_key = {'total_mbps': torch.zeros(B, 2), 'sinr_db': torch.zeros(B, 2, N)}
    texts['Evaluate.planes/key_not_asked_for'] = _text(lambda: k.planes(t, rb, pwr, ('capacity_mbps',), extra_key, 0))

    k = graph.NeighborGraph(sim, N, torch, cpu)
    tensors('NeighborGraph.coupling_torch', (B, N, N), f32, lambda out: k.coupling_torch(t, out, 0))
    tuples('NeighborGraph.neighbors_torch', ((B, N, 2),) * 2, (i32, f32), lambda out: k.neighbors_torch(t, 2, out, 0))
    tensors('NeighborGraph.neighbors_torch(idx)', (B, N, 2), i32, lambda out: k.neighbors_torch(t, 2, (out, torch.zeros(B, N, 2)), 0))

    k = sensing.RbSensor(sim, N, torch, cpu)
    tensors('RbSensor.sense_torch', (B, N, R), f32, lambda out: k.sense_torch(t, sensing.WHAT['sinr_db'], out, 0))
    return texts


def collect(setattr_):
    """{case: text or None} of every refusal and every out= check; setattr_(object, name, value) replaces the launches (a test's
    monkeypatch.setattr, or the builtin)."""
    from gym_d2d_amd import _native
    for name in LAUNCHES:
        assert callable(getattr(_native, name)), name
        setattr_(_native, name, lambda *args: None)
    return {**_refusals(), **_out_checks()}


def test_every_refusal_and_out_text_is_the_one_the_copies_gave(monkeypatch):
    golden = json.loads(GOLDEN.read_text())
    got = collect(monkeypatch.setattr)
    assert len(got) == len(golden) and set(got) == set(golden)
    refusals = [key for key in got if '.refusal/' in key]
    assert len(refusals) == 7 * len(MODULES) + len(TORCH_ONLY) == 77
    assert sum(got[key] is None for key in refusals) == len(MODULES)             # 'served' alone is no refusal
    for key, text in golden.items():
        assert got[key] == text, key
    # every bad out= is refused in words but the two that are no error: an absent optional plane, and a pair whose dtypes differ
    passed = {key for key, text in got.items() if text is None and key not in refusals}
    assert passed == {'Coloring.plane(tx_bias)/none', 'NeighborGraph.neighbors_torch/shared_memory'}

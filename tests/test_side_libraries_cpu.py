"""The side libraries' shared Python half, the part that needs no GPU: the one table `_native.SIDE` against `build.LIBRARIES` and
the built .so files, the one loader `side_library` behind every `load_<name>_library`, what a missing library says, pointer
arguments passed as plain ints, and the opening `sensing.PairKernel` states once for the add-on classes."""
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from gym_d2d_amd import _native, build

NAMES = list(_native.SIDE)


def test_the_table_lists_what_the_build_builds():
    assert NAMES == [stem for stem in build.LIBRARIES if stem not in ('hip', 'probe')] and len(NAMES) == 12
    for name in NAMES:
        assert _native.side_path(name) == build.lib_path(name)
        assert _native.SIDE[name] is getattr(_native, f'{name.upper()}_SIGNATURES')


@pytest.mark.parametrize('name', NAMES)
def test_one_loader_one_object_and_exactly_the_exported_symbols(name):
    lib = _native.side_library(name)
    assert _native.side_library(name) is lib and getattr(_native, f'load_{name}_library')() is lib
    nm = subprocess.run(['nm', '-D', '--defined-only', str(build.lib_path(name))], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ' T d2d_' in ln}
    assert exported == set(_native.SIDE[name]) and f'd2d_{name}_last_error' in exported
    for symbol, (res, args) in _native.SIDE[name].items():
        assert getattr(lib, symbol).restype is res and list(getattr(lib, symbol).argtypes) == args
    assert isinstance(getattr(lib, f'd2d_{name}_last_error')(), bytes)


@pytest.mark.parametrize('name', NAMES)
def test_a_missing_library_says_how_to_build_it(name, tmp_path, monkeypatch):
    monkeypatch.setattr(_native, '_side', {})                      # nothing cached: the loader has to look
    monkeypatch.setattr(_native, 'side_path', lambda n: tmp_path / f'libd2d_{n}.so')
    missing = tmp_path / f'libd2d_{name}.so'
    with pytest.raises(ImportError) as e:
        getattr(_native, f'load_{name}_library')()
    assert str(e.value) == f'{missing} is missing - build it with `python -m gym_d2d_amd.build`'
    assert _native._side == {}


def test_pointers_are_passed_as_plain_ints():
    top = 2 ** 64 - 8
    # nothing to do (n_envs = 0): accepted whatever the pointers hold - null, small, past 2^63 - and no ctypes conversion error
    for p in (0, 8, 2 ** 63 + 8, top):
        _native.episode_advance(p, p, p, p, p, 0, 0, 0, 1)
        _native.episode_advance(p, p, p, p, p, p, 1, 0, 1, p)
    # the library sees the values: a null among real ones is refused by name, as every per-library refusal test demands
    before = _native.sense_launches
    for ptrs in ((0,) * 7, (8, 8, 8, 8, 8, 8, 0), (top,) * 6 + (0,)):
        with pytest.raises(_native.NativeError, match='null device pointer'):
            _native.sense_rb(*ptrs, 0, 0, 2, 5, 2, 3, 0, 8)
    with pytest.raises(_native.NativeError, match='null device pointer'):
        _native.sense_rb(8, 8, 8, 8, 8, 8, 8, 0, 0, 2, 5, 2, 3, 0, 0)
    with pytest.raises(_native.NativeError, match='null device pointer'):
        _native.episode_advance(0, 8, 8, 8, 8, 0, 0, 4, 1)
    assert _native.sense_launches == before


# ---------------------------------------------------------------------------------------------- sensing.PairKernel
def _stub_sim(num_rbs=4, link_tx=(1, 2), link_rx=(0, 0)):
    dev = SimpleNamespace(tx_offset_dB=lambda: 3.0, rx_offset_dB=lambda: -1.5, thermal_noise_dBm=-116.4, rx_sensitivity_dBm=-107.5,
                          rb_bandwidth_kHz=180)
    law = {'a_tx_db': [30.0, 31.0, 32.0], 'a_rx_db': [0.0, 0.5, 1.0], 'exponent': [2.0, 3.6, 4.375]}
    return SimpleNamespace(num_envs=5, handle=SimpleNamespace(num_devices=3), config=SimpleNamespace(num_rbs=num_rbs),
                           link_tx=np.asarray(link_tx), link_rx=np.asarray(link_rx), _dev_list=[dev] * 3,
                           path_loss_table=SimpleNamespace(law=law))


def test_pair_kernel_opens_the_add_on_classes_on_the_torch_cpu_path():
    import torch
    from gym_d2d_amd import evaluate, graph, sensing
    from gym_d2d_amd.device import link_budget_columns
    sim, cpu = _stub_sim(), torch.device('cpu')
    budget = link_budget_columns(sim._dev_list)
    cols, law, pow_k = sensing.fold_columns(budget, sim.path_loss_table.law, sim.link_tx)
    cap_cols = sensing.fold_capacity_columns(budget)
    for cls, names in ((sensing.RbSensor, ('tx', 'rx', 'cols')), (evaluate.Evaluate, ('tx', 'rx', 'cols', 'cap_cols'))):
        k = cls(sim, 2, torch, cpu)
        assert isinstance(k, sensing.PairKernel) and (k.sim, k.torch, k.device) == (sim, torch, cpu)
        assert (k.b, k.d, k.n, k.r, k.law, k.pow_k) == (5, 3, 2, 4, law, pow_k) == (5, 3, 2, 4, _native.SENSE_LAW_POW_K, 4)
        assert k.ptrs == tuple(getattr(k, name).data_ptr() for name in names) and hasattr(k, 'cap_cols') == ('cap_cols' in names)
        for name, host in zip(names, (sim.link_tx.astype(np.int32), sim.link_rx.astype(np.int32), cols, cap_cols)):
            t = getattr(k, name)
            assert t.numpy().dtype == host.dtype and np.array_equal(t.numpy(), host), name
        assert not hasattr(k, 'mem')
        k.close()                                                  # the torch path owns no HIP allocation: nothing to free
    assert (sensing.RbSensor(sim, 2, torch, cpu).own, evaluate.Evaluate(sim, 2, torch, cpu).own_k) == (None, 0)
    # the graph reads no RB: no cap, no r, and a sim without a config serves it
    del sim.config
    g = graph.NeighborGraph(sim, 2, torch, cpu)
    assert (g.b, g.d, g.n, g.own) == (5, 3, 2, {}) and not hasattr(g, 'r') and len(g.ptrs) == 3
    g.close()


@pytest.mark.parametrize('module, cls, api, cap', [('sensing', 'RbSensor', 'sense', 'SENSE_MAX_RBS'),
                                                   ('evaluate', 'Evaluate', 'evaluate', 'EVALUATE_MAX_RBS')])
def test_pair_kernel_refuses_with_the_texts_and_in_the_order_of_the_classes_it_replaced(module, cls, api, cap):
    import importlib
    import torch
    make = getattr(importlib.import_module(f'gym_d2d_amd.{module}'), cls)
    top = getattr(_native, cap)
    assert top == 8192
    cpu = torch.device('cpu')
    cap_text = rf'^{api}\(\) serves at most 8192 RBs \(num_rbs = 8193\)$'
    list_text = '^the link list does not match the env$'
    with pytest.raises(ValueError, match=cap_text):
        make(_stub_sim(num_rbs=top + 1), 2, torch, cpu)
    with pytest.raises(ValueError, match=cap_text):                  # the RB cap comes first
        make(_stub_sim(num_rbs=top + 1, link_tx=(1, 3)), 2, torch, cpu)
    make(_stub_sim(num_rbs=top), 2, torch, cpu).close()             # at the cap: served
    for bad in (dict(link_tx=(1, 3)), dict(link_tx=(-1, 2)), dict(link_rx=(0, 3)), dict(link_rx=(-1, 0)), dict(link_tx=(1, 2, 2), link_rx=(0, 0, 0))):
        with pytest.raises(ValueError, match=list_text):
            make(_stub_sim(**bad), 2, torch, cpu)
    # the link list comes before the columns: a constant float32 cannot hold is refused only for a list that matches
    off = _stub_sim()
    off._dev_list = [SimpleNamespace(**{**vars(off._dev_list[0]), 'thermal_noise_dBm': -400.0})] * 3
    with pytest.raises(ValueError, match='outside the float32 linear range'):
        make(off, 2, torch, cpu)
    off.link_tx = np.asarray((1, 3))
    with pytest.raises(ValueError, match=list_text):
        make(off, 2, torch, cpu)

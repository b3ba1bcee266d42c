"""libd2d_plugin.so's d2d_plugin_normal (ArrayPathLoss's view.normal()): the built-in shadowing's normal stream, checked against
the oracle's restatement of it (ShadowSpec.normals) and independent of how the envs are split over calls."""
import numpy as np
import pytest

from oracle import d2d_oracle as orc

pytestmark = pytest.mark.gpu


def _normals(torch, n_envs, first_env, n, step, kind, seed):
    from gym_d2d_amd import _native
    shape = (n_envs, n, n) if kind == 0 else (n_envs, n)
    out = torch.empty(shape, dtype=torch.float64, device='cuda')
    _native.plugin_normal(out.data_ptr(), _native.F64, n_envs, first_env, n if kind == 0 else 1, n, step, kind, seed,
                          torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize('first_env', [1000, 70000])
@pytest.mark.parametrize('kind', [0, 1])
def test_plugin_normal_matches_the_oracle_stream(first_env, kind):
    torch = pytest.importorskip('torch')
    b, n, step, seed = 8, 300, 5, (123 << 32) | 987654321
    got = _normals(torch, b, first_env, n, step, kind, seed).cpu().numpy()
    spec = orc.ShadowSpec(seed=seed, step=step, first_env=first_env)
    env = np.arange(b)[:, None, None]
    if kind == 0:
        ref = spec.normals(env, np.arange(n)[None, :, None], np.arange(n)[None, None, :], 0)
    else:
        ref = spec.normals(env[:, :, 0], np.arange(n)[None, :], np.arange(n)[None, :], 1)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-6
    assert abs(float(got.mean())) < 0.05 and abs(float(got.std()) - 1.0) < 0.05


def test_plugin_normal_does_not_depend_on_the_env_split():
    torch = pytest.importorskip('torch')
    whole = _normals(torch, 16, 0, 37, 2, 0, 99)
    parts = torch.cat([_normals(torch, 5, 0, 37, 2, 0, 99), _normals(torch, 11, 5, 37, 2, 0, 99)])
    assert torch.equal(whole, parts)
    # float32 output: the same values, rounded once
    from gym_d2d_amd import _native
    f32 = torch.empty((16, 37, 37), dtype=torch.float32, device='cuda')
    _native.plugin_normal(f32.data_ptr(), _native.F32, 16, 0, 37, 37, 2, 0, 99, torch.cuda.current_stream().cuda_stream)
    assert torch.equal(f32, whole.float())

"""libd2d_plugin.so's d2d_plugin_normal (ArrayPathLoss's view.normal()): the built-in shadowing's normal stream, checked against
the oracle's restatement of it (ShadowSpec.normals) and independent of how the envs are split over calls; below the three first
tests, both widths inside guard elements at the shapes where csrc/d2d_plugin.hip's normal_kernel takes its other paths: tails of 1
to 3 elements, fewer elements than a vector, row and env carries inside a vector, 65536 rows, 65536 columns, more vectors than
the capped grid holds, and the refusal of a pointer off 16 bytes.  Not covered: blocks of 2^32 elements and more (the 64-bit index
arithmetic, narrow == 0: 16 GiB planes).  gain_from_db_kernel, one expression per element without an entry point of its own, is
covered by test_gpu_table_route.py through d2d_set_path_loss_link_table_dev: both widths against the float64 reference and, bit for
bit, against the conversion inside the step, and past its capped grid at 2 x 1100 x 1100 float64 and 2048 x 2048 float32 entries.

Measured on an MI355X (256 CUs): 44 tail-and-carry cases, 88 launches, worst |got - oracle| 6.76e-7 (2 x 1 x 65536, kind 1,
first_env 2^32 - 2) at the bar of 1e-6, float32 equal to float64 cast once in every case; past the capped grid 24 x 600 x 600
(float32) and 12 x 600 x 600 (float64), 2 160 000 vectors each against a grid of 2 097 152, equal bit for bit to 24 and 12
per-env launches, 0.03 s each; no test of this file over 0.05 s.  With the `r = 0; ++b` carry taken out of normal_kernel (a scratch
build), the cases (3,1,1,1), (5,3,3,0), (7,2,5,0), (3,1,37,1) and (9,37,41,0) fail, and the env-split test."""
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


# ------------------------------------------------------------------------------------------ tails, carries, the capped grid
GUARD = 64                          # elements on either side: a multiple of 16 bytes in both widths
SENTINEL = -12345.0                 # no normal of 24-bit uniforms comes near it (the largest is under 6)
SEED = (123 << 32) | 987654321
# (n_envs, n_rows, n_cols, kind): one element; one vector's worth and less; rows of one column; float32 tails of 1, 2 and 3 (the
# last a float64 tail of 1); 65536 rows of one column (every float32 vector crosses four rows, r reaches 65535); 65536 columns
# (c << 16 with the top bit of c set) in both kinds; a plain odd block of several workgroups; and 65535 rows of one column, where,
# unlike at 65536, vectors straddle two envs, so the row carry into the next env happens inside a vector at the largest r
EDGE_SHAPES = [(1, 1, 1, 0), (1, 1, 3, 0), (3, 1, 1, 1), (5, 3, 3, 0), (7, 2, 5, 0), (3, 1, 37, 1), (2, 65536, 1, 0), (2, 1, 65536, 0),
               (2, 1, 65536, 1), (9, 37, 41, 0), (3, 65535, 1, 0)]


def _guarded_normals(torch, dtype, n_envs, first_env, n_rows, n_cols, step, kind, seed):
    """One d2d_plugin_normal into the middle of a larger allocation of SENTINEL; the guards on either side are checked element by
    element and no element between them is left unwritten.  Returns the device tensor [n_envs, n_rows, n_cols]."""
    from gym_d2d_amd import _native
    total = n_envs * n_rows * n_cols
    buf = torch.full((total + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
    live = buf[GUARD:GUARD + total]
    assert live.data_ptr() % 16 == 0
    _native.plugin_normal(live.data_ptr(), _native.F64 if dtype == torch.float64 else _native.F32, n_envs, first_env, n_rows, n_cols,
                          step, kind, seed, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = f'{n_envs} x {n_rows} x {n_cols} kind {kind} {dtype}'
    assert bool((buf[:GUARD] == SENTINEL).all()), f'{what}: elements before the block were written'
    assert bool((buf[GUARD + total:] == SENTINEL).all()), f'{what}: elements after the block were written'
    assert not bool((live == SENTINEL).any()), f'{what}: elements of the block were not written'
    return live.view(n_envs, n_rows, n_cols)


def _oracle(n_envs, first_env, n_rows, n_cols, step, kind, seed):
    spec = orc.ShadowSpec(seed=seed, step=step, first_env=first_env)
    env, col = np.arange(n_envs)[:, None, None], np.arange(n_cols)[None, None, :]
    ref = spec.normals(env, np.arange(n_rows)[None, :, None] if kind == 0 else col, col, kind)
    assert ref.shape == (n_envs, n_rows, n_cols)
    return ref


@pytest.mark.parametrize('step', [0, 2 ** 32 - 1])
@pytest.mark.parametrize('last_envs', [False, True])
@pytest.mark.parametrize('n_envs,n_rows,n_cols,kind', EDGE_SHAPES)
def test_plugin_normal_tails_and_carries_match_the_oracle(n_envs, n_rows, n_cols, kind, last_envs, step):
    """Both widths inside guards, against ShadowSpec.normals at the file's bar; first_env 0 or the last envs of the 32-bit counter
    word.  Not covered: blocks of 2^32 elements and more (the 64-bit index arithmetic; 16 GiB).  (gain_from_db_kernel, which is one
    expression per element and has no entry point of its own: test_gpu_table_route.py.)"""
    torch = pytest.importorskip('torch')
    first_env = 2 ** 32 - n_envs if last_envs else 0
    ref = _oracle(n_envs, first_env, n_rows, n_cols, step, kind, SEED)
    wide = _guarded_normals(torch, torch.float64, n_envs, first_env, n_rows, n_cols, step, kind, SEED)
    narrow = _guarded_normals(torch, torch.float32, n_envs, first_env, n_rows, n_cols, step, kind, SEED)
    assert torch.equal(narrow, wide.float())
    for name, got in (('float64', wide), ('float32', narrow)):
        err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - ref)))
        total = n_envs * n_rows * n_cols
        print(f'{n_envs} x {n_rows} x {n_cols} kind {kind} first_env {first_env} step {step} {name}: tail {total % (2 if name == "float64" else 4)}, '
              f'worst |got - oracle| {err:.3g}')
        assert err <= 1e-6


@pytest.mark.parametrize('width', ['float32', 'float64'])
def test_plugin_normal_past_the_capped_grid_equals_per_env_launches(width):
    """More 16-byte vectors than 32 workgroups per CU of 256 lanes hold, so every lane takes a second trip of its loop: the block
    is, bit for bit, the per-env launches of the same arguments (each under the cap) put together; its first and last env are
    compared with the oracle."""
    torch = pytest.importorskip('torch')
    dtype, vec = (torch.float32, 4) if width == 'float32' else (torch.float64, 2)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap, n, first_env, step = 32 * cus * 256, 600, 5, 3
    n_envs = -(-(cap + 4096) * vec // (n * n))
    nvec = n_envs * n * n // vec
    print(f'{cus} CUs, {width}: {n_envs} x {n} x {n}, nvec {nvec}, cap {cap} vectors')
    assert nvec >= cap + 4096 and n * n // vec < cap
    whole = _guarded_normals(torch, dtype, n_envs, first_env, n, n, step, 0, SEED)
    for e in range(n_envs):
        one = _guarded_normals(torch, dtype, 1, first_env + e, n, n, step, 0, SEED)
        assert torch.equal(whole[e:e + 1].view(torch.uint8), one.view(torch.uint8)), f'env {e} of {n_envs}'
    for e in (0, n_envs - 1):
        err = float(np.max(np.abs(whole[e:e + 1].cpu().numpy().astype(np.float64) - _oracle(1, first_env + e, n, n, step, 0, SEED))))
        print(f'env {e}: worst |got - oracle| {err:.3g}')
        assert err <= 1e-6


@pytest.mark.parametrize('width', ['float32', 'float64'])
def test_plugin_normal_refuses_a_pointer_off_16_bytes_by_name(width):
    torch = pytest.importorskip('torch')
    from gym_d2d_amd import _native
    dtype = torch.float32 if width == 'float32' else torch.float64
    buf = torch.full((45 + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
    off = buf[GUARD + 1:]
    assert off.data_ptr() % 16 != 0
    with pytest.raises(_native.NativeError, match='out_dev must be 16-byte aligned'):
        _native.plugin_normal(off.data_ptr(), _native.F64 if width == 'float64' else _native.F32, 5, 0, 3, 3, 1, 0, SEED,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())

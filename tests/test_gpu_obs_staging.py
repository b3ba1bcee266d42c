"""The flat LinearObs expansion kernels' single-trip staging (T[env] staged with 16-byte loads, all issued before the first wait, every
piece's index arithmetic ahead of the barrier): D2D_BUF_OBS must equal expand_table_torch of the table the same step wrote, bit
for bit - the expansion is a copy - under the planner's store policy, under policy 1 and under policy 0, as float32 and as
float64, and once more through d2d_expand_table.  The shapes are the ones at which the staging takes another path."""
import numpy as np
import pytest

from sim_util import random_batch

pytestmark = pytest.mark.gpu

# (id, envs, links, tuning keys set for the shape)
SHAPES = [
    ('n2_unfused_one_partly_filled_workgroup', 3, 2, {'TUNE_STEP_FUSE_OBS': 0}),     # 3 float4 of T, 6 float4 of output: all tail guards
    ('n130_no_xcd_grouping', 9, 130, {}),                                            # smallest even N not fused; B % 8 != 0
    ('n130_xcd_grouping', 16, 130, {}),
    ('n684_two_staged_pieces', 8, 684, {}),                                          # 1026 float4 of T: some threads stage two pieces
    ('n2048_three_staged_pieces', 2, 2048, {}),                                      # 48 KB of LDS, 201 MB of output
    ('n131_odd_8byte_rows', 4, 131, {}),                                             # the row-aligned 8-byte kernel; float64: 8-byte staging
    *[(f'n512_pieces{p}_block{blk}', 8, 512, {'TUNE_OBS_ROWS_PER_WG': p, 'TUNE_OBS_BLOCK': blk})
      for p in (2, 3, 4) for blk in (512, 1024)],
    ('n2048_block256_staging_loops', 1, 2048, {'TUNE_OBS_BLOCK': 256}),              # more than three pieces per thread: the staging loop
]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_obs_block_is_the_expansion_of_the_steps_table(native, shape, dtype):
    import torch
    from gym_d2d_amd.distributed import expand_table, expand_table_torch
    _, b, n, tune = shape
    cues = n // 2
    sim, pos, raw = random_batch(b, max(1, n // 2), cues, n - cues, rng_seed=n + b)
    h = sim.handle
    h.set_obs_mode(native.OBS_LINEAR)
    for key, value in tune.items():
        h.set_tuning(getattr(native, key), value)
    f64 = dtype == 'float64'
    if f64:
        h.set_obs_dtype(native.F64)
    obs = torch.empty((b, n, 6 * n), dtype=torch.float64 if f64 else torch.float32, device='cuda')
    h.bind_buffer(native.BUF_OBS, obs.data_ptr(), obs.numel() * obs.element_size())
    bits = lambda x: x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)      # exact, and NaN compares equal to itself
    ref = table = None
    for policy in (-1, 1, 0):                                # the planner's choice, nontemporal, plain
        h.set_tuning(native.TUNE_OBS_NONTEMPORAL, policy)
        obs.fill_(float('nan'))
        torch.cuda.synchronize()
        sim.step_arrays(raw)
        t = torch.from_numpy(np.ascontiguousarray(sim.fetch(native.BUF_OBS_TABLE))).cuda()
        torch.cuda.synchronize()
        if ref is None:
            table, ref = t, expand_table_torch(t)
            ref = ref.double() if f64 else ref
        assert torch.equal(bits(t), bits(table)), policy     # the same step: the same table
        assert torch.equal(bits(obs), bits(ref)), (policy, torch.nonzero(bits(obs) != bits(ref))[:3].tolist())
    h.set_tuning(native.TUNE_OBS_NONTEMPORAL, -1)
    out = expand_table(table, h)                             # d2d_expand_table: float32, this handle's tuning
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(expand_table_torch(table)))
    h.close()

"""The flat LinearObs expansion kernels with scalar (preloadable) kernel arguments, the block size a template constant at 1024 and
512 threads and read from blockDim elsewhere: D2D_BUF_OBS must equal expand_table_torch of the table the same step wrote, bit for
bit - the expansion is a copy - under the planner's store policy, under policy 1 and under policy 0, as float32 and as float64,
and once more through d2d_expand_table.  The block is bound with a sentinel band behind it, which must come back untouched.  The
shapes are the smallest at which the 16-byte staging of T[env] takes another path (a partly filled wave, a wave boundary, a second
and third piece, the staging loop of a small block), whichever way the float4 travel to LDS."""
import numpy as np
import pytest

from sim_util import random_batch

pytestmark = pytest.mark.gpu

BAND_BYTES = 4096
UNFUSED = {'TUNE_STEP_FUSE_OBS': 0}           # N <= 128: the step kernel would write the block itself

# (id, envs, links, tuning keys set for the shape)
SHAPES = [
    ('n2_one_partly_filled_wave', 3, 2, UNFUSED),                     # 3 float4 of T: one wave of 3 lanes, fifteen with no piece
    ('n42_one_lane_short_of_a_wave', 5, 42, UNFUSED),                 # 63 float4
    ('n86_two_waves_and_one_lane', 8, 86, UNFUSED),                   # 129 float4
    ('n130_no_xcd_grouping', 9, 130, {}),                             # B % 8 != 0
    ('n130_xcd_grouping', 16, 130, {}),
    ('n684_second_piece_of_two_lanes', 8, 684, {}),                   # 1026 float4
    ('n2048_three_pieces', 2, 2048, {}),                              # 48 KB of LDS
    ('n2048_block256_staging_loop', 1, 2048, {'TUNE_OBS_BLOCK': 256}),
    *[(f'n512_pieces{p}_block{blk}', 8, 512, {'TUNE_OBS_ROWS_PER_WG': p, 'TUNE_OBS_BLOCK': blk})
      for p in (2, 3, 4) for blk in (512, 1024)],
    ('n131_odd_8byte_staging', 4, 131, {}),                           # the row-aligned 8-byte kernel; float64: 8-byte staging
]


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('shape', SHAPES, ids=[s[0] for s in SHAPES])
def test_obs_block_is_the_expansion_and_the_band_behind_it_is_untouched(native, shape, dtype):
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
    tdtype = torch.float64 if f64 else torch.float32
    numel, band = b * n * 6 * n, BAND_BYTES // (8 if f64 else 4)
    buf = torch.empty(numel + band, dtype=tdtype, device='cuda')
    obs, behind = buf[:numel].view(b, n, 6 * n), buf[numel:]
    h.bind_buffer(native.BUF_OBS, obs.data_ptr(), numel * obs.element_size())
    bits = lambda x: x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)      # exact, and NaN compares equal to itself
    sentinel = 0x5A5A5A5A5A5A5A5A if f64 else 0x5A5A5A5A
    ref = table = None
    for policy in (-1, 1, 0):                                # the planner's choice, nontemporal, plain
        h.set_tuning(native.TUNE_OBS_NONTEMPORAL, policy)
        obs.fill_(float('nan'))
        bits(behind).fill_(sentinel)
        torch.cuda.synchronize()
        sim.step_arrays(raw)
        t = torch.from_numpy(np.ascontiguousarray(sim.fetch(native.BUF_OBS_TABLE))).cuda()
        torch.cuda.synchronize()
        if ref is None:
            table, ref = t, expand_table_torch(t)
            ref = ref.double() if f64 else ref
        assert torch.equal(bits(t), bits(table)), policy     # the same step: the same table
        assert torch.equal(bits(obs), bits(ref)), (policy, torch.nonzero(bits(obs) != bits(ref))[:3].tolist())
        assert bool((bits(behind) == sentinel).all()), policy
    h.set_tuning(native.TUNE_OBS_NONTEMPORAL, -1)
    out = expand_table(table, h)                             # d2d_expand_table: float32, this handle's tuning
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(expand_table_torch(table)))
    h.close()

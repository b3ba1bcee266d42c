"""The step planner (gym_d2d_amd/csrc/d2d_plan.hip) without a GPU: which kernel serves a configuration, in what launch shape and with
which StepArgs geometry.  tests/c/step_plan.cpp drives plan_step, compiled with hipcc as host code; every kernel the table names
must exist in the gfx950 code object of d2d_step.hip / d2d_rollout.hip.  The table holds the BASELINE configurations and the
configurations the GPU tests describe by the kernel that serves them."""
import re

import pytest

from step_plan_util import build_step_plan, kernel_names as _kernel_names, mangled as _mangled

GEOMETRY = ('lpt', 'tpe', 'epw', 'mask_words', 'walk', 'fuse_obs', 'rec_uniform', 'nt_results', 'prefetch_envs', 'obs_expand')

# (id, StepInputs as key=value - unnamed fields keep step_plan.cpp's defaults: one env of one link on one RB, SystemCapacity,
#  inverse square (mode = d2d::PlMode), LinearObs, bucketing on, tuning on auto, 256 CUs -, kernel, grid, block, dynamic LDS
#  bytes, GEOMETRY)
PLANS = [
    ('config2_traffic_fused', 'B=1024 N=50 R=25 n_fixed=25', 'step_kernel<0,1,false,2,0>', 256, 256, 10432, '1 64 4 2 0 4 0 0 8192 0'),
    ('config3_stress_linear', 'B=4096 N=512 R=256 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,2,2>', 4096, 256, 17600, '2 256 1 0 2 0 1 0 2048 1'),
    ('config4_table', 'B=4096 N=512 R=256 obs_mode=1 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,6,2>', 4096, 256, 17600, '2 256 1 0 2 0 1 1 2048 0'),
    ('learner_obs_none', 'B=4096 N=512 R=256 obs_mode=0 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,6,2>', 4096, 256, 17600, '2 256 1 0 2 0 1 1 2048 0'),
    ('hata_powk_obs_none', 'B=4096 N=512 R=256 mode=4 obs_mode=0 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<4,6,1>', 4096, 512, 19664, '1 512 1 0 2 0 1 1 1024 0'),
    ('hata_powk_linear', 'B=4096 N=512 R=256 mode=4 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<4,2,1>', 4096, 512, 19664, '1 512 1 0 2 0 1 0 1024 1'),
    ('power_law_table', 'B=4096 N=512 R=256 mode=1 obs_mode=1 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<1,6,1>', 4096, 512, 21712, '1 512 1 0 2 0 1 1 1024 0'),
    ('shadowing', 'B=256 N=512 R=256 mode=3 obs_mode=1', 'step_kernel<3,1,true,0,0>', 256, 512, 31888, '1 512 1 16 0 0 0 0 1024 0'),
    ('device_table', 'B=256 N=512 R=256 mode=2 obs_mode=1', 'step_kernel<2,1,true,0,0>', 256, 512, 27792, '1 512 1 16 0 0 0 0 1024 0'),
    ('live_db_table', 'B=256 N=512 R=256 mode=5 obs_mode=1', 'step_kernel<5,1,true,0,0>', 256, 512, 27792, '1 512 1 16 0 0 0 0 1024 0'),
    ('dense_hot1_masks', 'B=4096 N=512 R=64 obs_mode=1 rec_uniform=1', 'step_kernel<0,1,true,1,2>', 4096, 512, 14736, '1 512 1 16 0 0 1 0 1024 0'),
    ('dense_hot1_nt', 'B=4096 N=512 R=64 obs_mode=0 rec_uniform=1 tune_nt=1', 'step_kernel<0,1,true,1,6>', 4096, 512, 14736, '1 512 1 16 0 0 1 1 1024 0'),
    ('dense_hot1_own_link_obs', 'B=37 N=128 R=16 obs_mode=1', 'step_kernel<0,1,false,0,0>', 19, 256, 5952, '1 128 2 4 0 0 0 0 4096 0'),
    ('dense_hot1_prefetch_off', 'B=37 N=128 R=16 obs_mode=1 tune_prefetch=0', 'step_kernel<0,1,false,0,0>', 19, 256, 5952, '1 128 2 4 0 0 0 0 0 0'),
    ('dense_hot1_learner', 'B=41 N=128 R=16 obs_mode=0 rec_uniform=1 rec_uniform128=1', 'step_kernel<0,1,false,0,0>', 21, 256, 5952, '1 128 2 4 0 0 1 0 4096 0'),
    ('dense_learner_prefetch_off', 'B=41 N=128 R=16 obs_mode=0 rec_uniform=1 rec_uniform128=1 tune_prefetch=0', 'step_kernel<0,1,false,0,0>', 21, 256, 5952, '1 128 2 4 0 0 1 0 0 0'),
    ('hot2_traffic_small', 'B=64 N=50 R=25 n_fixed=25', 'step_kernel<0,1,false,2,0>', 16, 256, 10432, '1 64 4 2 0 4 0 0 8192 0'),
    ('hot2_prefetch_off', 'B=64 N=50 R=25 n_fixed=25 tune_prefetch=0', 'step_kernel<0,1,false,0,0>', 16, 256, 10432, '1 64 4 2 0 4 0 0 0 0'),
    ('n2048_two_per_thread', 'B=64 N=2048 R=1024 obs_mode=1', 'step_kernel<0,2,true,0,1>', 64, 1024, 61536, '2 1024 1 0 2 0 0 0 512 0'),
    ('n3000_strided', 'B=16 N=3000 R=1500 obs_mode=1', 'step_kernel<0,0,false,0,0>', 16, 1024, 84080, '0 1024 1 0 0 0 0 0 256 0'),
    ('odd_n_8byte_rows', 'B=1024 N=51 R=25', 'step_kernel<0,1,false,0,0>', 256, 256, 10624, '1 64 4 2 0 2 0 0 8192 0'),
    ('odd_n_unfused', 'B=64 N=257 R=128', 'rollout_kernel<0,8,1>', 64, 320, 8928, '1 320 1 0 2 0 0 0 1536 1'),
    ('obs_f64', 'B=1024 N=50 R=25 obs_f64=1', 'step_kernel<0,1,false,0,0>', 256, 256, 5632, '1 64 4 2 0 0 0 0 8192 1'),
    ('fixed_prefix_rollout', 'B=4096 N=512 R=256 obs_mode=0 n_fixed=256 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,4,1>', 4096, 512, 17600, '1 512 1 0 2 0 0 1 1024 0'),
    ('fixed_set_col_mode1', 'B=4096 N=512 R=256 obs_mode=0 n_fixed=256 col_mode=1 rec_uniform=1', 'step_kernel<0,1,true,0,1>', 4096, 512, 32928, '1 512 1 16 2 0 1 0 1024 0'),
    ('cue_sinr_shannon_rollout', 'B=4096 N=512 R=256 obs_mode=1 reward_fn=3 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,6,1>', 4096, 512, 19664, '1 512 1 0 2 0 1 1 1024 0'),
    ('cue_sinr_shannon_generic', 'B=1024 N=50 R=25 reward_fn=3', 'step_kernel<0,1,false,0,0>', 256, 256, 12032, '1 64 4 2 0 4 0 0 8192 0'),
    ('shannon_rollout', 'B=4096 N=512 R=256 obs_mode=1 reward_fn=2 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,6,2>', 4096, 256, 17600, '2 256 1 0 2 0 1 1 2048 0'),
    ('exact_positions_rollout', 'B=4096 N=512 R=256 obs_mode=0 xpos=1 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,22,1>', 4096, 512, 21712, '1 512 1 0 2 0 1 1 1024 0'),
    ('exact_positions_table', 'B=32 N=128 R=64 mode=4 obs_mode=1 xpos=1', 'rollout_kernel<4,20,1>', 32, 128, 6096, '1 128 1 0 2 0 0 1 4096 0'),
    ('exact_positions_generic', 'B=1024 N=50 R=25 xpos=1', 'step_kernel<0,1,false,0,16>', 256, 256, 12032, '1 64 4 2 0 4 0 0 8192 0'),
    ('padded_rollout', 'B=4096 N=100 R=50 obs_mode=0', 'rollout_kernel<0,12,1>', 4096, 128, 3584, '1 128 1 0 2 0 0 1 4096 0'),
    ('rb_pwr_actions', 'B=4096 N=512 R=256 action_mode=1 obs_mode=1 rec_uniform=1', 'step_kernel<0,1,true,0,0>', 4096, 512, 27792, '1 512 1 16 0 0 1 0 1024 0'),
    ('no_bucketing', 'B=4096 N=512 R=256 bucketing=0 obs_mode=1', 'step_kernel<0,1,true,0,0>', 4096, 512, 10320, '1 512 1 0 0 0 0 0 1024 0'),
    ('tune_walk0', 'B=4096 N=512 R=256 obs_mode=1 tune_walk=0 rec_uniform=1 rec_uniform128=1', 'step_kernel<0,1,true,1,2>', 4096, 512, 27792, '1 512 1 16 0 0 1 0 1024 0'),
    ('tune_prefetch0', 'B=4096 N=512 R=256 obs_mode=1 tune_prefetch=0 rec_uniform=1', 'step_kernel<0,1,true,0,0>', 4096, 512, 27792, '1 512 1 16 0 0 1 0 0 0'),
    ('tune_threads256', 'B=4096 N=512 R=256 obs_mode=1 tune_threads=256', 'step_kernel<0,2,true,0,0>', 4096, 256, 27792, '2 256 1 16 0 0 0 0 1280 0'),
    ('tune_epw2', 'B=4096 N=128 R=64 obs_mode=1 tune_epw=2', 'step_kernel<0,1,false,0,0>', 2048, 256, 7872, '1 128 2 4 0 0 0 0 4096 0'),
    ('tune_block1024', 'B=1024 N=50 R=25 tune_block=1024', 'step_kernel<0,1,false,2,0>', 256, 1024, 10432, '1 64 4 2 0 4 0 0 2048 0'),
    ('tune_lpt1', 'B=4096 N=512 R=256 obs_mode=1 tune_lpt=1 rec_uniform=1 rec_uniform128=1', 'rollout_kernel<0,6,1>', 4096, 512, 17600, '1 512 1 0 2 0 1 1 1024 0'),
    ('tune_lpt2_generic', 'B=4096 N=512 R=256 obs_mode=1 tune_lpt=2 tune_walk=0', 'step_kernel<0,2,true,0,0>', 4096, 256, 27792, '2 256 1 16 0 0 0 0 1280 0'),
    ('tune_fuse0', 'B=1024 N=50 R=25 tune_fuse=0', 'step_kernel<0,1,false,0,0>', 256, 256, 5632, '1 64 4 2 0 0 0 0 8192 1'),
]

# (id, StepInputs, D2D_ERR_* code, d2d_last_error message)
REFUSALS = [
    ('refuse_2_32', 'B=300000 N=1000 R=500', 4, 'envs x links per GPU must stay below 2^32 / 24 (32-bit byte offsets in the step kernel)'),
    ('refuse_lds', 'B=16 N=4096 R=2000 obs_mode=1 mode=1 reward_fn=2', 4, 'links per env exceed the LDS staging capacity'),
    ('refuse_block', 'B=64 N=128 R=64 obs_mode=1 tune_block=1088', 1, 'step workgroup exceeds 1024 threads'),
]


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    return build_step_plan(tmp_path_factory.mktemp('plan'))


def test_plans(plan):
    got = plan([case[1] for case in PLANS])
    assert len(got) == len(PLANS)
    for (name, config, kernel, grid, block, lds, geometry), p in zip(PLANS, got):
        assert (p['kernel'], p['grid'], p['block'], p['lds'], ' '.join(str(p[k]) for k in GEOMETRY)) == (kernel, grid, block, lds, geometry), name
        envs = int(re.search(r'\bB=(\d+)', config).group(1))
        assert p['grid'] == -(-envs // p['epw']) and p['lds'] == p['env_bytes'] * p['epw'], name
        assert p['tpe_magic'] == -(-(1 << 20) // p['tpe']), name


def test_refusals(plan):
    got = plan([case[1] for case in REFUSALS])
    assert [(p.get('error'), p.get('message')) for p in got] == [(code, message) for _, _, code, message in REFUSALS]


def test_every_planned_kernel_is_instantiated(tmp_path):
    (tmp_path / 'step').mkdir()
    (tmp_path / 'rollout').mkdir()
    names = _kernel_names(tmp_path / 'step', 'd2d_step.hip') | _kernel_names(tmp_path / 'rollout', 'd2d_rollout.hip')
    missing = sorted(case[2] for case in PLANS if _mangled(case[2]) not in names)
    assert not missing, missing

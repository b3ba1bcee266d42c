// Launch planner of the step (d2d_plan.hip): which kernel serves a step and in what shape, as a pure function of the
// handle's configuration.  Host code only - no kernels, no HIP runtime calls - so that a CPU test can pin its choices
// (tests/test_step_plan_cpu.py).  run_step (d2d_capi.hip) fills StepInputs, copies the plan into StepArgs and hands the
// kernel identity to launch_step / launch_rollout, which map it to a template instantiation and decide nothing.
#pragma once
#include "d2d_internal.h"

namespace d2d {

// the D2D_TUNE_STEP_* keys (include/d2d_hip.h, d2d_hip_diag.h); -1 / 0 = auto
struct StepTuning {
    int threads = 0;         // threads per env
    int epw = 0;             // envs per workgroup
    int block = 0;           // threads per workgroup
    int fuse = -1;           // fused LinearObs expansion: -1 auto (N <= 128), 0 off, 1 on
    int walk = -1;           // same-RB search (StepArgs::walk)
    int prefetch = -1;       // action prefetch distance in envs: -1 auto, 0 off
    int lpt = -1;            // links per thread: -1 auto, 1, 2
    int nt = -1;             // nontemporal result stores: -1 auto, 0 off, 1 on (if legal)
    int srec = -1;           // scalar record loads: -1 auto, 0 off, 1 on (if legal)
    int obs_rotate = -1;     // fused expansion start-phase multiplier: -1 auto (29), 0 off
    int ablate = 0;          // diagnostic builds only
};

// the D2D_TUNE_OBS_* keys: the LinearObs expansion kernel's shape
struct ObsTuning {
    int rows = 0, nt = -1, xcd = 1, block = 0, variant = 0, stagger = 0;       // nt: the store policy of store16, -1 = plan_obs chooses
};

// everything the choice of the step kernel reads, as plain values
struct StepInputs {
    int B, N, R, num_cus;
    int action_mode;         // 0: raw actions (d2d_step)   1: explicit rb / pwr (d2d_step_rb_pwr, d2d_step_host)
    int n_fixed, col_mode, reward_fn;
    PlMode mode;
    int obs_mode, obs_f64, bucketing;
    int rec_uniform, rec_uniform128;   // the handle's record uniformity within aligned groups of 64 / 128 links (refresh_tables)
    int xpos;                          // float64 positions with a non-zero low part somewhere: the OPT_XPOS kernels
    StepTuning tune;
};

// The kernel of one step: step_kernel<mode, lpt, full, hot, opt> (d2d_step.hip) or, with rollout set,
// rollout_kernel<mode, opt, lpt> (d2d_rollout.hip).
struct StepKernel {
    int rollout;
    int mode, lpt, full, hot, opt;
};

struct StepPlan {
    // the geometry fields of StepArgs
    int lpt, tpe;
    unsigned tpe_magic;
    int epw, mask_words, walk, fuse_obs, obs_rotate;
    unsigned obs_q_per_row;
    unsigned long long obs_q_magic;
    StepLds lds;
    int rollout, rec_uniform, nt_results, prefetch_envs;
    // the launch
    unsigned grid;
    int block;
    size_t lds_bytes;        // dynamic LDS per workgroup
    StepKernel kernel;
    int obs_expand;          // the LinearObs expansion runs as a launch of its own behind the step
};

// D2D_OK, or a D2D_ERR_* code with *error set to the message for d2d_last_error
int plan_step(const StepInputs& in, StepPlan* out, const char** error);
// LinearObs expansion geometry for a [B, N, 6] table (ObsArgs::table / obs left null)
ObsArgs plan_obs(const ObsTuning& t, int B, int N, int out_f64);

}  // namespace d2d

/* Driver of the step planner (gym_d2d_amd/csrc/d2d_plan.hip) for tests/test_step_plan_cpu.py: host code only, no GPU needed.
 * Every argument is one configuration, "key=value key=value ..." over the fields of StepInputs (tuning keys as tune_<field>);
 * fields left out keep the defaults below.  One JSON line per configuration: the plan, or the refusal's code and message. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "../../gym_d2d_amd/csrc/d2d_plan.h"
#include "d2d_hip.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        d2d::StepInputs in{};
        in.B = 1; in.N = 1; in.R = 1; in.num_cus = 256;
        in.reward_fn = D2D_REWARD_SYSTEM_CAPACITY; in.mode = d2d::PL_INV_SQUARE; in.obs_mode = D2D_OBS_LINEAR; in.bucketing = 1;
        std::istringstream words(argv[a]);
        std::string w;
        while (words >> w) {
            const size_t eq = w.find('=');
            const std::string key = w.substr(0, eq);
            const int v = std::atoi(w.c_str() + eq + 1);
            struct { const char* name; int* field; } fields[] = {
                {"B", &in.B}, {"N", &in.N}, {"R", &in.R}, {"num_cus", &in.num_cus}, {"action_mode", &in.action_mode},
                {"n_fixed", &in.n_fixed}, {"col_mode", &in.col_mode}, {"reward_fn", &in.reward_fn}, {"obs_mode", &in.obs_mode},
                {"obs_f64", &in.obs_f64}, {"bucketing", &in.bucketing}, {"rec_uniform", &in.rec_uniform},
                {"rec_uniform128", &in.rec_uniform128}, {"xpos", &in.xpos}, {"tune_threads", &in.tune.threads},
                {"tune_epw", &in.tune.epw}, {"tune_block", &in.tune.block}, {"tune_fuse", &in.tune.fuse}, {"tune_walk", &in.tune.walk},
                {"tune_prefetch", &in.tune.prefetch}, {"tune_lpt", &in.tune.lpt}, {"tune_nt", &in.tune.nt}, {"tune_srec", &in.tune.srec},
                {"tune_obs_rotate", &in.tune.obs_rotate}, {"tune_ablate", &in.tune.ablate}};
            bool known = key == "mode";
            if (known) in.mode = (d2d::PlMode)v;
            for (auto& f : fields) if (key == f.name) { *f.field = v; known = true; }
            if (!known) { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        d2d::StepPlan p;
        const char* why = "";
        const int rc = d2d::plan_step(in, &p, &why);
        if (rc) { std::printf("{\"error\": %d, \"message\": \"%s\"}\n", rc, why); continue; }
        const d2d::StepKernel& k = p.kernel;
        char kernel[64];
        if (k.rollout) std::snprintf(kernel, sizeof(kernel), "rollout_kernel<%d,%d,%d>", k.mode, k.opt, k.lpt);
        else std::snprintf(kernel, sizeof(kernel), "step_kernel<%d,%d,%s,%d,%d>", k.mode, k.lpt, k.full ? "true" : "false", k.hot, k.opt);
        std::printf("{\"kernel\": \"%s\", \"grid\": %u, \"block\": %d, \"lds\": %zu, \"obs_expand\": %d, \"lpt\": %d, \"tpe\": %d, "
                    "\"tpe_magic\": %u, \"epw\": %d, \"mask_words\": %d, \"walk\": %d, \"fuse_obs\": %d, \"obs_rotate\": %d, "
                    "\"obs_q_per_row\": %u, \"obs_q_magic\": %llu, \"rollout\": %d, \"rec_uniform\": %d, \"nt_results\": %d, "
                    "\"prefetch_envs\": %d, \"env_bytes\": %u}\n",
                    kernel, p.grid, p.block, p.lds_bytes, p.obs_expand, p.lpt, p.tpe, p.tpe_magic, p.epw, p.mask_words, p.walk, p.fuse_obs,
                    p.obs_rotate, p.obs_q_per_row, p.obs_q_magic, p.rollout, p.rec_uniform, p.nt_results, p.prefetch_envs, p.lds.env_bytes);
    }
    return 0;
}

/* Driver of the LinearObs expansion planner (plan_obs, gym_d2d_amd/csrc/d2d_plan.hip) for tests/test_obs_plan_cpu.py: host code only,
 * the twin of step_plan.cpp.  Every argument is one configuration, "key=value ..." over B, N, f64 and the fields of ObsTuning
 * (tune_<field>); fields left out keep their defaults.  One JSON line per configuration: the launch shape plan_obs chose. */
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>

#include "../../gym_d2d_amd/csrc/d2d_plan.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        int B = 1, N = 2, f64 = 0;
        d2d::ObsTuning t;
        std::istringstream words(argv[a]);
        std::string w;
        while (words >> w) {
            const size_t eq = w.find('=');
            const std::string key = w.substr(0, eq);
            const int v = std::atoi(w.c_str() + eq + 1);
            struct { const char* name; int* field; } fields[] = {
                {"B", &B}, {"N", &N}, {"f64", &f64}, {"tune_rows", &t.rows}, {"tune_nt", &t.nt}, {"tune_xcd", &t.xcd},
                {"tune_block", &t.block}, {"tune_variant", &t.variant}, {"tune_stagger", &t.stagger}};
            bool known = false;
            for (auto& f : fields) if (key == f.name) { *f.field = v; known = true; }
            if (!known) { std::fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
        }
        const d2d::ObsArgs o = d2d::plan_obs(t, B, N, f64);
        std::printf("{\"block\": %d, \"pieces\": %d, \"chunks\": %d, \"policy\": %d, \"vec\": %d, \"variant\": %d, \"xcd_remap\": %d, "
                    "\"q_per_row\": %u, \"out_f64\": %d, \"chunk_magic\": %llu}\n",
                    o.block, o.rows_per_wg, o.chunks, o.nontemporal, o.vec, o.variant, o.xcd_remap, o.q_per_row, o.out_f64, o.chunk_magic);
    }
    return 0;
}

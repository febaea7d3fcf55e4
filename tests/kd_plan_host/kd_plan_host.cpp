// kd_plan_host.cpp -- TEST INFRASTRUCTURE: the k-d level tables of a launch plan and the level from which a re-sort
// finishes in one kernel (LaunchPlan::kd_finish_from), as plan_engine decides them from n and the LJMD_* knobs of the
// environment.  usage: kd_plan_host N...  -> one JSON object per line.  Host code only: no device is touched.
#include "ljmd_engine.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int k = 1; k < argc; ++k) {
        const int n = std::atoi(argv[k]);
        const double L = std::cbrt(n / 0.8);
        const SimParams sim = ljmdh::derive_params(n, L, 0.005, 0.49 * L);
        ljmdh::LaunchPlan p;
        if (ljmdh::plan_engine(sim, n, 1, LJMD_PRECISION_FP64, ljmdh::read_knobs(), &p) != LJMD_OK) return 1;
        std::printf("{\"n\": %d, \"S\": %d, \"P\": %d, \"cap\": %d, \"max_levels\": %d, \"kd_finish_from\": %d, \"levels\": [", n, p.S,
                    p.P, kKdFinishCap, kKdFinishMaxLevels, p.kd_finish_from);
        for (size_t l = 0; l < p.kd_level_nseg.size(); ++l) {
            std::printf("%s[", l ? ", " : "");
            for (int j = 0; j <= p.kd_level_nseg[l]; ++j) std::printf("%s%d", j ? ", " : "", p.kd_offsets[p.kd_level_off[l] + j]);
            std::printf("]");
        }
        std::printf("]}\n");
    }
    return 0;
}

// select_shim.cpp — TEST-ONLY C entry to the step-kernel selector
// (multi-agent-rl-for-fjsp_amd/csrc/fjsp_select.h) for tests/test_step_select.py.
#define FJSP_DEV inline
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_select.h"
using namespace fjsp;

// opts: fused_lds, pipeline, predraw, agents, ag_envs, step_envs, test_stall
// plan: family, lds, full, nemit, predraw, epw, stall, grid, waves; returns the name
extern "C" const char* sel_step_many(int n, int K, int mode, int autoreset, int full, const int* opts, int* plan) {
    const StepOpts o{opts[0], opts[1], opts[2], opts[3], opts[4], opts[5], opts[6]};
    const StepPlan p = select_step_many(n, K, mode, autoreset, full != 0, o);
    const int v[9] = {p.kernel.family, p.kernel.lds, p.kernel.full, p.kernel.nemit, p.kernel.predraw,
                      p.epw, p.stall, p.grid, p.waves};
    for (int i = 0; i < 9; i++) plan[i] = v[i];
    return p.kernel.name;
}

// fjsp_select.h — which step kernel a launch gets: host-only, no HIP types, so the rules are
// tested on the CPU (tests/test_step_select.py compiles this header with g++).
//
// STEP_KERNELS is the one table of fjsp_step_many's kernels: a row's name is what
// fjsp_last_kernel reports (bench.py's benchmark line, the path-pinning GPU tests) and its
// index (StepPlan::variant) is what the launch switches on, so the two cannot drift apart.  A
// new variant is one enumerator, one row, one rule in select_step_many and one case in
// fjsp_step_many.
#pragma once
#include "fjsp_env.h"
#include "../../include/fjsp.h"

namespace fjsp {

// per-handle knobs (fjsp_set_option; defaults in fjsp_create): every variant writes the same bytes
struct StepOpts {
    int fused_lds;    // order table + tray-slot arena in LDS: -1 = auto, 0 / 1
    int pipeline;     // the multi-wave k_step_pipe for lean outputs
    int predraw;      // pre-draw wave in the pipelined kernels
    int agents;       // agent-group pipeline k_step_ag for uniform-random actions
    int ag_envs;      // k_step_ag envs per workgroup: 64 / 32 / 16, 0 = auto
    int step_envs;    // k_step envs per workgroup: 64 / 32 / 16, 0 = 64
    int test_stall;   // tests: launch k_step_ag's STALL build
};

enum StepFamily : int { STEP_MANY, STEP_PIPE, STEP_AG };

enum StepVariant : int {
    SV_MANY, SV_MANY_LDS, SV_MANY_FULL, SV_MANY_LDS_FULL,
    SV_PIPE_1EMIT, SV_PIPE_2EMIT, SV_PIPE_LDS_1EMIT, SV_PIPE_LDS_2EMIT, SV_PIPE_LDS_2EMIT_PREDRAW,
    SV_AG
};
constexpr int SV_COUNT = SV_AG + 1;   // not an enumerator: the launch switch names every variant, no default

// one kernel of fjsp_step_many: its reported name, its family and the family's template arguments
struct StepKernel {
    const char* name;
    StepFamily family;
    bool lds, full;   // k_step_many<LDS, FULL>, k_step_pipe<LDS, ..>
    int nemit;        // k_step_pipe<.., NEMIT, ..>
    bool predraw;     // k_step_pipe<.., PG>
    bool has_stall;   // a STALL (test_stall) build exists: k_step_ag only, the one kernel with bounded waits
};

constexpr StepKernel STEP_KERNELS[SV_COUNT] = {
    /* SV_MANY */                   {"k_step_many", STEP_MANY, false, false, 0, false, false},
    /* SV_MANY_LDS */               {"k_step_many<lds>", STEP_MANY, true, false, 0, false, false},
    /* SV_MANY_FULL */              {"k_step_many<full>", STEP_MANY, false, true, 0, false, false},
    /* SV_MANY_LDS_FULL */          {"k_step_many<lds,full>", STEP_MANY, true, true, 0, false, false},
    /* SV_PIPE_1EMIT */             {"k_step_pipe<1emit>", STEP_PIPE, false, false, 1, false, false},
    /* SV_PIPE_2EMIT */             {"k_step_pipe<2emit>", STEP_PIPE, false, false, 2, false, false},
    /* SV_PIPE_LDS_1EMIT */         {"k_step_pipe<lds,1emit>", STEP_PIPE, true, false, 1, false, false},
    /* SV_PIPE_LDS_2EMIT */         {"k_step_pipe<lds,2emit>", STEP_PIPE, true, false, 2, false, false},
    /* SV_PIPE_LDS_2EMIT_PREDRAW */ {"k_step_pipe<lds,2emit,predraw>", STEP_PIPE, true, false, 2, true, false},
    // k_step_ag<EPW>: fixed roles (four emit waves, pre-draw); every EPW reports the one name
    /* SV_AG */                  {"k_step_ag<lds,predraw>", STEP_AG, true, false, 4, true, true},
};

constexpr int AG_WAVES = 8;    // k_step_ag's roles: AM, P, K, PD and the four emit waves
constexpr int NUM_CUS = 256;   // MI355X

struct StepPlan {
    StepVariant variant;   // row of STEP_KERNELS: the name and the instantiation
    StepKernel kernel;     // = STEP_KERNELS[variant]
    int epw;               // envs per workgroup (k_step_ag<EPW>, k_step<.., EPW>; BLOCK elsewhere)
    bool stall;            // launch the kernel's STALL build
    int grid, waves;       // workgroups, wavefronts per workgroup
};

inline StepPlan step_plan(StepVariant v, int n, int epw, const StepOpts& o) {
    const StepKernel k = STEP_KERNELS[v];
    const int waves = k.family == STEP_AG ? AG_WAVES : k.family == STEP_PIPE ? 1 + k.nemit + k.predraw : 1;
    return StepPlan{v, k, epw, o.test_stall && k.has_stall, (n + epw - 1) / epw, waves};
}

// fjsp_step_many's kernel for n envs x K steps (K > 0); full_outputs: any output beyond the lean
// set (obs, masks, rewards, term, trunc, status) is asked for
inline StepPlan select_step_many(int n, int K, int action_mode, int autoreset, bool full_outputs, const StepOpts& o) {
    // LDS tables (97.5 KB per 64-env workgroup) pay while every workgroup has a CU of its own
    const bool lds = o.fused_lds < 0 ? n <= NUM_CUS * BLOCK : o.fused_lds != 0;
    // a second emit wave pays while the CUs are not full (N <= 16384 at 64 envs per CU)
    const bool two_emit = n <= NUM_CUS * BLOCK;
    // the pre-draw wave pays while the CUs have a free SIMD (and only with auto-reset)
    const bool pg = o.predraw && lds && two_emit && autoreset;
    // the multi-wave kernels write the lean outputs only
    const bool pipe = o.pipeline && !full_outputs;
    // the agent-group pipeline: state-independent (uniform-random) actions, LDS tables, pre-draw;
    // also for 16 384 < N <= 32 768, where its 64-env workgroups run in two rounds and still beat
    // k_step_pipe<1emit> (24 576 envs 3.17 against 3.75, 32 768 3.20-3.59 against 3.87 ms per
    // 1 024-step launch; 49 152: 4.85 against 4.37-4.72; profiles/r04/ag_two_rounds_ab.json)
    const bool ag_wide = n > NUM_CUS * BLOCK && n <= 2 * NUM_CUS * BLOCK && o.fused_lds != 0 && o.predraw && autoreset;
    if (o.agents && pipe && (pg || ag_wide) && action_mode == FJSP_ACTIONS_UNMASKED) {
        // envs per workgroup: auto = the fewest that still give every workgroup a CU of its own
        // for long launches (1.30 -> 1.22 us per step at 4 096 envs); 64 for launches of fewer
        // than 64 steps, whose time is mostly the per-workgroup fixed cost (K = 20: 36.6 against
        // 39.9 us in rocprof)
        int epw = o.ag_envs;
        if (epw == 0) epw = K < 64 ? 64 : n <= NUM_CUS * 16 ? 16 : n <= NUM_CUS * 32 ? 32 : 64;
        return step_plan(SV_AG, n, epw, o);
    }
    StepVariant v;
    if (pipe) {
        v = pg         ? SV_PIPE_LDS_2EMIT_PREDRAW
            : lds      ? (two_emit ? SV_PIPE_LDS_2EMIT : SV_PIPE_LDS_1EMIT)
            : two_emit ? SV_PIPE_2EMIT
                       : SV_PIPE_1EMIT;
    } else if (full_outputs) {
        v = lds ? SV_MANY_LDS_FULL : SV_MANY_FULL;
    } else {
        v = lds ? SV_MANY_LDS : SV_MANY;
    }
    return step_plan(v, n, BLOCK, o);
}

// fjsp_step's kernel k_step<CANON, EPW>: the agents in canonical order or in a caller-given one
struct KStepPlan {
    const char* name;
    bool canon;
    int epw, grid;
};

inline KStepPlan select_step(int n, bool canon, const StepOpts& o) {
    // 64 envs per workgroup unless the option says otherwise: at 4 096 envs 16- / 32-env
    // workgroups (all 256 CUs busy) measured slower, 8.58 / 8.32 against 7.61 us per launch
    // (profiles/r06/kstep/ab_step_envs_4096.json): the step is not bound by its lanes' branch union
    const int epw = o.step_envs ? o.step_envs : 64;
    return KStepPlan{canon ? "k_step<canon>" : "k_step<ordered>", canon, epw, (n + epw - 1) / epw};
}

}  // namespace fjsp

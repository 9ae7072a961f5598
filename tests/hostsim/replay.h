// replay.h — TEST-ONLY: the replay loop of the wave shims.  `envs` envs x `steps` steps of
// uniform-random actions with auto-reset; world R takes the plain step (env_step<true>), world S
// the step as one wave of k_step_ag schedules it, which the shim's model supplies; every env-step
// is compared.  README.md has the contract.
#pragma once
#include "world.h"

// what the loop hands the model at each env-step
struct Step {
    int env, k, steps, num_orders;
    const int* act;            // this step's actions
    const int* nxt;            // the next step's and the one's after it, where the model
    const int* nx2;            // asked for them (AHEAD); else null
    const World& R0;           // R before the plain step
    const World& R;            // and after it
    const uint32_t* res_ref;   // R's result words
    int dead_slot;             // the model may name one more slot whose link same_live skips
};

struct Replayed {
    int64_t compared, resets;
};

// A model is a struct with
//   static constexpr int AHEAD     how many steps' actions are drawn ahead of the step that runs (0..2)
//   void begin(World& S)           a new env, both worlds freshly reset
//   bool step(Step& st, World& S)  S's step; false if something the wave checks beyond same_live differs
//   void end_step(const Step& st, World& S, bool done, Mismatch& bad)
//                                  after the step counters moved on and, if done, both worlds were reset:
//                                  what the wave does between two steps, its own counters, its own reset
// The action stream of env e is seeded seed * 1000003 + e and the order tables' seed + 77 * e; S's
// tables continue a copy of R's stream.
template <class Model>
Replayed replay(const Cfg& C, int envs, int steps, int num_orders, uint64_t seed, Model& m, Mismatch& bad, const char* what) {
    Replayed n{0, 0};
    for (int e = 0; e < envs; e++) {
        Lcg ga{seed * 1000003ull + (uint64_t)e}, gr{seed + 77ull * (uint64_t)e}, gs = gr;
        World R, S;
        memset(&R, 0, sizeof(R));
        memset(&S, 0, sizeof(S));
        reset_world(R, C, num_orders, gr);
        reset_world(S, C, num_orders, gs);
        Tables TR = R.tabs();
        int act[3][NA];
        for (int i = 1; i <= Model::AHEAD; i++) draw_actions(ga, act[i]);
        m.begin(S);
        for (int k = 0; k < steps; k++) {
            for (int i = 0; i < Model::AHEAD; i++) memcpy(act[i], act[i + 1], sizeof(act[i]));
            draw_actions(ga, act[Model::AHEAD]);
            const World R0 = R;
            uint32_t res_ref[NA];
            double rew[NA];
            env_step<true>(R.E, TR, C, act[0], nullptr, res_ref, rew);
            Step st{e, k, steps, num_orders, act[0], Model::AHEAD >= 1 ? act[1] : nullptr, Model::AHEAD >= 2 ? act[2] : nullptr,
                    R0, R, res_ref, NIL};
            const bool ok = m.step(st, S) && same_live(R, S, num_orders, st.dead_slot);
            n.compared++;
            bad.check(ok, "env %d step %d (orders %d): %s", e, k, num_orders, what);
            // end of step: auto-reset (the next table continues each side's own stream)
            const bool done = episode_over(R.E, C);
            R.E.set_step(R.E.step() + 1);
            S.E.set_step(S.E.step() + 1);
            if (done) {
                const int nord = R.E.norders();
                reset_world(R, C, nord, gr);
                reset_world(S, C, nord, gs);
                n.resets++;
            }
            m.end_step(st, S, done, bad);
        }
    }
    return n;
}

// pack_shim.cpp — TEST-ONLY host build of fjsp_env.h's pack_words (the pack words of
// fjsp_step_sched) for tests/test_pack_host.py: replays of the reference's recorded runs (actions,
// order tables and configs from tests/golden/packaging.npz).
#include "world.h"

extern "C" {

// One recorded run: actions u8 [T][8], the recorded result words u32 [T][8] and flags u8 [T], the
// order tables u8 [episodes][num_orders][3] of its episodes in order; cfg = pt_packaging,
// max_episode_steps, packaging capacity.  pack u32 [T][4] receives the pack words of the state after
// each step and before the reset, packaged i32 [T] the state's total.  out: [0] steps whose result
// words differ from the recording, [1] steps whose term / trunc differ, [2] resets, [3] states that
// pack_words changed, [4] status bits ORed over the run.
void pack_replay(const uint8_t* actions, const uint32_t* results, const uint8_t* term, const uint8_t* trunc,
                 const uint8_t* orders, int episodes, int num_orders, int T, const int32_t* cfg, uint32_t* pack,
                 int32_t* packaged, int64_t* out) {
    Cfg C = default_cfg();
    C.ptk_pack = cfg[0] / 10; C.max_steps = cfg[1]; C.pkg_cap = cfg[2];
    for (int i = 0; i < 5; i++) out[i] = 0;
    World W;
    memset(&W, 0, sizeof(W));
    int ep = 0;
    reset_world(W, C, num_orders, orders);
    Tables Tb = W.tabs();
    for (int t = 0; t < T; t++) {
        int act[NA];
        for (int a = 0; a < NA; a++) act[a] = actions[t * NA + a];
        uint32_t res[NA];
        double rew[NA];
        env_step<true>(W.E, Tb, C, act, nullptr, res, rew);
        bool same = true;
        for (int a = 0; a < NA; a++) same = same && res[a] == results[t * NA + a];
        out[0] += !same;
        const Env before = W.E;
        pack_words(W.E, pack + 4 * t);
        out[3] += memcmp(before.w, W.E.w, sizeof(W.E.w)) != 0;
        packaged[t] = W.E.total_packaged();
        out[4] |= W.E.status();
        const int nord = W.E.norders();
        const bool te = all_done(W.E), tr = W.E.step() >= C.max_steps;
        out[1] += (te != (term[t] != 0)) || (tr != (trunc[t] != 0));
        W.E.set_step(W.E.step() + 1);
        if (te || tr) {
            ep++;
            if (ep >= episodes) { out[1] += 1000000; return; }
            reset_world(W, C, nord, orders + (size_t)ep * num_orders * 3);
            out[2]++;
        }
    }
}

}  // extern "C"

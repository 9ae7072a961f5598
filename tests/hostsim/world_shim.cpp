// world_shim.cpp — TEST-ONLY entry to world.h's comparers for tests/test_hostsim_world.py: two equal
// worlds in the middle of an episode, one flip at a time in a copy of the second.
#include "world.h"

namespace {
World R, S;
int norders;
}  // namespace

extern "C" {

// Random steps on both worlds until the AGV carries a tray and slots beyond it are in use (at most
// max_steps).  info: steps taken (-1: no such state), slot_next, the carried slot.
void world_prepare(int num_orders, uint64_t seed, int max_steps, int32_t* info) {
    const Cfg C = default_cfg();
    Lcg ga{seed}, gr{seed + 1}, gs = gr;
    memset(&R, 0, sizeof(R));
    memset(&S, 0, sizeof(S));
    reset_world(R, C, num_orders, gr);
    reset_world(S, C, num_orders, gs);
    norders = num_orders;
    Tables TR = R.tabs(), TS = S.tabs();
    info[0] = -1;
    for (int k = 0; k < max_steps && info[0] < 0 && !episode_over(R.E, C); k++) {
        int act[NA];
        uint32_t res[NA];
        double rew[NA];
        draw_actions(ga, act);
        env_step<true>(R.E, TR, C, act, nullptr, res, rew);
        env_step<true>(S.E, TS, C, act, nullptr, res, rew);
        R.E.set_step(R.E.step() + 1);
        S.E.set_step(S.E.step() + 1);
        if (R.E.carry() != NIL && R.E.slot_next() >= R.E.carry() + 3) info[0] = k + 1;
    }
    info[1] = R.E.slot_next();
    info[2] = R.E.carry();
}

// One bit flipped in a copy of S: table 0 state words, 1 orders, 2 scode, 3 snext, 4 scstep (< 0: no
// flip), element index.  verdict: same_live(R, copy, num_orders, dead_slot), same_world(R, copy).
void world_flip(int table, int index, int dead_slot, int32_t* verdict) {
    World T = S;
    if (table == 0) T.E.w[index] ^= 1u;
    if (table == 1) T.orders[index] ^= 1u;
    if (table == 2) T.scode[index] ^= 1u;
    if (table == 3) T.snext[index] ^= 1u;
    if (table == 4) T.scstep[index] ^= 1u;
    verdict[0] = same_live(R, T, norders, dead_slot);
    verdict[1] = same_world(R, T);
}

}  // extern "C"

// search_shim.cpp — TEST-ONLY host build of fjsp_search.h (the perturbed heuristic and the lane loop
// of k_search_rollout) with the state machine of fjsp_env.h, for tests/test_search_host.py: the
// policy and the lane loop against the oracle, on worlds the caller holds as bytes.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define FJSP_DEV inline
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_orders.h"
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_search.h"
using namespace fjsp;

namespace {

struct World {   // one env with its tables (stride 1)
    Env E;
    uint32_t pgw;
    uint32_t orders[MAX_ORDERS];
    uint16_t scode[MAX_SLOTS];
    uint8_t snext[MAX_SLOTS];
    uint16_t scstep[MAX_SLOTS];
    Tables tabs() { return Tables{orders, scode, snext, scstep, 1}; }
};

const double* reward_lut() {   // the default weights
    static double lut[RLUT_SIZE];
    static bool built = false;
    if (!built) {
        const double w[NW] = {100.0, 10.0, -0.1, 1.0, 5.0, -1.0, 2.0, -0.1, 10.0, -5.0, 5.0, 1.0, -2.0, 20.0, 2.0, -1.0};
        build_reward_lut(w, 10, lut);
        built = true;
    }
    return lut;
}

Cfg make_cfg() {   // the default config
    Cfg C;
    C.step_size = 10; C.max_steps = 200; C.tray_cap = 5; C.mask_tray_cap = 5; C.storage_cap = 100;
    C.pool0 = 1000; C.pkg_cap = 20; C.ptk_small = 6; C.ptk_big = 12; C.ptk_pack = 3;
    C.lut = reward_lut();
    return C;
}

}  // namespace

extern "C" {

int search_world_bytes(void) { return (int)sizeof(World); }

// a reset with the caller's book (K order words n | type << 4 | colour << 6); 1 = accepted
int search_world_reset(void* world, const uint32_t* book, int K) {
    World& W = *(World*)world;
    memset(&W, 0, sizeof(W));
    const Cfg C = make_cfg();
    Tables Tb = W.tabs();
    return put_orders_env(W.E, Tb, C, book, 1, K, K, 0, &W.pgw) ? 1 : 0;
}

// the three policies on the world's current state (no state change)
void search_eps_actions(void* world, uint64_t seed, uint32_t gid, uint32_t step, int eps8, uint8_t* out) {
    World& W = *(World*)world;
    const Cfg C = make_cfg();
    int act[NA];
    eps_heuristic_actions(seed, gid, step, eps8, W.E, W.tabs(), C, act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}
void search_heuristic(void* world, uint8_t* out) {
    World& W = *(World*)world;
    int act[NA];
    heuristic_actions(W.E, W.tabs(), act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}
void search_masked(void* world, uint64_t seed, uint32_t gid, uint32_t step, uint8_t* out) {
    World& W = *(World*)world;
    const Cfg C = make_cfg();
    int act[NA];
    masked_actions(action_word(seed, gid, step), W.E, C, act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}

// one step without auto-reset; info: term, trunc, orders_completed, packaged; returns sim_time
double search_step(void* world, const uint8_t* actions, int32_t* info) {
    World& W = *(World*)world;
    const Cfg C = make_cfg();
    int act[NA];
    uint32_t res[NA];
    double rew[NA];
    for (int a = 0; a < NA; a++) act[a] = actions[a];
    env_step<true>(W.E, W.tabs(), C, act, nullptr, res, rew);
    flag_obs_overflow(W.E);
    const int nord = W.E.norders();
    info[0] = W.E.ncompleted() == nord && nord > 0 && W.E.next_order() == nord;
    info[1] = W.E.step() >= C.max_steps;
    info[2] = W.E.ncompleted();
    info[3] = W.E.total_packaged();
    const double t = (double)(W.E.step() + 1) * (double)C.step_size;
    W.E.set_step(W.E.step() + 1);
    return t;
}

// what fjsp_search_rollout does over n worlds (lane e = worlds + e * sizeof(World)), the arrays laid
// out as the entry's: script u8 [L][8][n] or null, script_len i32 [n] or null, active u8 [n] or
// null, trace u8 [K][8][n], the end arrays [n]
void search_rollout_host(void* worlds, int n, int K, int eps8, uint64_t seed, uint32_t gid0, uint32_t step_base, int t0,
                         const uint8_t* script, int L, const int32_t* script_len, const uint8_t* active, uint8_t* trace,
                         int32_t* steps, uint8_t* flags, int32_t* orders_completed, int32_t* packaged, double* sim_time) {
    const Cfg C = make_cfg();
    for (int e = 0; e < n; e++) {
        if (active && !active[e]) {
            steps[e] = -1;
            continue;
        }
        World& W = ((World*)worlds)[e];
        int slen = 0;
        if (script) {
            slen = script_len ? script_len[e] : L;
            slen = slen < 0 ? 0 : slen > L ? L : slen;
        }
        const LaneEnd r = search_lane(W.E, W.tabs(), C, K, eps8, seed, gid0 + (uint32_t)e, step_base + (uint32_t)t0,
                                      script ? script + e : nullptr, slen, trace + e, (size_t)n);
        steps[e] = r.steps;
        flags[e] = (uint8_t)r.flags;
        orders_completed[e] = r.orders_completed;
        packaged[e] = r.packaged;
        sim_time[e] = r.sim_time;
    }
}

uint32_t search_world_status(void* world) { return ((World*)world)->E.status(); }

}  // extern "C"

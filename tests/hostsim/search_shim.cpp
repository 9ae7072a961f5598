// search_shim.cpp — TEST-ONLY host build of fjsp_search.h (the perturbed heuristic and the lane loop
// of k_search_rollout) with the state machine of fjsp_env.h, for tests/test_search_host.py: the
// policy and the lane loop against the oracle, on worlds the caller holds as bytes.
#include "world.h"

#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_orders.h"
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_search.h"

extern "C" {

int search_world_bytes(void) { return (int)sizeof(BookWorld); }

// a reset with the caller's book (K order words n | type << 4 | colour << 6); 1 = accepted
int search_world_reset(void* world, const uint32_t* book, int K) {
    BookWorld& W = *(BookWorld*)world;
    memset(&W, 0, sizeof(W));
    const Cfg C = default_cfg();
    Tables Tb = W.tabs();
    return put_orders_env(W.E, Tb, C, book, 1, K, K, 0, &W.pgw) ? 1 : 0;
}

// the three policies on the world's current state (no state change)
void search_eps_actions(void* world, uint64_t seed, uint32_t gid, uint32_t step, int eps8, uint8_t* out) {
    BookWorld& W = *(BookWorld*)world;
    const Cfg C = default_cfg();
    int act[NA];
    eps_heuristic_actions(seed, gid, step, eps8, W.E, W.tabs(), C, act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}
void search_heuristic(void* world, uint8_t* out) {
    BookWorld& W = *(BookWorld*)world;
    int act[NA];
    heuristic_actions(W.E, W.tabs(), act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}
void search_masked(void* world, uint64_t seed, uint32_t gid, uint32_t step, uint8_t* out) {
    BookWorld& W = *(BookWorld*)world;
    const Cfg C = default_cfg();
    int act[NA];
    masked_actions(action_word(seed, gid, step), W.E, C, act);
    for (int a = 0; a < NA; a++) out[a] = (uint8_t)act[a];
}

// one step without auto-reset; info: term, trunc, orders_completed, packaged; returns sim_time
double search_step(void* world, const uint8_t* actions, int32_t* info) {
    BookWorld& W = *(BookWorld*)world;
    const Cfg C = default_cfg();
    int act[NA];
    uint32_t res[NA];
    double rew[NA];
    for (int a = 0; a < NA; a++) act[a] = actions[a];
    env_step<true>(W.E, W.tabs(), C, act, nullptr, res, rew);
    flag_obs_overflow(W.E);
    info[0] = all_done(W.E);
    info[1] = W.E.step() >= C.max_steps;
    info[2] = W.E.ncompleted();
    info[3] = W.E.total_packaged();
    const double t = (double)(W.E.step() + 1) * (double)C.step_size;
    W.E.set_step(W.E.step() + 1);
    return t;
}

// what fjsp_search_rollout does over n worlds (lane e = worlds + e * sizeof(BookWorld)), the arrays
// laid out as the entry's: script u8 [L][8][n] or null, script_len i32 [n] or null, active u8 [n] or
// null, trace u8 [K][8][n], the end arrays [n]
void search_rollout_host(void* worlds, int n, int K, int eps8, uint64_t seed, uint32_t gid0, uint32_t step_base, int t0,
                         const uint8_t* script, int L, const int32_t* script_len, const uint8_t* active, uint8_t* trace,
                         int32_t* steps, uint8_t* flags, int32_t* orders_completed, int32_t* packaged, double* sim_time) {
    const Cfg C = default_cfg();
    for (int e = 0; e < n; e++) {
        if (active && !active[e]) {
            steps[e] = -1;
            continue;
        }
        BookWorld& W = ((BookWorld*)worlds)[e];
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

uint32_t search_world_status(void* world) { return ((BookWorld*)world)->E.status(); }

}  // extern "C"

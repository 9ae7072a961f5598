// fjsp_search.h — what the rollout search over order books runs per env (search.py, fjsp_actions_eps,
// fjsp_search_rollout): the counter RNG of the synthetic actions, the masked-uniform draw, the
// perturbed heuristic and the lane loop of k_search_rollout, written so that the same source
// compiles for the device (fjsp_hip.hip) and for the host (tests/hostsim/search_shim.cpp, TEST-ONLY).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fjsp_env.h"

namespace fjsp {

// fmix64 counter RNG for synthetic actions (oracle_actions spec)
FJSP_DEV uint64_t fmix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// The word env gid's synthetic actions of vector step `step` are cut from (one byte per agent).
FJSP_DEV uint64_t action_word(uint64_t seed, uint32_t gid, uint32_t step) {
    return fmix64(seed ^ fmix64(((uint64_t)gid << 32) | step));
}

// FJSP_ACTIONS_MASKED: agent a's byte of h scaled by the number of its valid actions picks the
// j-th set bit of its mask (spec: oracle/fjsp_oracle.c oracle_actions with masks).
FJSP_DEV void masked_actions(uint64_t h, const Env& E, const Cfg& C, int* act) {
    MaskBits mb;
    compute_masks(E, C, mb);
#pragma unroll
    for (int a = 0; a < NA; a++) {
        const uint32_t bits = mb.bits[a];
        const int cnt = __builtin_popcount(bits);
        int j = (int)((((uint32_t)(h >> (8 * a)) & 0xFFu) * (uint32_t)cnt) >> 8);
        // j-th set bit
        uint32_t b = bits;
        for (int k = 0; k < j; k++) b &= b - 1u;
        act[a] = __builtin_ffs((int)b) - 1;
    }
}

// The perturbed heuristic: each agent follows heuristic_actions, except that with probability
// eps8 / 256 (its byte of a second word h2, an independent coin per agent and step) it takes the
// masked-uniform draw of the same (seed, gid, step).  eps8 = 0 is the heuristic and eps8 = 256 the
// masked stream, byte for byte.
constexpr uint64_t EPS_COIN_MIX = 0x9E3779B97F4A7C15ull;
FJSP_DEV void eps_heuristic_actions(uint64_t seed, uint32_t gid, uint32_t step, int eps8, const Env& E, const Tables& T,
                                    const Cfg& C, int* act) {
    const uint64_t h = action_word(seed, gid, step);
    const uint64_t h2 = fmix64(h ^ EPS_COIN_MIX);
    int m[NA];
    masked_actions(h, E, C, m);
    heuristic_actions(E, T, act);
#pragma unroll
    for (int a = 0; a < NA; a++)
        if ((int)((h2 >> (8 * a)) & 0xFFu) < eps8) act[a] = m[a];
}

// End record of one lane of fjsp_search_rollout.
constexpr uint32_t SEARCH_TERM = 1u, SEARCH_TRUNC = 2u;
struct LaneEnd {
    int32_t steps;              // k + 1 at the lane's first step that reported term or trunc; -1: none within K
    uint32_t flags;             // SEARCH_TERM | SEARCH_TRUNC of that step
    int32_t orders_completed;   // the infos of the lane's last executed step
    int32_t packaged;
    double sim_time;
};

// One lane of fjsp_search_rollout: up to K steps of one env without auto-reset, stopping at the first
// that reports term or trunc (a finished env is not stepped again).  Step k takes the lane's script
// row while k < script_len (script[(k * 8 + a) * stride]) and eps_heuristic_actions(seed, gid,
// step0 + k, eps8) on the current state after that; the action taken goes to trace[(k * 8 + a) *
// stride].  The step is FJSPSimulation.step (FJSPSimulation.py:144-242) without its outputs: no
// observation and no reward is built, only the sticky status bit the observation would set.
FJSP_DEV LaneEnd search_lane(Env& E, const Tables& T, const Cfg& C, int K, int eps8, uint64_t seed, uint32_t gid,
                             uint32_t step0, const uint8_t* script, int script_len, uint8_t* trace, size_t stride) {
    LaneEnd r{-1, 0u, 0, 0, 0.0};
    for (int k = 0; k < K; k++) {
        int act[NA];
        if (k < script_len) {
#pragma unroll
            for (int a = 0; a < NA; a++) act[a] = script[((size_t)k * NA + a) * stride];
        } else {
            eps_heuristic_actions(seed, gid, step0 + (uint32_t)k, eps8, E, T, C, act);
        }
#pragma unroll
        for (int a = 0; a < NA; a++) trace[((size_t)k * NA + a) * stride] = (uint8_t)act[a];
        uint32_t res[NA];
        (void)env_advance<true>(E, T, C, act, nullptr, res);
        flag_obs_overflow(E);
        const auto [all_done, truncated] = episode_end(E, C);
        r.orders_completed = E.ncompleted();
        r.packaged = E.total_packaged();
        r.sim_time = (double)(E.step() + 1) * (double)C.step_size;
        E.set_step(E.step() + 1);
        if (all_done || truncated) {
            r.steps = k + 1;
            r.flags = (all_done ? SEARCH_TERM : 0u) | (truncated ? SEARCH_TRUNC : 0u);
            break;
        }
    }
    return r;
}

}  // namespace fjsp

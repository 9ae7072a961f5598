// station_i8_shim.cpp — TEST-ONLY host build of fjsp_env.h's station_i8 (the stations' is_busy /
// queue_length of a state, k_policy_step's KPI output obs_i8) for tests/test_station_i8_host.py:
// random rollouts with auto-reset and a constructed state, both against what observe() hands its
// sink's i8().  Its rollout is written out here and not replay.h's: there is one world, no second
// schedule of the step, and the state is compared once more after every reset.
#include "world.h"

namespace {

// what observe() hands i8(), as the sinks store it: (int8_t)v
struct I8Sink {
    int8_t v[NI8];
    int seen;
    void i32(int, int) {}
    void i8(int f, int x) { v[f] = (int8_t)x; seen |= 1 << f; }
    void f32(int, float) {}
    void mask(int, int) {}
};

// observe() on a copy (it may flag the state) against station_i8 on the state itself, which must
// stay as it is; returns the number of differing fields
int compare(const Env& E, const Cfg& C, int* nonzero) {
    Env O = E;
    I8Sink sink;
    memset(&sink, 0, sizeof(sink));
    observe(O, C, sink);
    int8_t got[NI8];
    memset(got, 0x5A, sizeof(got));
    const Env before = E;
    station_i8(E, got);
    int bad = sink.seen != (1 << NI8) - 1 || memcmp(before.w, E.w, sizeof(E.w)) != 0;
    for (int f = 0; f < NI8; f++) {
        bad += got[f] != sink.v[f];
        if (got[f] != 0) nonzero[f]++;
    }
    return bad;
}

}  // namespace

extern "C" {

// `envs` envs x `steps` steps of uniform-random actions with auto-reset; after every step (before
// the reset, as the step kernels emit obs_i8) and after every reset.  out: states compared,
// states with a difference, resets, then per field the states where it was non-zero.
void station_i8_replay(int envs, int steps, int num_orders, uint64_t seed, int64_t* out) {
    const Cfg C = default_cfg();
    for (int i = 0; i < 3 + NI8; i++) out[i] = 0;
    int nonzero[NI8] = {0};
    for (int e = 0; e < envs; e++) {
        Lcg ga{seed * 1000003ull + (uint64_t)e}, gr{seed + 77ull * (uint64_t)e};
        World W;
        memset(&W, 0, sizeof(W));
        reset_world(W, C, num_orders, gr);
        Tables T = W.tabs();
        for (int k = 0; k < steps; k++) {
            int act[NA];
            draw_actions(ga, act);
            uint32_t res[NA];
            double rew[NA];
            env_step<true>(W.E, T, C, act, nullptr, res, rew);
            out[0]++;
            out[1] += compare(W.E, C, nonzero) != 0;
            const bool done = episode_over(W.E, C);
            W.E.set_step(W.E.step() + 1);
            if (done) {
                reset_world(W, C, W.E.norders(), gr);
                out[2]++;
                out[0]++;
                out[1] += compare(W.E, C, nonzero) != 0;
            }
        }
    }
    for (int f = 0; f < NI8; f++) out[3 + f] = nonzero[f];
}

// a state whose queue words are above 127: machine queue lengths q0 / q1 (list words), the
// packaging stations' queued counts qp, every station busy or not.  got / want: the twelve values
// of station_i8 and of observe()'s i8(); status: the state's status word after station_i8 and after
// observe() (which flags the overflow).
void station_i8_case(int q0, int q1, int qp, int busy, int8_t* got, int8_t* want, uint32_t* status) {
    const Cfg C = default_cfg();
    Env E;
    env_clear(E, C);
    E.set_list(L_M0Q, 0, 0, q0);
    E.set_list(L_M1Q, 0, 0, q1);
    for (int m = 0; m < 2; m++) E.set_m_busy(m, busy);
    for (int s = 0; s < 4; s++) {
        E.set_p_queued(s, qp + s);
        E.set_p_busy(s, busy);
    }
    station_i8(E, got);
    status[0] = E.status();
    I8Sink sink;
    memset(&sink, 0, sizeof(sink));
    observe(E, C, sink);
    memcpy(want, sink.v, NI8);
    status[1] = E.status();
}

}  // extern "C"

// held_shim.cpp — TEST-ONLY host build of fjsp_env.h's held_words (the held-tray words of
// fjsp_step_held) for tests/test_held_host.py: replays of the reference's recorded runs (actions and
// order tables from the fixtures) and constructed states with stale code bits.
#include "world.h"

namespace {

// held_words on the state itself, which must stay as it is (status included)
bool held_pure(const Env& E, uint32_t* v) {
    const Env before = E;
    held_words(E, v);
    return memcmp(before.w, E.w, sizeof(E.w)) == 0;
}

}  // namespace

extern "C" {

// One recorded run: actions u8 [T][8], the recorded result words u32 [T][8] and flags u8 [T], the
// order tables u8 [episodes][num_orders][3] of its episodes in order.  held u32 [T][3] receives the
// held-tray words of the state after each step and before the reset.  out: [0] steps whose result
// words differ from the recording, [1] steps whose term / trunc differ, [2] resets, [3] states that
// held_words changed, [4] status bits ORed over the run.
void held_replay(const uint8_t* actions, const uint32_t* results, const uint8_t* term, const uint8_t* trunc,
                 const uint8_t* orders, int episodes, int num_orders, int T, uint32_t* held, int64_t* out) {
    const Cfg C = default_cfg();
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
        out[3] += !held_pure(W.E, held + 3 * t);
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

// Constructed states.  v [6][3] held words, raw [6] the stale code fields, ok [0] = held_words left
// every state as it was:
//   0 a machine holding a finished tray (code `code`)         1 the same after its SIGNAL
//   2 the AGV carrying `code` at the small machine            3 after its DROP there
//   4 both holding an empty tray of the same order / start    5 a fresh env
void held_cases(int code, uint32_t* v, uint32_t* raw, int* ok) {
    const Cfg C = default_cfg();
    World W;
    memset(&W, 0, sizeof(W));
    const uint8_t table[3] = {9, 1, 1};   // one SMALL order of 9 products
    reset_world(W, C, 1, table);
    Tables Tb = W.tabs();
    Env& E = W.E;
    bool pure = true;
    E.set_m_grant(1, 7, code, 0);
    pure = held_pure(E, v) && pure;                       raw[0] = (uint32_t)E.m_code(1);
    int slot = -1;
    machine_execute<1>(E, Tb, 2, &slot);
    pure = held_pure(E, v + 3) && pure;                   raw[1] = (uint32_t)E.m_code(1);
    E.set_loc(LOC_SMALL);
    W.scode[9] = (uint16_t)code;
    E.set_carried(9, code, 1, 1, 1, 1);
    pure = held_pure(E, v + 6) && pure;                   raw[2] = (uint32_t)E.carry_code();
    int move_to = 0;
    const uint32_t r = agv_execute(E, Tb, C, 7, &move_to);
    pure = held_pure(E, v + 9) && pure && (r & 16u);      raw[3] = (uint32_t)E.carry_code();
    const int empty = code & 0x3FF;   // count 0, order and start kept
    E.set_carried(11, empty, 0, 0, 0, 0);
    E.set_m_grant(0, 12, empty, 0);
    pure = held_pure(E, v + 12) && pure;                  raw[4] = (uint32_t)E.carry_code();
    env_clear(E, C);
    pure = held_pure(E, v + 15) && pure;                  raw[5] = 0;
    *ok = pure;
}

}  // extern "C"

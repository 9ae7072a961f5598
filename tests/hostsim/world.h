// world.h — TEST-ONLY scaffolding shared by the host shims of this directory: one env with its
// stride-1 tables, the default config and reward table, the random streams of the replays, the
// episode-end predicate and the comparers.  Header only, no state.  README.md says how a shim uses it.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define FJSP_DEV inline
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h"
using namespace fjsp;

struct World {   // one env with its tables (stride 1)
    Env E;
    uint32_t orders[MAX_ORDERS];
    uint16_t scode[MAX_SLOTS];
    uint8_t snext[MAX_SLOTS];
    uint16_t scstep[MAX_SLOTS];
    Tables tabs() { return Tables{orders, scode, snext, scstep, 1}; }
};

struct BookWorld : World {   // with the env's pre-draw record, which put_orders_env drops (fjsp_orders.h)
    uint32_t pgw;
};

// a fresh world for a constructed case, its links and completion steps stale: a missing store shows
inline void poison_world(World& W) {
    memset(&W, 0, sizeof(W));
    memset(W.snext, 0x77, sizeof(W.snext));
    memset(W.scstep, 0x55, sizeof(W.scstep));
}

// the default reward weights (fjsp_reward_weights order) and their table
constexpr double DEFAULT_WEIGHTS[NW] = {100.0, 10.0, -0.1, 1.0, 5.0, -1.0, 2.0, -0.1, 10.0, -5.0, 5.0, 1.0, -2.0, 20.0, 2.0, -1.0};
inline void default_lut(double* lut, int step_size = 10) { build_reward_lut(DEFAULT_WEIGHTS, step_size, lut); }

// the default config over the default reward table; a shim that differs assigns the fields after the call
inline Cfg default_cfg() {
    static double lut[RLUT_SIZE];
    static const bool built = (default_lut(lut), true);
    (void)built;
    Cfg C;
    C.step_size = 10; C.max_steps = 200; C.tray_cap = 5; C.mask_tray_cap = 5; C.storage_cap = 100;
    C.pool0 = 1000; C.pkg_cap = 20; C.ptk_small = 6; C.ptk_big = 12; C.ptk_pack = 3;
    C.lut = lut;
    return C;
}

struct Lcg {
    uint64_t s;
    uint32_t next(uint32_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33) % n; }
};

// a reset with an order table drawn from g (a replay's own stream) ...
inline void reset_world(World& W, const Cfg& C, int num_orders, Lcg& g) {
    env_clear(W.E, C);
    W.E.set_norders(num_orders);
    for (int o = 0; o < num_orders; o++) {
        const int n = 1 + (int)g.next(9), ty = 1 + (int)g.next(3), co = 1 + (int)g.next(3);
        W.orders[o] = ow_make(n, ty, co);
    }
}
// ... or with a recorded one, table [num_orders][3]
inline void reset_world(World& W, const Cfg& C, int num_orders, const uint8_t* table) {
    env_clear(W.E, C);
    W.E.set_norders(num_orders);
    for (int o = 0; o < num_orders; o++) W.orders[o] = ow_make(table[3 * o], table[3 * o + 1], table[3 * o + 2]);
}

// uniform-random actions of one step, agent by agent
inline void draw_actions(Lcg& g, int act[NA]) {
    const int nact[NA] = {3, 8, 3, 3, 3, 3, 3, 3};
    for (int a = 0; a < NA; a++) act[a] = (int)g.next((uint32_t)nact[a]);
}

// the episode's end, read after a step and before the step counter moves on
inline bool all_done(const Env& E) {
    const int nord = E.norders();
    return E.ncompleted() == nord && nord > 0 && E.next_order() == nord;
}
inline bool episode_over(const Env& E, const Cfg& C) { return all_done(E) || E.step() >= C.max_steps; }

// every state word and every table byte
inline bool same_world(const World& A, const World& B) {
    return memcmp(A.E.w, B.E.w, sizeof(A.E.w)) == 0 && memcmp(A.orders, B.orders, sizeof(A.orders)) == 0 &&
           memcmp(A.scode, B.scode, sizeof(A.scode)) == 0 && memcmp(A.snext, B.snext, sizeof(A.snext)) == 0 &&
           memcmp(A.scstep, B.scstep, sizeof(A.scstep)) == 0;
}

// Every state word and the live part of the tables, R being the reference: the orders below
// num_orders and the slots below R's slot_next.  Two links are exempt.  The carried slot's is dead
// (no list holds it; every push rewrites it), and a wave that splits the AGV's step (agv_pre) may
// already have cleared it.  dead_slot is for a wave that runs an agent ahead of the reference: the
// link of L_PREADY's tail may already name the tray of a pickup run ahead (pickup_ahead_shim.cpp),
// which checks what that link may hold itself.
inline bool same_live(const World& R, const World& S, int num_orders, int dead_slot = NIL) {
    const int nslot = R.E.slot_next(), carry = R.E.carry();
    bool ok = memcmp(R.E.w, S.E.w, sizeof(R.E.w)) == 0 && memcmp(R.orders, S.orders, 4u * (size_t)num_orders) == 0 &&
              memcmp(R.scode, S.scode, 2u * (size_t)nslot) == 0 && memcmp(R.scstep, S.scstep, 2u * (size_t)nslot) == 0;
    for (int s = 0; s < nslot; s++) ok = ok && (s == carry || s == dead_slot || R.snext[s] == S.snext[s]);
    return ok;
}

// counts the failed checks in *count and keeps the first one's message
struct Mismatch {
    int64_t* count;
    char* msg;
    int len;
    Mismatch(int64_t* count_, char* msg_, int len_) : count(count_), msg(msg_), len(len_) { *count = 0; msg[0] = 0; }
    __attribute__((format(printf, 3, 4))) void check(bool ok, const char* fmt, ...) {
        if (ok || (*count)++) return;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, (size_t)len, fmt, ap);
        va_end(ap);
    }
};

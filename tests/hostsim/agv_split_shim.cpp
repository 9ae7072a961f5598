// agv_split_shim.cpp — TEST-ONLY host build of the AGV step's two halves
// (multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h: agv_pre + agv_fin, k_step_ag's P wave) for
// tests/test_agv_split_host.py: a constructed sweep and a replay in P's schedule, both against
// agv_execute<true> / the plain step.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#define FJSP_DEV inline
#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h"
using namespace fjsp;

namespace {

struct World {   // one env with its tables (stride 1)
    Env E;
    uint32_t orders[MAX_ORDERS];
    uint16_t scode[MAX_SLOTS];
    uint8_t snext[MAX_SLOTS];
    uint16_t scstep[MAX_SLOTS];
    Tables tabs() { return Tables{orders, scode, snext, scstep, 1}; }
};

Cfg make_cfg(int storage_cap, const double* lut) {
    Cfg C;
    C.step_size = 10; C.max_steps = 200; C.tray_cap = 5; C.mask_tray_cap = 5; C.storage_cap = storage_cap;
    C.pool0 = 1000; C.pkg_cap = 20; C.ptk_small = 6; C.ptk_big = 12; C.ptk_pack = 3;
    C.lut = lut;
    return C;
}

void fill(World& W, int lid, int len, int* slot_order) {   // `len` trays of distinct orders on list lid
    Tables T = W.tabs();
    for (int i = 0; i < len; i++) {
        const int o = (*slot_order)++ % 8;
        const int s = slot_new(W.E, T, tc_make(o, 0, ow_n(W.orders[o])));
        list_push_dyn<0x3Fu>(W.E, T, lid, s);
    }
}

// what other agents do between the two halves: a push on the AGV's source list (pickup station,
// a machine's SIGNAL), a pop on its destination queue (a machine's START)
void others(World& W, int change, int src, int dst) {
    Tables T = W.tabs();
    if ((change & 1) && src >= 0 && src != L_STORAGE) {
        const int s = slot_new(W.E, T, tc_make(7, 0, ow_n(W.orders[7])));
        list_push_dyn<0x3Fu>(W.E, T, src, s);
    }
    if ((change & 2) && (dst == L_M0Q || dst == L_M1Q) && (W.E.w[7 + dst] >> 16) != 0) list_pop_dyn<0x3Fu>(W.E, T, dst);
}

bool same(const World& A, const World& B) {
    return memcmp(A.E.w, B.E.w, sizeof(A.E.w)) == 0 && memcmp(A.orders, B.orders, sizeof(A.orders)) == 0 &&
           memcmp(A.scode, B.scode, sizeof(A.scode)) == 0 && memcmp(A.snext, B.snext, sizeof(A.snext)) == 0 &&
           memcmp(A.scstep, B.scstep, sizeof(A.scstep)) == 0;
}

struct Lcg {
    uint64_t s;
    uint32_t next(uint32_t n) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33) % n; }
};

void reset_world(World& W, const Cfg& C, int num_orders, Lcg& g) {
    env_clear(W.E, C);
    W.E.set_norders(num_orders);
    for (int o = 0; o < num_orders; o++) {
        const int n = 1 + (int)g.next(9), ty = 1 + (int)g.next(3), co = 1 + (int)g.next(3);
        W.orders[o] = ow_make(n, ty, co);
    }
}

}  // namespace

extern "C" {

// (a) every action x location x carried tray x source / destination length x storage cap x change of
// the other agents.  out: cases, mismatches, cases with pre_len == 0 -> len > 0, with pre_len == 1 ->
// len >= 2, pickups, drops that push.  msg: the first mismatch.
void agv_sweep(int64_t* out, char* msg, int msg_len) {
    static double lut[RLUT_SIZE];
    for (int i = 0; i < 6; i++) out[i] = 0;
    msg[0] = 0;
    // carried tray: none, an empty one, and one of each type unprocessed / processed / packaged
    struct Hand { int has, count, type, processed, packaged; };
    Hand hands[11];
    int nh = 0;
    hands[nh++] = Hand{0, 0, 0, 0, 0};
    hands[nh++] = Hand{1, 0, 0, 0, 0};
    for (int ty = 1; ty <= 3; ty++)
        for (int st = 0; st < 3; st++) hands[nh++] = Hand{1, 3, ty, st >= 1, st >= 2};
    for (int action = 0; action < 8; action++)
    for (int loc = 1; loc <= 5; loc++)
    for (int h = 0; h < nh; h++)
    for (int slen = 0; slen <= 3; slen++)
    for (int dlen = 0; dlen <= 3; dlen++)
    for (int capmode = 0; capmode < 2; capmode++)
    for (int change = 0; change < 4; change++) {
        const int src = nib(nibs(0xF, L_PREADY, L_M1R, L_M0R, L_STORAGE, 0xF), loc) == 0xF ? -1
                        : nib(nibs(0xF, L_PREADY, L_M1R, L_M0R, L_STORAGE, 0xF), loc);
        const int dst = nib(nibs(0xF, 0xF, L_M1Q, L_M0Q, L_STORAGE, 0xF), loc) == 0xF ? -1
                        : nib(nibs(0xF, 0xF, L_M1Q, L_M0Q, L_STORAGE, 0xF), loc);
        World W;
        memset(&W, 0, sizeof(W));
        memset(W.snext, 0x77, sizeof(W.snext));     // stale links: a missing store shows
        memset(W.scstep, 0x55, sizeof(W.scstep));
        // storage at its cap (capmode 0) or below it
        const int storage_len = src == L_STORAGE ? slen : 0;
        const Cfg C = make_cfg(capmode == 0 ? storage_len : storage_len + 1, lut);
        env_clear(W.E, C);
        W.E.set_norders(10);
        // orders 0..7 for list trays (types, colours and processed / packaged states vary), 8 carried
        for (int o = 0; o < 8; o++) {
            const uint32_t n = 2 + o % 4, full = (1u << n) - 1u;
            W.orders[o] = ow_make((int)n, 1 + o % 3, 1 + (o / 3) % 3) | (o & 1 ? full : 0u) | (o & 2 ? full << 9 : 0u);
        }
        const Hand& H = hands[h];
        W.orders[8] = ow_make(3, H.type ? H.type : 1, 1 + h % 3) | (H.processed ? 7u : 0u) | (H.packaged ? 7u << 9 : 0u);
        W.E.w[5] = (7u << 8);   // a small pool
        Tables T = W.tabs();
        int so = loc + h;       // which orders the list trays belong to varies with the case
        if (src >= 0) fill(W, src, slen, &so);
        if (dst >= 0 && dst != src) fill(W, dst, dlen, &so);
        W.E.set_loc(loc);
        if (H.has) {
            const int code = tc_make(8, 0, H.count);
            const int s = slot_new(W.E, T, code);
            const uint32_t ow = W.orders[8];
            if (H.count)
                W.E.set_carried(s, code, ow_type(ow), ow_color(ow), (ow & 7u) != 7u, ((ow >> 9) & 7u) != 7u);
            else
                W.E.set_carried(s, code, 0, 0, 0, 0);
        }
        World A = W, B = W;
        Tables TA = A.tabs(), TB = B.tabs();
        const AgvPre pre = agv_pre(A.E, TA, C, action);
        others(A, change, src, dst);
        others(B, change, src, dst);
        // which path the case takes
        const bool want6 = action == 6 && !H.has && loc != LOC_PACK;
        const uint32_t len_before = want6 ? (W.E.w[7 + src] >> 16) : 0u, len_after = want6 ? (B.E.w[7 + src] >> 16) : 0u;
        if (want6 && len_before == 0 && len_after > 0) out[2]++;
        if (want6 && len_before == 1 && len_after >= 2) out[3]++;
        int mva = 0, mvb = 0;
        uint32_t pa = 0, pb = 0;
        const uint32_t ra = agv_fin(A.E, TA, pre, &mva, &pa);
        const uint32_t rb = agv_execute<true>(B.E, TB, C, action, &mvb, &pb) | ((uint32_t)action << 8);
        if (mvb) B.E.set_loc(mvb);   // agv_fin folds the move into W6
        if (rb & 8u) out[4]++;
        if ((rb & 16u) && dst >= 0 && !(dst == L_STORAGE && capmode == 0)) out[5]++;
        out[0]++;
        if (!(same(A, B) && ra == rb && mva == mvb && pa == pb)) {
            if (!out[1]++)
                snprintf(msg, (size_t)msg_len, "action %d loc %d hand %d slen %d dlen %d capmode %d change %d: r %x/%x mv %d/%d "
                         "pend %x/%x w6 %x/%x state %d", action, loc, h, slen, dlen, capmode, change, ra, rb, mva, mvb, pa, pb,
                         A.E.w[6], B.E.w[6], (int)same(A, B));
        }
    }
}

// (b) `envs` envs x `steps` steps of uniform-random actions with auto-reset: the plain step against
// the step in P's schedule (AGV of step k -> agv_pre of k+1 -> the rest of step k -> pickup of
// k+1 -> agv_fin).  out: env-steps compared, mismatches, rare path 0 (front new), rare path 1
// (successor new), resets.
void agv_replay(int envs, int steps, int num_orders, uint64_t seed, int64_t* out, char* msg, int msg_len) {
    static double lut[RLUT_SIZE];
    const double w[NW] = {100.0, 10.0, -0.1, 1.0, 5.0, -1.0, 2.0, -0.1, 10.0, -5.0, 5.0, 1.0, -2.0, 20.0, 2.0, -1.0};
    build_reward_lut(w, 10, lut);
    const Cfg C = make_cfg(100, lut);
    for (int i = 0; i < 5; i++) out[i] = 0;
    msg[0] = 0;
    const int nact[NA] = {3, 8, 3, 3, 3, 3, 3, 3};
    for (int e = 0; e < envs; e++) {
        Lcg ga{seed * 1000003ull + (uint64_t)e}, gr_ref{seed + 77ull * (uint64_t)e}, gr_split = gr_ref;
        World R, S;
        memset(&R, 0, sizeof(R));
        memset(&S, 0, sizeof(S));
        reset_world(R, C, num_orders, gr_ref);
        reset_world(S, C, num_orders, gr_split);
        Tables TR = R.tabs(), TS = S.tabs();
        int act[NA], nxt[NA];
        for (int a = 0; a < NA; a++) nxt[a] = (int)ga.next((uint32_t)nact[a]);
        bool fresh = true;
        uint32_t r0 = 0, r1 = 0, pend = 0;
        int mv = 0;
        for (int k = 0; k < steps; k++) {
            for (int a = 0; a < NA; a++) { act[a] = nxt[a]; nxt[a] = (int)ga.next((uint32_t)nact[a]); }
            // plain step
            uint32_t res_ref[NA], res[NA];
            double rew[NA];
            env_step<true>(R.E, TR, C, act, nullptr, res_ref, rew);
            // P's schedule
            if (fresh) {   // the launch's first step, and the step after a reset: both agents in place
                r0 = pickup_execute(S.E, TS, C, act[0]);
                mv = 0; pend = 0;
                r1 = agv_execute<true>(S.E, TS, C, act[1], &mv, &pend) | ((uint32_t)act[1] << 8);
                if (mv) S.E.set_loc(mv);
                fresh = false;
            }
            const AgvPre pre = agv_pre(S.E, TS, C, nxt[1]);   // step k + 1's AGV, its own half
            if (pend) agv_pack_drop(S.E, TS, C, pend);
            // the rest of step k: the move lands inside the run (machine_execute does not read the
            // location), the pickup station and the AGV have acted (255 = no action)
            if (mv) S.E.set_loc(mv);
            int rest[NA];
            for (int a = 0; a < NA; a++) rest[a] = a < 2 ? 255 : act[a];
            env_advance<true>(S.E, TS, C, rest, nullptr, res);
            res[0] = r0; res[1] = r1;
            // compare: state words, results, the live tables.  The carried slot's link is dead (no
            // list holds it; every push rewrites it) and agv_pre may already have cleared it.
            bool ok = memcmp(R.E.w, S.E.w, sizeof(R.E.w)) == 0;
            for (int a = 0; a < NA; a++) ok = ok && (a == 1 ? (res_ref[1] | ((uint32_t)act[1] << 8)) == res[1] : res_ref[a] == res[a]);
            const int nslot = R.E.slot_next(), carry = R.E.carry();
            ok = ok && memcmp(R.orders, S.orders, 4u * (size_t)num_orders) == 0 && memcmp(R.scode, S.scode, 2u * (size_t)nslot) == 0;
            for (int s = 0; s < nslot; s++) ok = ok && (s == carry || R.snext[s] == S.snext[s]) && R.scstep[s] == S.scstep[s];
            out[0]++;
            if (!ok && !out[1]++) snprintf(msg, (size_t)msg_len, "env %d step %d (orders %d): split differs from the plain step", e, k, num_orders);
            // end of step: auto-reset (the next table continues each side's own stream)
            const int nord = R.E.norders();
            const bool done = (R.E.ncompleted() == nord && nord > 0 && R.E.next_order() == nord) || R.E.step() >= C.max_steps;
            R.E.set_step(R.E.step() + 1);
            S.E.set_step(S.E.step() + 1);
            if (done) {
                reset_world(R, C, nord, gr_ref);
                reset_world(S, C, nord, gr_split);
                fresh = true;
                out[4]++;
            } else {
                r0 = pickup_execute(S.E, TS, C, nxt[0]);
                if (!pre.force && pre.thr != ~0u) {   // which rare path agv_fin takes: the source list's final length
                    uint32_t len = 0;
                    for (int i = 0; i < 6; i++) len = pre.m[i] ? S.E.w[7 + i] >> 16 : len;
                    if (len > pre.thr) out[2 + pre.thr]++;
                }
                mv = 0; pend = 0;
                r1 = agv_fin(S.E, TS, pre, &mv, &pend);
            }
        }
    }
}

}  // extern "C"

// pickup_ahead_shim.cpp — TEST-ONLY host build of the pickup station run ahead of the AGV's
// previous step (multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h: pickup_execute on the words before
// that AGV + pickup_compose, k_step_ag's E3 wave) for tests/test_pickup_ahead_host.py: a
// constructed sweep and a replay in the kernel's schedule, both against the plain order.
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

Cfg make_cfg(int pool0, const double* lut) {
    Cfg C;
    C.step_size = 10; C.max_steps = 200; C.tray_cap = 5; C.mask_tray_cap = 5; C.storage_cap = 100;
    C.pool0 = pool0; C.pkg_cap = 20; C.ptk_small = 6; C.ptk_big = 12; C.ptk_pack = 3;
    C.lut = lut;
    return C;
}

bool same(const World& A, const World& B) {
    return memcmp(A.E.w, B.E.w, sizeof(A.E.w)) == 0 && memcmp(A.orders, B.orders, sizeof(A.orders)) == 0 &&
           memcmp(A.scode, B.scode, sizeof(A.scode)) == 0 && memcmp(A.snext, B.snext, sizeof(A.snext)) == 0 &&
           memcmp(A.scstep, B.scstep, sizeof(A.scstep)) == 0;
}

// the AGV's delta on the pickup's words: a PICKUP pops L_PREADY's front (bit 0), a DROP of an
// empty tray at the pickup location refills the pool (bit 1)
uint32_t agv_delta(World& W, int delta) {
    Tables T = W.tabs();
    if ((delta & 1) && W.E.ll(L_PREADY) > 0) list_pop<L_PREADY>(W.E, T);
    if (delta & 2) W.E.set_pool(W.E.pool() + 1);
    return (delta & 2) ? PKS_POOL_ADD : 0u;
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

// the pickup's words of an env, as E3 holds them
struct Pk {
    uint32_t w0, w4, w5, w7, r, st;
};
Pk pk_run(const uint32_t w[4], const Tables& T, const Cfg& C, int action, bool speculative) {
    Env Ep;
    for (int i = 0; i < NSTATE; i++) Ep.w[i] = 0u;
    Ep.w[0] = w[0]; Ep.w[4] = w[1]; Ep.w[5] = w[2]; Ep.w[7] = w[3];
    uint32_t f = speculative && pickup_reads_empty_pool(Ep, action) ? PKS_POOL0 : 0u;
    const uint32_t r = pickup_execute(Ep, T, C, action);
    if (speculative && Ep.w[7] != w[3]) f |= PKS_PUSHED;
    return Pk{Ep.w[0], Ep.w[4], Ep.w[5], Ep.w[7], r | f, Ep.w[2]};
}

}  // namespace

extern "C" {

// (a) pickup action x current order x tray x pool x L_PREADY length x the AGV's delta x orders left.
// out: cases, mismatches, sensitive, pop and push at n = 1, pop and push at n >= 2, sensitive where the
// two orders agree.  msg: the first mismatch.
void pickup_sweep(int64_t* out, char* msg, int msg_len) {
    static double lut[RLUT_SIZE];
    for (int i = 0; i < 6; i++) out[i] = 0;
    msg[0] = 0;
    for (int action = 0; action < 3; action++)
    for (int cur = 0; cur < 3; cur++)        // no current order, mid-order, the order's last product next
    for (int tray = 0; tray < 3; tray++)     // no tray, partly filled, one below tray_cap
    for (int pool = 0; pool < 3; pool++)
    for (int len = 0; len <= 3; len++)
    for (int delta = 0; delta < 4; delta++)  // none, pop, pool_add, both
    for (int left = 0; left < 2; left++) {
        const Cfg C = make_cfg(1000, lut);
        World W;
        memset(&W, 0, sizeof(W));
        memset(W.snext, 0x77, sizeof(W.snext));     // stale links: a missing or an extra store shows
        memset(W.scstep, 0x55, sizeof(W.scstep));
        memset(W.scode, 0x33, sizeof(W.scode));
        env_clear(W.E, C);
        W.E.set_norders(6);
        for (int o = 0; o < 6; o++) W.orders[o] = ow_make(o == 2 ? 8 : 6, 1 + o % 3, 1 + (o / 2) % 3);
        W.E.set_next_order(left ? 4 : 6);
        const int co = cur == 0 ? -1 : cur == 1 ? 2 : 3;   // order 2 has 8 products, order 3 has 6
        if (co >= 0) {
            W.E.set_cur_order(co);
            W.E.set_cur_info(W.orders[co]);
            W.E.set_cur_idx(5);
        }
        const int cnt = tray == 1 ? 2 : C.tray_cap - 1;
        if (tray) {
            W.E.set_tray_valid(1);
            W.E.set_tray_count(cnt);
            W.E.set_tray_order(co >= 0 ? co : left ? 4 : 1);   // the order a LOAD would continue or start
            W.E.set_tray_start(co >= 0 ? 5 - cnt : 0);
        }
        W.E.set_pool(pool);
        Tables T = W.tabs();
        for (int i = 0; i < len; i++) list_push<L_PREADY>(W.E, T, slot_new(W.E, T, tc_make(i % 2, 0, 3)));
        // plain order: the AGV, then the pickup
        World B = W;
        Tables TB = B.tabs();
        agv_delta(B, delta);
        const uint32_t rb = pickup_execute(B.E, TB, C, action);
        // the other order, left as it is: the pickup, then the AGV
        World D = W;
        Tables TD = D.tabs();
        const uint32_t rd = pickup_execute(D.E, TD, C, action);
        agv_delta(D, delta);
        const bool agree = rd == rb && D.E.w[0] == B.E.w[0] && D.E.w[4] == B.E.w[4] && D.E.w[5] == B.E.w[5];
        // ahead: the pickup on the words before the AGV, the AGV on its own copy of them, compose
        World A = W, G = W;
        Tables TA = A.tabs();
        const uint32_t w[4] = {W.E.w[0], W.E.w[4], W.E.w[5], W.E.w[7]};
        const Pk q = pk_run(w, TA, C, action, true);
        const uint32_t pool_add = agv_delta(G, delta);
        const PickupTrue pt = pickup_compose(q.w5, q.w7, q.r, pool_add, G.E.w[7]);
        uint32_t ra;
        const bool popped = (delta & 1) && len > 0, pushed = (q.r & PKS_PUSHED) != 0u;
        if (pt.sensitive) {
            out[2]++;
            if (agree) out[5]++;
            // the speculative run left no store behind: the pickup again, on the words after the AGV
            const uint32_t v[4] = {G.E.w[0], G.E.w[4], G.E.w[5], G.E.w[7]};
            const Pk t = pk_run(v, TA, C, action, false);
            A.E.w[0] = t.w0; A.E.w[4] = t.w4; A.E.w[5] = t.w5; A.E.w[7] = t.w7; A.E.w[2] |= t.st;
            ra = t.r;
        } else {
            if (pt.unlink) pickup_unlink(TA, q.w7);
            A.E.w[0] = q.w0; A.E.w[4] = q.w4; A.E.w[5] = pt.w5; A.E.w[7] = pt.w7; A.E.w[2] |= q.st;
            ra = q.r & 0xFFFFu;
            if (popped && pushed) out[len == 1 ? 3 : 4]++;
        }
        out[0]++;
        if (!(same(A, B) && ra == rb) || (pt.unlink != (!pt.sensitive && popped && pushed && len == 1))) {
            if (!out[1]++)
                snprintf(msg, (size_t)msg_len, "action %d cur %d tray %d pool %d len %d delta %d left %d: r %x/%x w0 %x/%x w4 %x/%x "
                         "w5 %x/%x w7 %x/%x sensitive %d unlink %d state %d", action, cur, tray, pool, len, delta, left, ra, rb,
                         A.E.w[0], B.E.w[0], A.E.w[4], B.E.w[4], A.E.w[5], B.E.w[5], A.E.w[7], B.E.w[7], (int)pt.sensitive,
                         (int)pt.unlink, (int)same(A, B));
        }
    }
}

// (b) `envs` envs x `steps` steps of uniform-random actions with auto-reset: the plain step against
// the step in the kernel's schedule (speculative pickup of step k+2 -> agv_pre of k+1 -> the rest
// of step k -> compose of the pickup of k+1 -> agv_fin).  out: env-steps compared, mismatches, the
// AGV pops L_PREADY, pop and push in one step, of those at n = 1, sensitive lanes, resets.
void pickup_replay(int envs, int steps, int num_orders, int pool0, uint64_t seed, int64_t* out, char* msg, int msg_len) {
    static double lut[RLUT_SIZE];
    const double w[NW] = {100.0, 10.0, -0.1, 1.0, 5.0, -1.0, 2.0, -0.1, 10.0, -5.0, 5.0, 1.0, -2.0, 20.0, 2.0, -1.0};
    build_reward_lut(w, 10, lut);
    const Cfg C = make_cfg(pool0, lut);
    for (int i = 0; i < 7; i++) out[i] = 0;
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
        int act[NA], nxt[NA], nx2[NA];
        for (int a = 0; a < NA; a++) nxt[a] = (int)ga.next((uint32_t)nact[a]);
        for (int a = 0; a < NA; a++) nx2[a] = (int)ga.next((uint32_t)nact[a]);
        bool fresh = true;
        uint32_t r0 = 0, r1 = 0, pend = 0, pool_add = 0;
        int mv = 0;
        Pk q{};   // E3: the speculative pickup of step k+1 at the top of step k
        for (int k = 0; k < steps; k++) {
            for (int a = 0; a < NA; a++) { act[a] = nxt[a]; nxt[a] = nx2[a]; nx2[a] = (int)ga.next((uint32_t)nact[a]); }
            // plain step
            uint32_t res_ref[NA], res[NA];
            double rew[NA];
            env_step<true>(R.E, TR, C, act, nullptr, res_ref, rew);
            // the kernel's schedule
            if (fresh) {   // the launch's first step, and the step after a reset: both agents in place
                r0 = pickup_execute(S.E, TS, C, act[0]);
                mv = 0; pend = 0;
                r1 = agv_execute<true>(S.E, TS, C, act[1], &mv, &pend) | ((uint32_t)act[1] << 8);
                if (mv) S.E.set_loc(mv);
            }
            // E3: the true pickup of step k+1 (composed, or run on the words after the AGV of step k
            // on a fresh or sensitive lane), then the speculative pickup of step k+2
            Pk t{};
            bool slow = fresh;
            if (!fresh) {
                const PickupTrue pt = pickup_compose(q.w5, q.w7, q.r, pool_add, S.E.w[7]);
                if (pt.unlink) pickup_unlink(TS, q.w7);
                t = Pk{q.w0, q.w4, pt.w5, pt.w7, q.r & 0xFFFFu, q.st};
                slow = pt.sensitive;
            }
            if (slow) {
                const uint32_t v[4] = {S.E.w[0], S.E.w[4], S.E.w[5], S.E.w[7]};
                t = pk_run(v, TS, C, nxt[0], false);
                if (!fresh) out[5]++;
            }
            if (k + 2 < steps) {
                const uint32_t v[4] = {t.w0, t.w4, t.w5, t.w7};
                q = pk_run(v, TS, C, nx2[0], true);
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
            // list holds it; every push rewrites it) and agv_pre may already have cleared it; the
            // link of L_PREADY's tail may already name the tray of a pickup run ahead.
            bool ok = memcmp(R.E.w, S.E.w, sizeof(R.E.w)) == 0;
            for (int a = 0; a < NA; a++) ok = ok && (a == 1 ? (res_ref[1] | ((uint32_t)act[1] << 8)) == res[1] : res_ref[a] == res[a]);
            const int nslot = R.E.slot_next(), carry = R.E.carry();
            const int ptail = R.E.ll(L_PREADY) > 0 ? R.E.lt(L_PREADY) : -1;
            ok = ok && memcmp(R.orders, S.orders, 4u * (size_t)num_orders) == 0 && memcmp(R.scode, S.scode, 2u * (size_t)nslot) == 0;
            for (int s = 0; s < nslot; s++)
                ok = ok && (s == carry || s == ptail || R.snext[s] == S.snext[s]) && R.scstep[s] == S.scstep[s];
            if (ptail >= 0) ok = ok && (S.snext[ptail] == NIL || S.snext[ptail] == nslot);
            out[0]++;
            if (!ok && !out[1]++) snprintf(msg, (size_t)msg_len, "env %d step %d (orders %d): the schedule differs from the plain step", e, k, num_orders);
            // end of step: auto-reset (the next table continues each side's own stream)
            const int nord = R.E.norders();
            const bool done = (R.E.ncompleted() == nord && nord > 0 && R.E.next_order() == nord) || R.E.step() >= C.max_steps;
            R.E.set_step(R.E.step() + 1);
            S.E.set_step(S.E.step() + 1);
            if (done) {   // what E3 ran ahead for this env is dropped
                reset_world(R, C, nord, gr_ref);
                reset_world(S, C, nord, gr_split);
                fresh = true;
                out[6]++;
            } else {
                // P: agv_fin on E3's post
                S.E.w[0] = (S.E.w[0] & 0x00FFFFFFu) | (t.w0 & 0xFF000000u);
                S.E.w[4] = t.w4; S.E.w[5] = t.w5; S.E.w[7] = t.w7; S.E.w[2] |= t.st;
                r0 = t.r;
                const uint32_t w7_in = S.E.w[7];
                mv = 0; pend = 0;
                r1 = agv_fin(S.E, TS, pre, &mv, &pend);
                pool_add = pre.pool_add;
                fresh = false;
                // the AGV of step k+1 popped L_PREADY; the pickup of step k+2 (run ahead of it, above)
                // pushed; the list held one tray before both
                if (S.E.w[7] != w7_in) {
                    out[2]++;
                    if (k + 2 < steps && (q.r & PKS_PUSHED)) {
                        out[3]++;
                        if ((w7_in >> 16) == 1u) out[4]++;
                    }
                }
            }
        }
    }
}

}  // extern "C"

// station_lanes_shim.cpp — TEST-ONLY host build of the packaging wave's lane-group form
// (multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h: pack_lane_*, k_step_ag's K wave) for
// tests/test_station_lanes_host.py.  The G lanes of an env run one after another here; the
// reference is the S = 0..3 sequence K ran before (pack_due / pack_complete<0..3>, agv_pack_drop,
// pack_execute / pack_finish<0..3>) on one Env.
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

Cfg make_cfg(int pkg_cap, const double* lut) {
    Cfg C;
    C.step_size = 10; C.max_steps = 200; C.tray_cap = 5; C.mask_tray_cap = 5; C.storage_cap = 100;
    C.pool0 = 1000; C.pkg_cap = pkg_cap; C.ptk_small = 6; C.ptk_big = 12; C.ptk_pack = 3;
    C.lut = lut;
    return C;
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

bool same_tables(const World& A, const World& B) {
    return memcmp(A.orders, B.orders, sizeof(A.orders)) == 0 && memcmp(A.scode, B.scode, sizeof(A.scode)) == 0 &&
           memcmp(A.snext, B.snext, sizeof(A.snext)) == 0 && memcmp(A.scstep, B.scstep, sizeof(A.scstep)) == 0;
}

// events of one reference step (what the inputs contain, counted on the S = 0..3 sequence alone)
struct Events {
    int64_t steps, two_stations, order_by_two, drop_to[4], drop_lost;
};

struct KOut {   // what K hands on after a step besides its state words
    uint32_t r[4];    // result | action << 8 per station
    uint32_t gs;      // orders completed | products packaged << 16 (the snapshot's SK_G)
};

// K's step as the S = 0..3 sequence on one Env (k_step_ag's K wave before the lane groups)
KOut k_step_ref(World& W, const Cfg& C, uint32_t a1, uint32_t pend, Events& ev) {
    Env& E = W.E;
    Tables T = W.tabs();
    const int step = E.step(), tp0 = E.total_packaged();
    int done[4], orders_done = 0;
    const bool due0 = pack_due<0>(E, T, step), due1 = pack_due<1>(E, T, step);
    const bool due2 = pack_due<2>(E, T, step), due3 = pack_due<3>(E, T, step);
    uint32_t before[MAX_ORDERS], touched[4][MAX_ORDERS];
    auto mark = [&](int s) {
        for (int o = 0; o < MAX_ORDERS; o++) touched[s][o] = (before[o] ^ W.orders[o]) & (0x1FFu << 9);
        memcpy(before, W.orders, sizeof(before));
    };
    uint32_t start[MAX_ORDERS];
    memcpy(start, W.orders, sizeof(start));
    memcpy(before, W.orders, sizeof(before));
    done[0] = pack_complete<0>(E, T, due0, &orders_done); mark(0);
    done[1] = pack_complete<1>(E, T, due1, &orders_done); mark(1);
    done[2] = pack_complete<2>(E, T, due2, &orders_done); mark(2);
    done[3] = pack_complete<3>(E, T, due3, &orders_done); mark(3);
    ev.steps++;
    if ((done[0] > 0) + (done[1] > 0) + (done[2] > 0) + (done[3] > 0) >= 2) ev.two_stations++;
    for (int o = 0; o < MAX_ORDERS; o++) {
        const bool completed = !(start[o] & (1u << 18)) && (W.orders[o] & (1u << 18));
        const int by = (touched[0][o] != 0) + (touched[1][o] != 0) + (touched[2][o] != 0) + (touched[3][o] != 0);
        if (completed && by >= 2) ev.order_by_two++;
    }
    if (pend) {
        const int st = pkg_station(E, C, (int)((pend >> 22) & 3u));
        if (st < 0) ev.drop_lost++;
        else ev.drop_to[st]++;
        agv_pack_drop(E, T, C, pend);
    }
    int st[4] = {0, 0, 0, 0};
    KOut out;
    out.r[0] = pack_execute<0>(E, (int)(a1 & 0xFFu), &st[0]);
    out.r[1] = pack_execute<1>(E, (int)((a1 >> 8) & 0xFFu), &st[1]);
    out.r[2] = pack_execute<2>(E, (int)((a1 >> 16) & 0xFFu), &st[2]);
    out.r[3] = pack_execute<3>(E, (int)(a1 >> 24), &st[3]);
    pack_finish<0>(E, T, C, st[0], done[0]);
    pack_finish<1>(E, T, C, st[1], done[1]);
    pack_finish<2>(E, T, C, st[2], done[2]);
    pack_finish<3>(E, T, C, st[3], done[3]);
    E.set_ncompleted(E.ncompleted() + orders_done);
    if (E.p_queued(0) > 127 || E.p_queued(1) > 127 || E.p_queued(2) > 127 || E.p_queued(3) > 127)
        E.flag(ST_OBS_OVERFLOW | ST_DIVERGED);
    for (int q = 0; q < 4; q++) out.r[q] = (out.r[q] & 0xFFu) | (((a1 >> (8 * q)) & 0xFFu) << 8);
    out.gs = (uint32_t)orders_done | ((uint32_t)(E.total_packaged() - tp0) << 16);
    return out;
}

// the env's G lanes: K's words of W's Env spread over them, as the launch prologue loads them
template <int G>
struct Lanes {
    Env L[G];
    void load(const Env& E) {
        for (int g = 0; g < G; g++) {
            for (int i = 0; i < NSTATE; i++) L[g].w[i] = 0u;
            pack_lane_load<G>(L[g], g, [&](int i) { return E.w[i]; });
            L[g].w[0] = E.w[0] & 0xFFFFu;
            L[g].w[2] = E.w[2];
        }
    }
    // K's step, the lanes one after another, the combines between the phases as the wave makes them
    KOut step(World& W, const Cfg& C, uint32_t a1, uint32_t pend) {
        Tables T = W.tabs();
        uint32_t room = 0, sums = 0, st = 0, r[G][4 / G];
        for (int g = 0; g < G; g++) room |= pack_lane_room<G>(L[g], C, g);
        for (int g = 0; g < G; g++) sums += pack_lane_step<G>(L[g], T, C, g, a1, pend, room, r[g]);
        for (int g = 0; g < G; g++) st |= L[g].w[2];
        KOut out;
        for (int g = 0; g < G; g++) {
            L[g].w[2] = st;
            pack_lane_apply(L[g], sums);
            for (int p = 0; p < 4 / G; p++) out.r[p * G + g] = r[g][p];
        }
        out.gs = (sums & 0xFFu) | ((sums >> 8) << 16);
        return out;
    }
    // K's words back into an Env, as the launch epilogue stores them; false if the groups disagree
    // on a word that is one per env
    bool store(Env& E) const {
        bool ok = true;
        for (int g = 0; g < G; g++) {
            ok = ok && L[g].w[1] == L[0].w[1] && L[g].w[2] == L[0].w[2] && L[g].w[0] == L[0].w[0];
            for (int p = 0; p < 4 / G; p++) {
                const int s = p * G + g;
                E.w[7 + L_PKG + s] = L[g].w[7 + L_PKG + p];
                E.w[20 + s] = L[g].w[20 + p];
                E.w[26 + s] = L[g].w[26 + p];
            }
        }
        E.w[1] = L[0].w[1];
        E.w[2] |= L[0].w[2];   // AM ORs K's status bits into its W2
        E.w[24] = 0u; E.w[25] = 0u;
        for (int g = 0; g < G; g++) { E.w[24] |= pack_lane_counts<G>(L[g], g, 0); E.w[25] |= pack_lane_counts<G>(L[g], g, 1); }
        return ok;
    }
};

// one K step of both forms from the same state; true if every state word, table byte, result word
// and snapshot word agrees
template <int G>
bool both(const World& W, const Cfg& C, uint32_t a1, uint32_t pend, Events& ev) {
    World A = W, B = W;
    const KOut ra = k_step_ref(A, C, a1, pend, ev);
    Lanes<G> lanes;
    lanes.load(B.E);
    const KOut rb = lanes.step(B, C, a1, pend);
    bool ok = lanes.store(B.E);
    ok = ok && memcmp(A.E.w, B.E.w, sizeof(A.E.w)) == 0 && same_tables(A, B);
    ok = ok && memcmp(ra.r, rb.r, sizeof(ra.r)) == 0 && ra.gs == rb.gs;
    return ok;
}

// constructed state of one station: 0 empty; 1 two runs queued; 2 a batch of two runs due now;
// 3 a batch due now and one run queued behind it; 4 a batch in flight, not due; 5 a batch in
// flight that fills the station (no room), not due
constexpr int NSTATES = 6;
void build_station(World& W, const Cfg& C, int s, int state, int step) {
    Tables T = W.tabs();
    Env& E = W.E;
    auto push = [&](int code, uint16_t cstep) {
        const int slot = slot_new(E, T, code);
        T.scstep[slot] = cstep;
        list_push_dyn<(0xFu << L_PKG)>(E, T, L_PKG + s, slot);
        return slot;
    };
    int inflight = 0, queued = 0, qfirst = NIL, busy = 0;
    if (state >= 2) {   // a batch of two runs: the first half of order s, the second half of order s + 1 (mod 4)
        const bool due = state == 2 || state == 3;
        push(tc_make(s, 0, 2), (uint16_t)(due ? step : step + 2));
        push(tc_make((s + 1) % 4, 2, 2), PKG_CONT);
        inflight = state == 5 ? C.pkg_cap : 4;
        busy = 1;
    }
    if (state == 1 || state == 3) {
        qfirst = push(tc_make(4 + s, 0, 3), PKG_CONT);
        queued = 3;
        if (state == 1) { push(tc_make(4 + s, 3, 1), PKG_CONT); queued = 4; }
    }
    E.w[20 + s] = (uint32_t)busy | ((uint32_t)(state >= 2) << 1) | ((uint32_t)qfirst << 2) | ((uint32_t)inflight << 10) |
                  ((uint32_t)queued << 18);
    E.w[26 + s] = state >= 2 ? 4u : 0u;
    E.set_p_completed(s, 3 * s + state);
}

template <int G>
void sweep_g(int64_t* out, char* msg, int msg_len, Events& ev) {
    static double lut[RLUT_SIZE];
    const Cfg C = make_cfg(6, lut);
    const int step = 17;
    for (int code = 0; code < NSTATES * NSTATES * NSTATES * NSTATES; code++)
    for (int acts = 0; acts < 81; acts++)
    for (int color = 0; color < 4; color++) {   // 0: no drop
        World W;
        memset(&W, 0, sizeof(W));
        memset(W.snext, 0x77, sizeof(W.snext));     // stale links: a missing store shows
        memset(W.scstep, 0x55, sizeof(W.scstep));
        env_clear(W.E, C);
        W.E.set_norders(10);
        W.E.set_step(step);
        W.E.set_total_packaged(40);
        W.E.set_ncompleted(1);
        // orders 0..3: four products, split over two stations' batches, processed; 4..7 queued; 8 dropped
        for (int o = 0; o < 4; o++) W.orders[o] = ow_make(4, 1 + o % 3, 1 + o % 3) | 0xFu;
        for (int o = 4; o < 8; o++) W.orders[o] = ow_make(4, 1 + o % 3, 1 + o % 3) | 0xFu;
        W.orders[8] = ow_make(3, 1, color ? color : 1) | 7u;
        int c = code, a = acts;
        uint32_t a1 = 0;
        for (int s = 0; s < 4; s++) {
            build_station(W, C, s, c % NSTATES, step);
            c /= NSTATES;
            a1 |= (uint32_t)(a % 3) << (8 * s);
            a /= 3;
        }
        uint32_t pend = 0;
        if (color) {
            Tables T = W.tabs();
            const int tcode = tc_make(8, 0, 3);
            const int slot = slot_new(W.E, T, tcode);
            pend = 1u | ((uint32_t)slot << 1) | ((uint32_t)tcode << 9) | ((uint32_t)color << 22);
        }
        out[0]++;
        if (!both<G>(W, C, a1, pend, ev) && !out[1]++)
            snprintf(msg, (size_t)msg_len, "G %d stations %d actions %d colour %d: the lane groups differ from the sequence",
                     G, code, acts, color);
    }
}

void put_events(const Events& ev, int64_t* out) {
    out[0] = ev.two_stations; out[1] = ev.order_by_two;
    for (int s = 0; s < 4; s++) out[2 + s] = ev.drop_to[s];
    out[6] = ev.drop_lost;
}

template <int G>
void replay_g(int envs, int steps, int num_orders, int pkg_cap, uint64_t seed, int64_t* out, char* msg, int msg_len,
              Events& ev) {
    static double lut[RLUT_SIZE];
    const double w[NW] = {100.0, 10.0, -0.1, 1.0, 5.0, -1.0, 2.0, -0.1, 10.0, -5.0, 5.0, 1.0, -2.0, 20.0, 2.0, -1.0};
    build_reward_lut(w, 10, lut);
    const Cfg C = make_cfg(pkg_cap, lut);
    const int nact[NA] = {3, 8, 3, 3, 3, 3, 3, 3};
    for (int e = 0; e < envs; e++) {
        Lcg ga{seed * 1000003ull + (uint64_t)e}, gr_ref{seed + 77ull * (uint64_t)e}, gr_k = gr_ref;
        // R: the plain step.  S: the step in K's schedule (the AGV's drop deferred to K), K's words
        // on the lane groups between the steps.
        World R, S;
        memset(&R, 0, sizeof(R));
        memset(&S, 0, sizeof(S));
        reset_world(R, C, num_orders, gr_ref);
        reset_world(S, C, num_orders, gr_k);
        Tables TR = R.tabs(), TS = S.tabs();
        Lanes<G> lanes;
        lanes.load(S.E);
        for (int k = 0; k < steps; k++) {
            int act[NA];
            for (int a = 0; a < NA; a++) act[a] = (int)ga.next((uint32_t)nact[a]);
            uint32_t res_ref[NA];
            double rew[NA];
            const int tp0 = R.E.total_packaged(), nc0 = R.E.ncompleted();
            env_step<true>(R.E, TR, C, act, nullptr, res_ref, rew);
            // every other agent of the step on S (they leave K's words alone)
            uint32_t res[NA], pend = 0;
            int mv = 0, s0 = -1, s1 = -1;
            res[0] = pickup_execute(S.E, TS, C, act[0]);
            res[1] = agv_execute<true>(S.E, TS, C, act[1], &mv, &pend);
            if (mv) S.E.set_loc(mv);
            res[2] = machine_execute<0>(S.E, TS, act[2], &s0);
            res[3] = machine_execute<1>(S.E, TS, act[3], &s1);
            machines_run(S.E, TS, C, s0, s1);
            const uint32_t a1 = (uint32_t)act[4] | ((uint32_t)act[5] << 8) | ((uint32_t)act[6] << 16) | ((uint32_t)act[7] << 24);
            // K's step: the sequence on a copy (it counts the events and is compared too), the lanes on S
            World Q = S;
            bool ok = lanes.store(Q.E);
            const KOut rq = k_step_ref(Q, C, a1, pend, ev);
            const KOut rl = lanes.step(S, C, a1, pend);
            ok = ok && lanes.store(S.E);
            ok = ok && memcmp(Q.E.w, S.E.w, sizeof(Q.E.w)) == 0 && same_tables(Q, S);
            ok = ok && memcmp(rq.r, rl.r, sizeof(rq.r)) == 0 && rq.gs == rl.gs;
            // and against the plain step: state, results, the step's counts, the live tables
            ok = ok && memcmp(R.E.w, S.E.w, sizeof(R.E.w)) == 0;
            for (int a = 0; a < 4; a++) ok = ok && (res_ref[a] & 0xFFu) == (res[a] & 0xFFu);
            for (int q = 0; q < 4; q++) ok = ok && rl.r[q] == ((res_ref[4 + q] & 0xFFu) | ((uint32_t)act[4 + q] << 8));
            ok = ok && rl.gs == ((uint32_t)(R.E.ncompleted() - nc0) | ((uint32_t)(R.E.total_packaged() - tp0) << 16));
            const int nslot = R.E.slot_next(), carry = R.E.carry();
            ok = ok && memcmp(R.orders, S.orders, 4u * (size_t)num_orders) == 0 && memcmp(R.scode, S.scode, 2u * (size_t)nslot) == 0;
            for (int s = 0; s < nslot; s++) ok = ok && (s == carry || R.snext[s] == S.snext[s]) && R.scstep[s] == S.scstep[s];
            out[0]++;
            if (!ok && !out[1]++)
                snprintf(msg, (size_t)msg_len, "G %d env %d step %d (orders %d): the lane groups differ", G, e, k, num_orders);
            const int nord = R.E.norders();
            const bool done = (R.E.ncompleted() == nord && nord > 0 && R.E.next_order() == nord) || R.E.step() >= C.max_steps;
            R.E.set_step(R.E.step() + 1);
            S.E.set_step(S.E.step() + 1);
            for (int g = 0; g < G; g++) lanes.L[g].set_step(lanes.L[g].step() + 1);
            if (done) {
                reset_world(R, C, nord, gr_ref);
                reset_world(S, C, nord, gr_k);
                // the wave's own reset of its lanes against a fresh load
                Lanes<G> fresh;
                fresh.load(S.E);
                for (int g = 0; g < G; g++) {
                    pack_lane_clear<G>(lanes.L[g]);
                    if (memcmp(lanes.L[g].w, fresh.L[g].w, sizeof(fresh.L[g].w)) != 0 && !out[1]++)
                        snprintf(msg, (size_t)msg_len, "G %d env %d step %d: reset of lane group %d", G, e, k, g);
                }
                out[2]++;
            }
        }
    }
}

}  // namespace

extern "C" {

// (a) constructed: every combination of the four stations' states (build_station) x their actions
// x no drop / a drop of each colour, at pkg_cap 6.  out: cases, mismatches, then the events
// [two_stations, order_by_two, drop_to[0..3], drop_lost].  msg: the first mismatch.
void lanes_sweep(int groups, int64_t* out, char* msg, int msg_len) {
    for (int i = 0; i < 9; i++) out[i] = 0;
    msg[0] = 0;
    Events ev;
    memset(&ev, 0, sizeof(ev));
    if (groups == 4) sweep_g<4>(out, msg, msg_len, ev);
    else if (groups == 2) sweep_g<2>(out, msg, msg_len, ev);
    else sweep_g<1>(out, msg, msg_len, ev);
    put_events(ev, out + 2);
}

// (b) `envs` envs x `steps` steps of uniform-random actions with auto-reset.  out: env-steps
// compared, mismatches, resets, then the events as above.
void lanes_replay(int groups, int envs, int steps, int num_orders, int pkg_cap, uint64_t seed, int64_t* out, char* msg,
                  int msg_len) {
    for (int i = 0; i < 10; i++) out[i] = 0;
    msg[0] = 0;
    Events ev;
    memset(&ev, 0, sizeof(ev));
    if (groups == 4) replay_g<4>(envs, steps, num_orders, pkg_cap, seed, out, msg, msg_len, ev);
    else if (groups == 2) replay_g<2>(envs, steps, num_orders, pkg_cap, seed, out, msg, msg_len, ev);
    else replay_g<1>(envs, steps, num_orders, pkg_cap, seed, out, msg, msg_len, ev);
    put_events(ev, out + 3);
}

}  // extern "C"

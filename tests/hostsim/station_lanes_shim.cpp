// station_lanes_shim.cpp — TEST-ONLY host build of the packaging wave's lane-group form
// (multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h: pack_lane_*, k_step_ag's K wave) for
// tests/test_station_lanes_host.py.  The G lanes of an env run one after another here; the
// reference is the S = 0..3 sequence K ran before (pack_due / pack_complete<0..3>, agv_pack_drop,
// pack_execute / pack_finish<0..3>) on one Env.
#include "replay.h"

namespace {

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
        const int st = pkg_station(E, C, pend_color(pend));
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
    return lanes.store(B.E) && same_world(A, B) && memcmp(ra.r, rb.r, sizeof(ra.r)) == 0 && ra.gs == rb.gs;
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
void sweep_g(int64_t* out, Mismatch& bad, Events& ev) {
    Cfg C = default_cfg();
    C.pkg_cap = 6;
    const int step = 17;
    for (int code = 0; code < NSTATES * NSTATES * NSTATES * NSTATES; code++)
    for (int acts = 0; acts < 81; acts++)
    for (int color = 0; color < 4; color++) {   // 0: no drop
        World W;
        poison_world(W);
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
            pend = pend_make(slot, tcode, color);
        }
        out[0]++;
        bad.check(both<G>(W, C, a1, pend, ev), "G %d stations %d actions %d colour %d: the lane groups differ from the sequence",
                  G, code, acts, color);
    }
}

void put_events(const Events& ev, int64_t* out) {
    out[0] = ev.two_stations; out[1] = ev.order_by_two;
    for (int s = 0; s < 4; s++) out[2 + s] = ev.drop_to[s];
    out[6] = ev.drop_lost;
}

// S's step in K's schedule (the AGV's drop deferred to K), K's words on the lane groups between
// the steps
template <int G>
struct KSchedule {
    static constexpr int AHEAD = 0;
    const Cfg& C;
    Events& ev;
    Lanes<G> lanes;

    void begin(World& S) { lanes.load(S.E); }

    bool step(Step& st, World& S) {
        Tables TS = S.tabs();
        const int* act = st.act;
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
        ok = ok && lanes.store(S.E) && same_world(Q, S);
        ok = ok && memcmp(rq.r, rl.r, sizeof(rq.r)) == 0 && rq.gs == rl.gs;
        // and against the plain step: results and the step's counts (same_live has the rest)
        for (int a = 0; a < 4; a++) ok = ok && (st.res_ref[a] & 0xFFu) == (res[a] & 0xFFu);
        for (int q = 0; q < 4; q++) ok = ok && rl.r[q] == ((st.res_ref[4 + q] & 0xFFu) | ((uint32_t)act[4 + q] << 8));
        const Env &R0 = st.R0.E, &R = st.R.E;
        ok = ok && rl.gs == ((uint32_t)(R.ncompleted() - R0.ncompleted()) | ((uint32_t)(R.total_packaged() - R0.total_packaged()) << 16));
        return ok;
    }

    void end_step(const Step& st, World& S, bool done, Mismatch& bad) {
        for (int g = 0; g < G; g++) lanes.L[g].set_step(lanes.L[g].step() + 1);
        if (!done) return;
        // the wave's own reset of its lanes against a fresh load
        Lanes<G> fresh;
        fresh.load(S.E);
        for (int g = 0; g < G; g++) {
            pack_lane_clear<G>(lanes.L[g]);
            bad.check(memcmp(lanes.L[g].w, fresh.L[g].w, sizeof(fresh.L[g].w)) == 0, "G %d env %d step %d: reset of lane group %d",
                      G, st.env, st.k, g);
        }
    }
};

template <int G>
Replayed replay_g(int envs, int steps, int num_orders, int pkg_cap, uint64_t seed, Mismatch& bad, Events& ev) {
    Cfg C = default_cfg();
    C.pkg_cap = pkg_cap;
    KSchedule<G> m{C, ev};
    char what[48];
    snprintf(what, sizeof(what), "the lane groups differ (G %d)", G);
    return replay(C, envs, steps, num_orders, seed, m, bad, what);
}

}  // namespace

extern "C" {

// (a) constructed: every combination of the four stations' states (build_station) x their actions
// x no drop / a drop of each colour, at pkg_cap 6.  out: cases, mismatches, then the events
// [two_stations, order_by_two, drop_to[0..3], drop_lost].  msg: the first mismatch.
void lanes_sweep(int groups, int64_t* out, char* msg, int msg_len) {
    for (int i = 0; i < 9; i++) out[i] = 0;
    Mismatch bad(out + 1, msg, msg_len);
    Events ev;
    memset(&ev, 0, sizeof(ev));
    if (groups == 4) sweep_g<4>(out, bad, ev);
    else if (groups == 2) sweep_g<2>(out, bad, ev);
    else sweep_g<1>(out, bad, ev);
    put_events(ev, out + 2);
}

// (b) `envs` envs x `steps` steps of uniform-random actions with auto-reset, every env-step against
// the sequence and against the plain step.  out: env-steps compared, mismatches, resets, then the
// events as above.
void lanes_replay(int groups, int envs, int steps, int num_orders, int pkg_cap, uint64_t seed, int64_t* out, char* msg,
                  int msg_len) {
    for (int i = 0; i < 10; i++) out[i] = 0;
    Mismatch bad(out + 1, msg, msg_len);
    Events ev;
    memset(&ev, 0, sizeof(ev));
    const Replayed n = groups == 4   ? replay_g<4>(envs, steps, num_orders, pkg_cap, seed, bad, ev)
                       : groups == 2 ? replay_g<2>(envs, steps, num_orders, pkg_cap, seed, bad, ev)
                                     : replay_g<1>(envs, steps, num_orders, pkg_cap, seed, bad, ev);
    out[0] = n.compared;
    out[2] = n.resets;
    put_events(ev, out + 3);
}

}  // extern "C"


// machine_lanes_shim.cpp — TEST-ONLY host build of the AM wave's lane-group form
// (multi-agent-rl-for-fjsp_amd/csrc/fjsp_env.h: mach_lane_*, k_step_ag's AM wave) for
// tests/test_machine_lanes_host.py.  The lanes of an env run one after another here; the reference
// is the sequence AM ran before on one Env: machine_execute<0>, machine_execute<1>,
// machines_run<true>.  groups 4 and 2: machine g on lane group g < 2 (the other groups idle);
// groups 1: the sequence itself with the queue fronts' successors known ahead (next_known).
#include "replay.h"

namespace {

// what the inputs contain, counted on the sequence alone
struct Events {
    int64_t both_start, start_signal, both_signal, both_done, done_same_order, overwrite, handover_changed, starts, signals, dones;
};

struct MOut {   // what AM hands on after the machines besides its state words
    uint32_t r[2];    // result | action << 8 per machine
    uint32_t p2[4];   // post 2: W9..W12 after the machines' actions
};

constexpr uint32_t POISON = 0xDEADBEEFu;

// the queue fronts' successors as AM reads them at the top of the step, before the AGV's drop
struct Ahead { int pl, pn; };
Ahead ahead(const Env& E, const Tables& T, int lq) {
    Ahead a{E.ll(lq), NIL};
    if (a.pl >= 2) a.pn = T.snext[E.lh(lq)];
    return a;
}
int known(bool fresh, const Ahead& a, const Env& E, int lq) { return fresh ? -1 : a.pl >= 2 ? a.pn : E.lt(lq); }

// the machines of one step as the sequence on one Env (k_step_ag's AM wave before the lane groups):
// nk0 / nk1 as AM passes them (-1: read the table)
MOut machines_ref(World& W, const Cfg& C, int act2, int act3, int nk0, int nk1, Events* ev) {
    Env& E = W.E;
    Tables T = W.tabs();
    int s0 = -1, s1 = -1;
    MOut out;
    out.r[0] = (machine_execute<0>(E, T, act2, &s0, nk0) & 0xFFu) | ((uint32_t)act2 << 8);
    out.r[1] = (machine_execute<1>(E, T, act3, &s1, nk1) & 0xFFu) | ((uint32_t)act3 << 8);
    for (int i = 0; i < 4; i++) out.p2[i] = E.w[9 + i];
    if (ev) {
        const int step = E.step();
        const bool due0 = E.m_busy(0) && E.m_next(0) == step, due1 = E.m_busy(1) && E.m_next(1) == step;
        const bool go0 = (out.r[0] & 2u) != 0, go1 = (out.r[1] & 2u) != 0, sg0 = (out.r[0] & 4u) != 0, sg1 = (out.r[1] & 4u) != 0;
        ev->starts += go0 + go1; ev->signals += sg0 + sg1; ev->dones += due0 + due1;
        ev->both_start += go0 && go1;
        ev->start_signal += (go0 && sg1) || (sg0 && go1);
        ev->both_signal += sg0 && sg1;
        ev->both_done += due0 && due1;
        ev->done_same_order += due0 && due1 && tc_order(E.m_code(0)) == tc_order(E.m_code(1));
        ev->overwrite += (s0 >= 0 && E.m_cur(0) != NIL) || (s1 >= 0 && E.m_cur(1) != NIL);
    }
    machines_run<true>(E, T, C, s0, s1);
    if (E.ll(L_M0Q) > 127 || E.ll(L_M1Q) > 127) E.flag(ST_OBS_OVERFLOW | ST_DIVERGED);
    return out;
}

// the env's two machine lanes: group 0 is the env's own Env less machine 1 (whose words are
// poisoned there: nothing may read them), group 1 holds machine 1 in slot 0
struct Lanes {
    Env M1;
    void load(Env& E) {
        for (int i = 0; i < NSTATE; i++) M1.w[i] = 0u;
        mach_lane_load(M1, 1, [&](int i) { return E.w[i]; });
        M1.w[0] = E.w[0];   // its copy of W0: the step counter and the reset decision
        E.w[18] = POISON;
        E.w[19] = (E.w[19] & 0xFFFFu) | (POISON << 16);
    }
    // group 0 gets its words of P's result (the whole Env here), group 1 its two list words
    void apply(Env& E, const Env& Q) {
        E = Q;
        M1.w[0] = (M1.w[0] & 0x00FFFFFFu) | (Q.w[0] & 0xFF000000u);   // next_order
        M1.w[7 + L_M0Q] = Q.w[7 + L_M1Q];
        M1.w[7 + L_M0R] = Q.w[7 + L_M1R];
        hide(E);
    }
    static void hide(Env& E) { E.w[7 + L_M1Q] = POISON; E.w[7 + L_M1R] = POISON; E.w[18] = POISON; }
    // the hand-over of a fresh step: machine 1's lists after group 0's AGV
    bool handover(Env& E) {
        const bool changed = M1.w[7 + L_M0Q] != E.w[7 + L_M1Q] || M1.w[7 + L_M0R] != E.w[7 + L_M1R];
        M1.w[0] = E.w[0];
        M1.w[7 + L_M0Q] = E.w[7 + L_M1Q];
        M1.w[7 + L_M0R] = E.w[7 + L_M1R];
        hide(E);
        return changed;
    }
    MOut machines(World& W, const Cfg& C, int act2, int act3, int nk0, int nk1) {
        Tables T = W.tabs();
        Env* L[2] = {&W.E, &M1};
        const int act[2] = {act2, act3}, nk[2] = {nk0, nk1}, ptk[2] = {C.ptk_small, C.ptk_big};
        int s[2] = {-1, -1};
        MOut out;
        for (int g = 0; g < 2; g++) out.r[g] = (machine_execute<0>(*L[g], T, act[g], &s[g], nk[g]) & 0xFFu) | ((uint32_t)act[g] << 8);
        for (int g = 0; g < 2; g++) { out.p2[2 * g] = L[g]->w[7 + L_M0Q]; out.p2[2 * g + 1] = L[g]->w[7 + L_M0R]; }
        for (int g = 0; g < 2; g++) {
            mach_lane_run<true>(*L[g], T, ptk[g], s[g]);
            if (L[g]->ll(L_M0Q) > 127) L[g]->flag(ST_OBS_OVERFLOW | ST_DIVERGED);
        }
        return out;
    }
    // the env's words as the launch epilogue stores them and the emit waves see them
    Env merged(const Env& E) const {
        Env R = E;
        R.w[7 + L_M1Q] = M1.w[7 + L_M0Q];
        R.w[7 + L_M1R] = M1.w[7 + L_M0R];
        R.w[18] = M1.w[17];
        R.w[19] = (E.w[19] & 0xFFFFu) | (M1.w[19] << 16);
        R.w[2] |= M1.w[2];
        return R;
    }
};

// one machines' step of both forms from the same state
bool both(const World& W, const Cfg& C, int groups, int act2, int act3, int drop, Events& ev) {
    World A = W, B = W;
    Tables TA = A.tabs(), TB = B.tabs();
    // top of the step: the fronts' successors, then P's AGV result (a drop onto a queue)
    const Ahead a0 = ahead(W.E, TA, L_M0Q), a1 = ahead(W.E, TA, L_M1Q);
    auto agv = [&](World& X, const Tables& T) {
        if (drop) {
            const int s = slot_new(X.E, T, tc_make(9, 0, 2));
            list_push_dyn<0x3Fu>(X.E, T, drop == 1 ? L_M0Q : L_M1Q, s);
        }
    };
    agv(A, TA);
    const MOut ra = machines_ref(A, C, act2, act3, -1, -1, &ev);   // the plain sequence reads the table
    MOut rb;
    if (groups == 1) {
        agv(B, TB);
        rb = machines_ref(B, C, act2, act3, known(false, a0, B.E, L_M0Q), known(false, a1, B.E, L_M1Q), nullptr);
    } else {
        Lanes lanes;
        lanes.load(B.E);
        World Q = B;   // P's AGV on AM's post
        Q.E.w[18] = 0u;
        agv(Q, TB);
        lanes.apply(B.E, Q.E);
        rb = lanes.machines(B, C, act2, act3, known(false, a0, B.E, L_M0Q), known(false, a1, lanes.M1, L_M0Q));
        B.E = lanes.merged(B.E);
    }
    return same_world(A, B) && memcmp(&ra, &rb, sizeof(ra)) == 0;
}

// constructed state of one machine: 0 empty; 1 one tray queued; 2 three queued; 3 busy, its last
// product due now; 4 busy, not due; 5 idle with a current tray; 6 idle with a current tray and two
// queued; 7 busy, a product due now and another to go, one tray queued
constexpr int NSTATES = 8;
void build_machine(World& W, int m, int state, int step, int order) {
    Tables T = W.tabs();
    Env& E = W.E;
    const int lq = m == 0 ? L_M0Q : L_M1Q;
    const int queued = state == 1 || state == 7 ? 1 : state == 2 ? 3 : state == 6 ? 2 : 0;
    for (int i = 0; i < queued; i++) list_push_dyn<0x3Fu>(E, T, lq, slot_new(E, T, tc_make(4 + 2 * m + (i & 1), 0, 2)));
    if (state >= 3) {   // a tray on the machine: two products of `order` from product 2 m on
        const int code = tc_make(order, 2 * m, 2);
        const int slot = slot_new(E, T, code);
        const bool busy = state == 3 || state == 4 || state == 7;
        E.set_m_grant(m, slot, code, busy);
        E.set_m_k(m, state == 3 ? 1 : state == 7 ? 0 : busy ? 0 : 2);
        if (busy) E.set_m_next(m, state == 4 ? step + 3 : step);
        else E.set_m_prog(m, 1);
    }
}

// S's step in AM's schedule, the machines on the lanes, in launches of `launch` steps.  Between two
// steps S.E is group 0's own Env (machine 1's words poisoned); for the comparison with the plain
// step it holds the words the launch epilogue would store.
struct AMSchedule {
    static constexpr int AHEAD = 0;
    const Cfg& C;
    const int groups, launch;
    Events& ev;
    int64_t& fresh_steps;
    Lanes lanes;
    Env G0;   // group 0's Env while S.E holds the merged words
    bool fresh;

    void begin(World&) { fresh = true; memset(&lanes, 0, sizeof(lanes)); }

    bool step(Step& st, World& S) {
        Tables TS = S.tabs();
        const int* act = st.act;
        if (st.k % launch == 0) {   // a launch starts: both groups load their words
            if (st.k > 0 && groups > 1) S.E = lanes.merged(S.E);
            if (groups > 1) {
                Env full = S.E;
                lanes.load(S.E);
                S.E.w[7 + L_M1Q] = full.w[7 + L_M1Q];   // group 0 loads the whole env: its AGV of
                S.E.w[7 + L_M1R] = full.w[7 + L_M1R];   // this step needs machine 1's lists
            }
            fresh = true;
        }
        // the events, on the plain sequence: the machines of a copy of R after its pickup and AGV
        {
            World Q = st.R0;
            Tables TQ = Q.tabs();
            int mv = 0;
            pickup_execute(Q.E, TQ, C, act[0]);
            agv_execute(Q.E, TQ, C, act[1], &mv);
            machines_ref(Q, C, act[2], act[3], -1, -1, &ev);
        }
        // S: the top of the step, then the pickup and the AGV (fresh: on group 0 itself, with the
        // hand-over; else P's, on AM's post), the machines, the packaging stations
        Env& E0 = S.E;
        const Ahead a0 = ahead(E0, TS, L_M0Q);
        const Ahead a1 = groups > 1 ? ahead(lanes.M1, TS, L_M0Q) : ahead(E0, TS, L_M1Q);
        uint32_t pend = 0;
        int mv = 0;
        if (groups > 1 && !fresh) {
            World Q = S;
            Q.E = lanes.merged(S.E);
            Tables TQ = Q.tabs();   // Q's own copy of the tables
            pickup_execute(Q.E, TQ, C, act[0]);
            agv_execute<true>(Q.E, TQ, C, act[1], &mv, &pend);
            if (mv) Q.E.set_loc(mv);
            if (pend) agv_pack_drop(Q.E, TQ, C, pend);
            const uint32_t w17 = S.E.w[17], w19 = S.E.w[19];
            memcpy(S.orders, Q.orders, sizeof(S.orders)); memcpy(S.scode, Q.scode, sizeof(S.scode));
            memcpy(S.snext, Q.snext, sizeof(S.snext)); memcpy(S.scstep, Q.scstep, sizeof(S.scstep));
            Q.E.w[2] &= ~lanes.M1.w[2] | S.E.w[2];   // group 1's status bits stay its own
            lanes.apply(S.E, Q.E);
            S.E.w[17] = w17; S.E.w[19] = w19;
        } else {
            pickup_execute(E0, TS, C, act[0]);
            agv_execute<true>(E0, TS, C, act[1], &mv, &pend);
            if (mv) E0.set_loc(mv);
            if (pend) agv_pack_drop(E0, TS, C, pend);
            if (groups > 1) {
                ev.handover_changed += lanes.handover(E0);
                fresh_steps++;
            }
        }
        MOut rm;
        if (groups > 1)
            rm = lanes.machines(S, C, act[2], act[3], known(fresh, a0, E0, L_M0Q), known(fresh, a1, lanes.M1, L_M0Q));
        else
            rm = machines_ref(S, C, act[2], act[3], known(fresh, a0, E0, L_M0Q), known(fresh, a1, E0, L_M1Q), nullptr);
        {   // the packaging stations, as the plain step runs them
            int sp[4] = {0, 0, 0, 0}, orders_done = 0;
            pack_execute<0>(E0, act[4], &sp[0]); pack_execute<1>(E0, act[5], &sp[1]);
            pack_execute<2>(E0, act[6], &sp[2]); pack_execute<3>(E0, act[7], &sp[3]);
            const int step = E0.step();
            const bool d0 = pack_due<0>(E0, TS, step), d1 = pack_due<1>(E0, TS, step);
            const bool d2 = pack_due<2>(E0, TS, step), d3 = pack_due<3>(E0, TS, step);
            pack_run<0>(E0, TS, C, sp[0], d0, &orders_done); pack_run<1>(E0, TS, C, sp[1], d1, &orders_done);
            pack_run<2>(E0, TS, C, sp[2], d2, &orders_done); pack_run<3>(E0, TS, C, sp[3], d3, &orders_done);
            E0.set_ncompleted(E0.ncompleted() + orders_done);
        }
        bool ok = groups == 1 || lanes.M1.w[0] == S.E.w[0];
        ok = ok && rm.r[0] == ((st.res_ref[2] & 0xFFu) | ((uint32_t)act[2] << 8)) &&
             rm.r[1] == ((st.res_ref[3] & 0xFFu) | ((uint32_t)act[3] << 8));
        fresh = false;
        if (groups > 1) {   // same_live reads the merged words
            G0 = S.E;
            S.E = lanes.merged(G0);
        }
        return ok;
    }

    void end_step(const Step& st, World& S, bool done, Mismatch& bad) {
        lanes.M1.set_step(lanes.M1.step() + 1);
        if (done) {
            fresh = true;
            if (groups == 1) return;
            // group 1's own reset of its lane against a fresh load
            Env full = S.E;
            Lanes fresh_lanes;
            fresh_lanes.load(full);
            mach_lane_clear(lanes.M1);
            lanes.M1.set_norders(S.E.norders());
            bad.check(memcmp(lanes.M1.w, fresh_lanes.M1.w, sizeof(lanes.M1.w)) == 0, "groups %d env %d step %d: reset of lane group 1",
                      groups, st.env, st.k);
        } else if (groups > 1) {
            G0.set_step(G0.step() + 1);
            S.E = G0;
        }
    }
};

}  // namespace

extern "C" {

// (a) constructed: both machines' states x their actions x no drop / a drop onto either queue x
// the trays on the machines of one order or of two.  out: cases, mismatches, then the events
// [both_start, start_signal, both_signal, both_done, done_same_order, overwrite].
void mlanes_sweep(int groups, int64_t* out, char* msg, int msg_len) {
    for (int i = 0; i < 8; i++) out[i] = 0;
    Mismatch bad(out + 1, msg, msg_len);
    Events ev;
    memset(&ev, 0, sizeof(ev));
    const Cfg C = default_cfg();
    const int step = 17;
    for (int st0 = 0; st0 < NSTATES; st0++)
    for (int st1 = 0; st1 < NSTATES; st1++)
    for (int acts = 0; acts < 9; acts++)
    for (int drop = 0; drop < 3; drop++)
    for (int same = 0; same < 2; same++) {
        World W;
        poison_world(W);
        env_clear(W.E, C);
        W.E.set_norders(10);
        W.E.set_step(step);
        for (int o = 0; o < 10; o++) W.orders[o] = ow_make(4, 1 + o % 3, 1 + o % 3);
        build_machine(W, 0, st0, step, 0);
        build_machine(W, 1, st1, step, same ? 0 : 1);
        out[0]++;
        bad.check(both(W, C, groups, acts % 3, acts / 3, drop, ev),
                  "groups %d machines %d / %d actions %d / %d drop %d same order %d: the lanes differ from the sequence",
                  groups, st0, st1, acts % 3, acts / 3, drop, same);
    }
    out[2] = ev.both_start; out[3] = ev.start_signal; out[4] = ev.both_signal; out[5] = ev.both_done;
    out[6] = ev.done_same_order; out[7] = ev.overwrite;
}

// (b) `envs` envs x `steps` steps of uniform-random actions with auto-reset, in launches of `launch`
// steps (a launch's first step, and the step after a reset, run the pickup and the AGV on group 0 and
// hand machine 1's lists over).  out: env-steps compared, mismatches, resets, fresh steps, then the
// events [both_start, start_signal, both_signal, both_done, done_same_order, overwrite,
// handover_changed, starts, signals, products done].
void mlanes_replay(int groups, int envs, int steps, int launch, int num_orders, uint64_t seed, int64_t* out, char* msg,
                   int msg_len) {
    for (int i = 0; i < 14; i++) out[i] = 0;
    Mismatch bad(out + 1, msg, msg_len);
    Events ev;
    memset(&ev, 0, sizeof(ev));
    const Cfg C = default_cfg();
    AMSchedule m{C, groups, launch, ev, out[3]};
    char what[64];
    snprintf(what, sizeof(what), "the lanes differ from the plain step (groups %d)", groups);
    const Replayed n = replay(C, envs, steps, num_orders, seed, m, bad, what);
    out[0] = n.compared;
    out[2] = n.resets;
    out[4] = ev.both_start; out[5] = ev.start_signal; out[6] = ev.both_signal; out[7] = ev.both_done;
    out[8] = ev.done_same_order; out[9] = ev.overwrite; out[10] = ev.handover_changed;
    out[11] = ev.starts; out[12] = ev.signals; out[13] = ev.dones;
}

}  // extern "C"


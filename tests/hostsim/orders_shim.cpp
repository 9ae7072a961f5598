// orders_shim.cpp — TEST-ONLY host build of fjsp_orders.h's put_orders_env (the per-env work of
// fjsp_put_orders) with the state machine of fjsp_env.h, for tests/test_orders_host.py: replays of
// the reference's recorded runs on caller-chosen order books and with orders arriving during the
// episode (tests/golden/orders.npz), and single calls on a caller-held world (rejections, appends).
#include "world.h"

#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_orders.h"

namespace {

void put_obs(Env& E, const Cfg& C, int32_t* i32, int8_t* i8, float* f32, int8_t* mk) {
    Obs o;
    memset(&o, 0, sizeof(o));
    ObsSink sink{o};
    observe(E, C, sink);
    memcpy(i32, o.i32, sizeof(o.i32));
    memcpy(i8, o.i8, sizeof(o.i8));
    memcpy(f32, o.f32, sizeof(o.f32));
    memcpy(mk, o.mask, sizeof(o.mask));
}

}  // namespace

extern "C" {

// what a replay reads and writes (ctypes.Structure OrdersRun in tests/test_orders_host.py)
struct OrdersRun {
    const uint32_t* book;      // [K] caller's order words
    const int64_t* arrivals;   // [n_arr][7]: step, argument, products, type, colour, id, arrival time
    const uint8_t* actions;    // [T][8]
    int32_t K, n_arr, T, pad;
    int32_t* init_i32; int8_t* init_i8; float* init_f32; int8_t* init_mk;        // after the reset
    int32_t* arr_i32; int8_t* arr_i8; float* arr_f32; int8_t* arr_mk;            // [n_arr][..] after each arrival
    int32_t* arr_id;                                                             // [n_arr] the id each order got
    int32_t* i32; int8_t* i8; float* f32; int8_t* mk;                            // [T][..]
    double* rew; uint8_t* term; uint8_t* trunc; uint32_t* res; double* sim_time; int32_t* oc; int32_t* pk;
    uint32_t status;           // status bits ORed over the run
    int32_t rejected;          // calls put_orders_env refused
};

// One recorded run: the book through put_orders_env(append = 0) on a dirty world, the arrivals
// through put_orders_env(append = 1) before their steps, the recorded actions through env_step.
void orders_replay(OrdersRun* r) {
    const Cfg C = default_cfg();
    BookWorld W;
    memset(&W, 0xA5, sizeof(W));   // a reset must not depend on what the env held
    W.E.w[3] = 0x12345u;
    W.pgw = 1u;
    Tables Tb = W.tabs();
    r->status = 0;
    r->rejected = 0;
    r->rejected += !put_orders_env(W.E, Tb, C, r->book, 1, r->K, r->K, 0, &W.pgw);
    r->rejected += W.E.w[3] != 0x12345u || W.pgw != 0u;
    put_obs(W.E, C, r->init_i32, r->init_i8, r->init_f32, r->init_mk);
    int a = 0;
    for (int t = 0; t < r->T; t++) {
        for (; a < r->n_arr && r->arrivals[7 * a] == t; a++) {
            const int64_t* v = r->arrivals + 7 * a;
            const uint32_t word = (uint32_t)v[2] | ((uint32_t)v[3] << 4) | ((uint32_t)v[4] << 6);
            r->arr_id[a] = W.E.norders();
            r->rejected += !put_orders_env(W.E, Tb, C, &word, 1, 1, 1, 1, &W.pgw);
            put_obs(W.E, C, r->arr_i32 + NI32 * a, r->arr_i8 + NI8 * a, r->arr_f32 + NF32 * a, r->arr_mk + NMASK * a);
        }
        int act[NA];
        for (int k = 0; k < NA; k++) act[k] = r->actions[t * NA + k];
        env_step<true>(W.E, Tb, C, act, nullptr, r->res + NA * t, r->rew + NA * t);
        put_obs(W.E, C, r->i32 + NI32 * t, r->i8 + NI8 * t, r->f32 + NF32 * t, r->mk + NMASK * t);
        r->term[t] = all_done(W.E);
        r->trunc[t] = W.E.step() >= C.max_steps;
        r->oc[t] = W.E.ncompleted();
        r->pk[t] = W.E.total_packaged();
        r->sim_time[t] = (double)(W.E.step() + 1) * (double)C.step_size;
        r->status |= W.E.status();
        W.E.set_step(W.E.step() + 1);
    }
}

// ---- single calls on a world the caller holds as bytes
int orders_world_bytes(void) { return (int)sizeof(BookWorld); }
// byte offsets of the state words, the pre-draw record and the order table; their counts
void orders_world_layout(int32_t* out) {
    BookWorld W;
    const char* base = (const char*)&W;
    out[0] = (int32_t)((const char*)W.E.w - base);
    out[1] = NSTATE;
    out[2] = (int32_t)((const char*)&W.pgw - base);
    out[3] = (int32_t)((const char*)W.orders - base);
    out[4] = MAX_ORDERS;
}
// put_orders_env on the world: the env's column of a [K][sstride] table starts at src
int orders_put(void* world, const uint32_t* src, int sstride, int K, int count, int append) {
    BookWorld& W = *(BookWorld*)world;
    const Cfg C = default_cfg();
    Tables Tb = W.tabs();
    return put_orders_env(W.E, Tb, C, src, sstride, K, count, append, &W.pgw) ? 1 : 0;
}
// n steps of the built-in heuristic (a state in the middle of an episode); returns the status word
uint32_t orders_world_run(void* world, int n) {
    BookWorld& W = *(BookWorld*)world;
    const Cfg C = default_cfg();
    Tables Tb = W.tabs();
    for (int t = 0; t < n; t++) {
        int act[NA];
        uint32_t res[NA];
        double rew[NA];
        heuristic_actions(W.E, Tb, act);
        env_step<true>(W.E, Tb, C, act, nullptr, res, rew);
        W.E.set_step(W.E.step() + 1);
    }
    return W.E.status();
}

}  // extern "C"

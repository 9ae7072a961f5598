// fjsp_stepdev.h — device side of one env step shared by the step kernels (fjsp_hip.hip) and the
// fused policy + step kernel of the A2C collect (fjsp_policy.hip): the HBM state layout
// (DevState), the per-env MT19937 stream and reset, the observation sinks and step_and_emit
// (FJSPSimulation.step, FJSPSimulation.py:144-242, on the fjsp_env.h state machine).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fjsp_env.h"
#include "fjsp_predraw.h"
#include "fjsp_search.h"
#include "fjsp_stamps.h"
#include "../../include/fjsp.h"

namespace fjsp {

struct DevState {
    uint32_t* words;
    uint32_t* orders;
    uint16_t* scode;
    uint8_t* snext;
    uint16_t* scstep;
    uint32_t* mt;       // [2][n][624] MT rows (live one selected by W3 bit 31)
    uint32_t* nxt;      // [MAX_ORDERS][n] pre-drawn next order tables (W[PGW])
    int n;
};
// Handle words after the state rows ([NWORDS][n] u32 + AUX_WORDS): the fault word (fjsp_faults:
// bit 0 = a bounded hand-off wait gave up) and the bound of those waits (option "spin_cap").
// Not kernel arguments: a pointer or a field more in DevState / Cfg, live through the step loops,
// pushed k_step_ag into SGPR spills (+6 % per step, measured).
// AUX_TEST_STALL: test option "test_stall" (tests/test_gpu_agents.py), see stall_for_test.
constexpr int AUX_WORDS = 4, AUX_FAULT = 0, AUX_SPIN_CAP = 1, AUX_TEST_STALL = 2;
__device__ __forceinline__ uint32_t* aux_words(const DevState& S) { return S.words + (size_t)NWORDS * S.n; }
// Test option "test_stall" = s: the wave that owns a multi-wave workgroup's hand-offs sleeps
// s x 127 x 64 cycles before its first step (called for workgroup 0 only, once per launch), so
// the other waves' bounded waits for its first post give up — the give-up path under test.  One
// scalar load per launch; nothing in the step loops.
__device__ __forceinline__ void stall_for_test(const DevState& S) {
    const uint32_t s = aux_words(S)[AUX_TEST_STALL];
    for (uint32_t i = 0; i < s; i++) __builtin_amdgcn_s_sleep(127);
}

// ---------------------------------------------------------------- load / store of Env
// The register state is the HBM row layout itself (fjsp_env.h, struct Env): 30 coalesced words.
__device__ __forceinline__ void env_load(Env& E, const uint32_t* __restrict__ w, int n, int e) {
#pragma unroll
    for (int i = 0; i < NSTATE; i++) E.w[i] = w[i * n + e];
}
__device__ __forceinline__ void env_store(const Env& E, uint32_t* __restrict__ w, int n, int e) {
#pragma unroll
    for (int i = 0; i < NSTATE; i++) w[i * n + e] = E.w[i];
}
static_assert(NWORDS >= NSTATE, "state buffer rows");

// ---------------------------------------------------------------- MT19937, lazily twisted
// Per-env state: 624 words, env-major (row e = mt + e * 624, 16-byte aligned), so the words a
// lane streams through are contiguous for that lane (lanes of a wave sit at different stream
// positions: a word-major layout would make every load touch 64 rows).
// Cursor word W3 (mtcur_*, fjsp_predraw.h): mti | g.  Words [0, g) of the row already hold the
// current block, [g, 624) still the previous one; mti <= g is the next word to consume.
// Word i of a new block is generated on demand with the same in-place recurrence as numpy's
// sequential twist (mt[i+1] is still old, mt[i+397 mod 624] is new iff i >= 227), so the k-th
// draw equals numpy's k-th draw.
// Standard numpy (key, pos): pos == 624 <-> (mti, g) = (0, 0); pos < 624 <-> (pos, 624).
__device__ inline void mt_seed(uint32_t* __restrict__ mt, int e, uint32_t seed) {
    uint4* row = reinterpret_cast<uint4*>(mt + (size_t)e * MT_N);
    uint32_t x = seed;
    for (int q = 0; q < MT_N / 4; q++) {
        uint32_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = 4 * q + j;
            if (i > 0) x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i;
            v[j] = x;
        }
        row[q] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

// The batched reader of the stream (mt_load, mt_batch_loaded, mt_batch), the order draw (OrderDraw,
// draw_orders) and the pre-draw lane's slices are in fjsp_predraw.h, which also compiles for the
// host.

// MT rows: two per env ([2][N][624]); the row bit of the cursor word W3 selects the live one (the
// other is the pre-draw wave's working copy, see k_step_pipe).  W[PGW] = the pre-draw record
// (pdrec_*, fjsp_predraw.h): 0, or the cursor after the pre-drawn orders, its row and num_orders,
// with the orders in S.nxt.
constexpr int PGW = NSTATE;
static_assert(NWORDS > PGW, "state buffer rows");
__device__ __forceinline__ uint32_t* mt_row(const DevState& S, uint32_t w3, int e) {
    return S.mt + ((size_t)mtcur_row(w3) * S.n + e) * MT_N;
}

// FJSPSimulation.reset body after the optional reseed (FJSPSimulation.py:301-320): clear the
// env and draw num_orders orders from the env's live MT row.  clear_pg: drop a pre-drawn
// next table (it was drawn from the stream position this reset consumes).
__device__ __forceinline__ void env_reset(Env& E, const Tables& T, const Cfg& C, const DevState& S, int e,
                                          int num_orders, bool clear_pg = true) {
    env_clear(E, C);
    E.set_norders(num_orders);
    const uint32_t w3 = (uint32_t)E.mti();
    uint32_t* roww = mt_row(S, w3, e);
    int pos = mtcur_pos(w3), g = mtcur_g(w3);
    OrderDraw d{0, 0, 0, 0, 0u};
    while (d.o < num_orders) {
        uint32_t v[MTB];
        int pa, cnt;
        mt_batch<MTB>(roww, pos, g, v, pa, cnt);
        pos += draw_orders<MTB>(v, pos - pa, cnt, num_orders, d, T.orders, T.stride);
        if (pos == MT_N) { pos = 0; g = 0; }
    }
    E.set_mti((int)mtcur_moved(w3, pos, g));
    if (clear_pg) S.words[(size_t)PGW * S.n + e] = PDREC_NONE;
}

// reset(seed=None) from a pre-drawn table (lane's slots nxt[o * BLOCK]): the same state as
// env_reset, the stream position and live row taken from the pre-draw.
__device__ __forceinline__ void env_reset_predrawn(Env& E, const Tables& T, const Cfg& C, int num_orders,
                                                   uint32_t w3, const uint32_t* nxt) {
    env_clear(E, C);
    E.set_norders(num_orders);
    for (int o = 0; o < num_orders; o++) T.orders[o * T.stride] = nxt[o * BLOCK];
    E.set_mti((int)w3);
}

// Auto-reset inside the step kernels is a cold path (once per ~200 steps), taken in a branch.
// Inlined: a call would need a stack frame in scratch memory (368 B per lane: the by-value
// state and the callee-saved registers), and a kernel that uses scratch pays for its set-up
// on every launch (measured: k_step 12.1 -> 7.9 us per launch in rocprof) and its allocation
// raised every step kernel to 228+ VGPRs (157-233 inlined).
__device__ __forceinline__
Env env_reset_cold(Env E, Tables T, Cfg C, DevState S, int e, int num_orders, bool clear_pg = true) {
    env_reset(E, T, C, S, e, num_orders, clear_pg);
    return E;
}

__device__ __forceinline__ Tables tables_of(const DevState& S, int e) {
    Tables T;
    T.orders = S.orders + e;
    T.scode = S.scode + e;
    T.snext = S.snext + e;
    T.scstep = S.scstep + e;
    T.stride = S.n;
    return T;
}
// a lane's tables in a kernel's LDS staging arrays (element i of the lane at base[i * BLOCK + lane])
__device__ __forceinline__ Tables lds_tables(uint32_t* orders, uint16_t* scode, uint8_t* snext, uint16_t* scstep, int lane) {
    Tables T;
    T.orders = orders + lane;
    T.scode = scode + lane;
    T.snext = snext + lane;
    T.scstep = scstep + lane;
    T.stride = BLOCK;
    return T;
}

// Output byte offsets are 32-bit (the host checks every output slab is < 4 GiB), so the
// stores use the SGPR-base + 32-bit VGPR-offset form instead of 64-bit per-lane addresses.
template <class V>
__device__ __forceinline__ void st32(V* base, uint32_t elem, V v) {
    *reinterpret_cast<V*>(reinterpret_cast<char*>(base) + elem * (uint32_t)sizeof(V)) = v;
}
// a2c feature column of each observation field (a2c.py:137-166: agents in order, keys sorted,
// action_mask dropped); checked against spec.a2c_feature_index by fjsp_a2c_layout's test.
constexpr int NFEAT = 38;
constexpr int8_t FEAT_OF_I32[NI32] = {5, 6, 4, 3, 2, 0, 1, 11, 12, 9, 18, 19, 17, 16, 10, 13, 7, 14, 8, 15};
constexpr int8_t FEAT_OF_I8[NI8] = {20, 22, 23, 25, 26, 28, 29, 31, 32, 34, 35, 37};
constexpr int8_t FEAT_OF_F32[NF32] = {21, 24, 27, 30, 33, 36};

// Sink that stores each observation field as soon as it is computed (fjsp_env.h observe()).
struct StoreSink {
    int32_t* pi32; int8_t* pi8; float* pf32; int8_t* pmk;
    uint32_t t, n, e;
    float* pfeat = nullptr;   // optional a2c features [T][38][N]
    __device__ __forceinline__ void feat(int c, float v) { if (pfeat) st32(pfeat, (t * NFEAT + (uint32_t)c) * n + e, v); }
    __device__ __forceinline__ void i32(int f, int v) {
        if (pi32) st32(pi32, (t * NI32 + (uint32_t)f) * n + e, (int32_t)v);
        feat(FEAT_OF_I32[f], (float)v);
    }
    __device__ __forceinline__ void i8(int f, int v) {
        if (pi8) st32(pi8, (t * NI8 + (uint32_t)f) * n + e, (int8_t)v);
        feat(FEAT_OF_I8[f], (float)(int8_t)v);
    }
    __device__ __forceinline__ void f32(int f, float v) {
        if (pf32) st32(pf32, (t * NF32 + (uint32_t)f) * n + e, v);
        feat(FEAT_OF_F32[f], v);
    }
    __device__ __forceinline__ void mask(int f, int v) { if (pmk) st32(pmk, (t * NMASK + (uint32_t)f) * n + e, (int8_t)v); }
};


// fmix64, the counter RNG of the synthetic actions, is in fjsp_search.h (it compiles for the host too)

// FULL = false: only obs, masks, rewards, term, trunc and status are written (the other
// fjsp_out pointers are never read, so they take no SGPRs in the hot loop).
// HP: nothing, or the held-tray slab u32 [T][3][N] of the HELD instance (fjsp_step_held): a
// trailing pack, so every other instance keeps its arguments and its code; or that slab and the
// pack slab u32 [T][4][N] of the SCHED instance (fjsp_step_sched).
template <bool CANON, bool FULL = true, class... HP>
__device__ __forceinline__ void step_and_emit(Env& E, const Tables& T, const Cfg& C, const DevState& S, int e,
                                              const int* act, const uint8_t* order, int autoreset, const fjsp_out& out,
                                              uint32_t t, HP... held) {
    static_assert(sizeof...(HP) <= 2, "at most the held-tray slab and the pack slab");
    const uint32_t n = (uint32_t)S.n, ue = (uint32_t)e;
    uint32_t res[NA];
    const double g8 = env_advance<CANON>(E, T, C, act, order, res);
    if (out.rewards) {
#pragma unroll
        for (int a = 0; a < NA; a++) st32(out.rewards, (t * NA + (uint32_t)a) * n + ue, g8 + local_reward(C, a, res[a], act[a]));
    }
    if (FULL && out.results) {
#pragma unroll
        for (int a = 0; a < NA; a++) st32(out.results, (t * NA + (uint32_t)a) * n + ue, res[a]);
    }
    FJSP_STAMP(E, 3);
    StoreSink sink{out.obs_i32, out.obs_i8, out.obs_f32, out.masks, t, n, ue};
    observe(E, C, sink);
    FJSP_STAMP(E, 4);
    const int nord = E.norders();
    const auto [all_done, truncated] = episode_end(E, C);
    if (out.term) st32(out.term, t * n + ue, (uint8_t)all_done);
    if (out.trunc) st32(out.trunc, t * n + ue, (uint8_t)truncated);
    if (FULL && out.orders_completed) st32(out.orders_completed, t * n + ue, E.ncompleted());
    if (FULL && out.packaged) st32(out.packaged, t * n + ue, E.total_packaged());
    if (FULL && out.sim_time) st32(out.sim_time, t * n + ue, (double)(E.step() + 1) * (double)C.step_size);
    if (out.status) st32(out.status, t * n + ue, E.status());
    if constexpr (sizeof...(HP) == 1) {   // the state the status is of: after the run, before the reset
        uint32_t* const hp = (held, ...);
        uint32_t hv[3];
        held_words(E, hv);
#pragma unroll
        for (int r = 0; r < 3; r++) st32(hp, (t * 3u + (uint32_t)r) * n + ue, hv[r]);
    }
    if constexpr (sizeof...(HP) == 2) {   // SCHED (fjsp_step_sched): the held words and the pack words
        uint32_t* const hp[2] = {held...};
        uint32_t hv[3], pv[4];
        held_words(E, hv);
        pack_words(E, pv);
#pragma unroll
        for (int r = 0; r < 3; r++) st32(hp[0], (t * 3u + (uint32_t)r) * n + ue, hv[r]);
#pragma unroll
        for (int s = 0; s < 4; s++) st32(hp[1], (t * 4u + (uint32_t)s) * n + ue, pv[s]);
    }
    FJSP_STAMP(E, 5);
    E.set_step(E.step() + 1);
    if (autoreset && (all_done || truncated))
        E = env_reset_cold(E, T, C, S, e, nord);   // reset(seed=None) continues the MT stream
    if (FULL && (out.next_i32 || out.next_i8 || out.next_f32 || out.next_masks || out.feats)) {
        StoreSink nsink{out.next_i32, out.next_i8, out.next_f32, out.next_masks, t, n, ue, out.feats};
        observe(E, C, nsink);
    }
    FJSP_STAMP(E, 6);
}

}  // namespace fjsp

// fjsp_policy.hip: the launch of the fused policy + step kernel (fjsp_a2c_policy_step) over the
// envs [env_begin, env_begin + env_count) (env_begin a multiple of 64); tile_cnt [ceil(n / 64)]
// arrival counters (zero between launches), tile_act [ceil(n / 64)][8][16] words.
int fjsp_internal_policy_step(const float* feats, const int8_t* masks, int32_t n, const float* actor_w,
                              const float* critic_w, const uint64_t* seed, uint32_t env_gid0, uint32_t step,
                              int32_t deterministic, uint8_t* actions, float* values, const fjsp::DevState& S,
                              const fjsp::Cfg& C, const fjsp_out& out, uint32_t* tile_cnt, uint32_t* tile_act,
                              int32_t autoreset, int32_t env_begin, int32_t env_count, hipStream_t stream);

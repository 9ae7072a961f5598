// predraw_shim.cpp — TEST-ONLY host build of fjsp_predraw.h (the lazily twisted MT stream, the
// order draw and the sliced pre-draw lane of k_step_ag's PD wave) for tests/test_predraw_host.py.
// The sliced lane is driven by the schedule the kernel's step loop gives it (pd_refill_step /
// pd_consume_step by the step's parity, the load after them) and compared with the one-shot draw
// of a reset (env_reset's loop, restated here on the same mt_batch / draw_orders) and with the
// sequential generator of hostsim.cpp (mt_next_, bounded).  predraw_san_main.cpp runs the sweep
// as a stand-alone program (the sanitizer build).
#include "hostsim.cpp"

#include <stdio.h>
#include <vector>

#include "../../multi-agent-rl-for-fjsp_amd/csrc/fjsp_predraw.h"

namespace {

struct Row {
    alignas(16) uint32_t w[MT_N];
};

// words [from, to) of the next block, in place: the sequential twist's recurrence, word by word
void advance(uint32_t* s, int from, int to) {
    for (int i = from; i < to; i++) {
        const uint32_t y = (s[i] & 0x80000000u) | (s[(i + 1) % MT_N] & 0x7fffffffu);
        s[i] = s[(i + 397) % MT_N] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
}

// env_reset's loop (fjsp_stepdev.h) on batches of B words: B = MTB is the reset, B = PD_B the
// unsliced draw of the same groups the lane refills
template <int B>
void oneshot(uint32_t* row, int& pos, int& g, int num_orders, uint32_t* orders) {
    OrderDraw d{0, 0, 0, 0, 0u};
    while (d.o < num_orders) {
        uint32_t v[B];
        int pa, cnt;
        mt_batch<B>(row, pos, g, v, pa, cnt);
        pos += draw_orders<B>(v, pos - pa, cnt, num_orders, d, orders, 1);
        if (pos == MT_N) { pos = 0; g = 0; }
    }
}

// generate_order over the sequential generator: key s (a whole block), mti as numpy's pos
void sequential(uint32_t* s, int& mti, int num_orders, uint32_t* orders) {
    for (int o = 0; o < num_orders; o++) {
        const int np = 1 + bounded(s, mti, 8, 15);
        const int ty = 1 + bounded(s, mti, 2, 3);
        const int co = 1 + bounded(s, mti, 2, 3);
        orders[o] = ow_make(np, ty, co);
    }
}

// The lane under the kernel's schedule from step k0 on, the lane promoted in the step before (its
// first load issued there): at most max_slices slices (a load, a refill or a consume each; < 0:
// to completion).  Returns the steps run; *slices = slices run, *ready = the table is complete.
template <bool ALT>
int run_lane(PreDrawLane& L, uint32_t* work, uint32_t* orders, int k0, int max_slices, int* slices, bool* ready) {
    int ns = 0, steps = 0;
    *ready = L.done();
    auto more = [&]() { return max_slices < 0 || ns < max_slices; };
    if (!*ready && more() && L.wants_load()) { L.load(work); ns++; }   // the promotion step's load site
    for (int k = k0; !*ready && more(); k++) {
        steps++;
        if (pd_refill_step<ALT>(k) && L.can_refill() && more()) { L.refill(work); ns++; }
        if (pd_consume_step<ALT>(k) && L.can_consume() && more()) { *ready = L.consume(orders, 1); ns++; }
        if (!*ready && L.wants_load() && more()) { L.load(work); ns++; }
        if (steps > 4 * MT_N) break;   // a lane that stopped moving: reported as not ready
    }
    *slices = ns;
    return steps;
}

struct Check {
    long fails = 0;
    int first = 0;   // code of the first failure
    void want(bool ok, int code) {
        if (!ok) { if (!fails) first = code; fails++; }
    }
};

// One table drawn by the sliced lane from the live row `live` at (pos, g) against the three
// references; returns the steps to readiness.
template <bool ALT>
int check_table(const Row& live, int pos, int g, const Row& key, int mti, int num_orders, int k0, PreDrawLane& L,
                Check& c) {
    Row work = live, r4 = live, r32 = live, ks = key;
    uint32_t got[MAX_ORDERS] = {0}, o4[MAX_ORDERS] = {0}, o32[MAX_ORDERS] = {0}, os[MAX_ORDERS] = {0};
    L.start(num_orders, pos, g);
    int slices;
    bool ready;
    const int steps = run_lane<ALT>(L, work.w, got, k0, -1, &slices, &ready);
    c.want(ready, 1);
    int p4 = pos, g4 = g, p32 = pos, g32 = g, ms = mti;
    oneshot<PD_B>(r4.w, p4, g4, num_orders, o4);
    oneshot<MTB>(r32.w, p32, g32, num_orders, o32);
    sequential(ks.w, ms, num_orders, os);
    c.want(memcmp(got, o4, sizeof(got)) == 0 && memcmp(got, o32, sizeof(got)) == 0 && memcmp(got, os, sizeof(got)) == 0, 2);
    // the same groups unsliced: cursor and row word for word
    c.want(L.pos == p4 && L.g == g4 && memcmp(work.w, r4.w, sizeof(work.w)) == 0, 3);
    // the reset's batches run further ahead in the same block: the same cursor, and the same row
    // once the words between the two g are regenerated
    c.want(L.pos == p32 && L.g <= g32 && (L.g > 0 || g32 == 0), 4);
    Row adv = work;
    advance(adv.w, L.g, g32);
    c.want(memcmp(adv.w, r32.w, sizeof(adv.w)) == 0, 5);
    // the sequential generator: numpy's (key, pos); pos 624 <-> (0, 0)
    if (L.pos == 0 && L.g == 0) {
        c.want(ms == MT_N || (ms == 0 && num_orders == 0), 6);
    } else {
        c.want(ms == L.pos, 6);
        advance(adv.w, g32, MT_N);
    }
    if (!(num_orders == 0 && L.g < MT_N && L.g > 0))   // no draw: the sequential key is still the block before
        c.want(memcmp(adv.w, ks.w, sizeof(adv.w)) == 0, 7);
    return steps;
}

template <bool ALT>
void sweep(const uint32_t* key624, int pos, int g, int num_orders, int with_interruptions, int64_t* out) {
    // live row at (pos, g): g == 624 the key's own block (numpy pos < 624), g == 0 the key before
    // its twist (numpy pos == 624), else words [0, g) of the next block over the key
    Row key, live;
    memcpy(key.w, key624, sizeof(key.w));
    live = key;
    int mti;
    if (g == MT_N) {
        mti = pos;
    } else {
        advance(live.w, 0, g);
        mti = MT_N;   // the next draw twists; then skip the pos words already consumed
        if (pos > 0) {
            for (int i = 0; i < pos; i++) mt_next_(key.w, mti);
        }
    }
    Check c;
    PreDrawLane L;
    int max_steps = 0, points = 0;
    for (int k0 = 0; k0 < 2; k0++) {
        const int steps = check_table<ALT>(live, pos, g, key, mti, num_orders, k0, L, c);
        max_steps = steps > max_steps ? steps : max_steps;
    }
    if (with_interruptions) {
        // a reset before readiness: the sim side draws its table from the live row in one shot and
        // posts the new cursor; the lane drops what it had and starts over on a copy of that row
        Row live2 = live, key2 = key;
        int p2 = pos, g2 = g, m2 = mti;
        uint32_t tmp[MAX_ORDERS];
        oneshot<MTB>(live2.w, p2, g2, num_orders, tmp);
        sequential(key2.w, m2, num_orders, tmp);
        if (g2 == 0) m2 = MT_N;   // (0, 0): the block is used up, key2 is the key before the twist
        for (int k0 = 0; k0 < 2; k0++) {
            for (int s = 1;; s++) {
                Row work = live;
                uint32_t part[MAX_ORDERS];
                L.start(num_orders, pos, g);
                int slices;
                bool ready;
                run_lane<ALT>(L, work.w, part, k0, s, &slices, &ready);
                if (ready || slices < s) break;   // past the last interruption point
                points++;
                // the lane keeps its registers (runs, held words, draw state): start() must drop them
                const int nord = L.nord;
                (void)nord;
                Row keyc = key2;
                int mc = m2;
                {
                    Row work2 = live2, r4 = live2;
                    uint32_t got[MAX_ORDERS] = {0}, o4[MAX_ORDERS] = {0}, os[MAX_ORDERS] = {0};
                    L.start(num_orders, p2, g2);
                    int sl2;
                    bool rdy2;
                    const int steps = run_lane<ALT>(L, work2.w, got, (k0 + s) & 1, -1, &sl2, &rdy2);
                    max_steps = steps > max_steps ? steps : max_steps;
                    c.want(rdy2, 11);
                    int p4 = p2, g4 = g2;
                    oneshot<PD_B>(r4.w, p4, g4, num_orders, o4);
                    sequential(keyc.w, mc, num_orders, os);
                    c.want(memcmp(got, o4, sizeof(got)) == 0 && memcmp(got, os, sizeof(got)) == 0, 12);
                    c.want(L.pos == p4 && L.g == g4 && memcmp(work2.w, r4.w, sizeof(r4.w)) == 0, 13);
                }
            }
        }
    }
    out[0] = c.fails;
    out[1] = c.first;
    out[2] = max_steps;
    out[3] = points;
}

}  // namespace

extern "C" {

// key [624]: a whole MT block (numpy's key); (pos, g): the lazily twisted cursor of the live row
// built from it (see sweep).  out: [0] failed checks, [1] the first one's code, [2] the most steps
// from a lane's first refill step to its table's readiness, [3] interruption points run.
void pd_sweep(const uint32_t* key, int pos, int g, int num_orders, int alternate, int with_interruptions, int64_t* out) {
    if (alternate) sweep<true>(key, pos, g, num_orders, with_interruptions, out);
    else sweep<false>(key, pos, g, num_orders, with_interruptions, out);
}

}  // extern "C"

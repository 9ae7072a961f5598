// fjsp_predraw.h — the lazily twisted MT19937 stream, the order draw and the per-lane pre-draw
// machine of k_step_ag's PD wave, written so that the same source compiles for the device
// (fjsp_stepdev.h) and for the host (tests/hostsim/predraw_shim.cpp, TEST-ONLY).
#pragma once
#include <stdint.h>

#include "fjsp_env.h"

namespace fjsp {

#ifndef __HIP__
// host build: the 16-byte runs stated as four words
struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
#endif

constexpr int MT_N = 624;

// ---------------------------------------------------------------- packed words of the stream
// Each layout is stated here once; kernels and host code go through these functions, or, where a
// call would move a kernel's instructions, spell the same expression from the named constants.
//
// MT cursor word W3: pos (mti, the next word to consume) [0,10) | g (words [0, g) of the row are
// current) [16,26) | live row of the env's two MT rows, bit 31.
constexpr int MTCUR_G_SH = 16, MTCUR_ROW_SH = 31;
constexpr uint32_t MTCUR_IDX_MASK = 0x3FFu, MTCUR_ROW_BIT = 0x80000000u;
FJSP_HD constexpr int mtcur_pos(uint32_t w3) { return (int)(w3 & MTCUR_IDX_MASK); }
FJSP_HD constexpr int mtcur_g(uint32_t w3) { return (int)((w3 >> MTCUR_G_SH) & MTCUR_IDX_MASK); }
FJSP_HD constexpr uint32_t mtcur_row(uint32_t w3) { return w3 >> MTCUR_ROW_SH; }
FJSP_HD constexpr uint32_t mtcur_make(uint32_t pos, uint32_t g, uint32_t row) { return pos | (g << MTCUR_G_SH) | (row << MTCUR_ROW_SH); }
// the cursor moved, the live row kept
FJSP_HD constexpr uint32_t mtcur_moved(uint32_t w3, int pos, int g) {
    return (uint32_t)pos | ((uint32_t)g << MTCUR_G_SH) | (w3 & MTCUR_ROW_BIT);
}
static_assert(MT_N <= (int)MTCUR_IDX_MASK && MTCUR_ROW_BIT == 1u << MTCUR_ROW_SH && (MTCUR_IDX_MASK << MTCUR_G_SH) < MTCUR_ROW_BIT &&
                  MTCUR_IDX_MASK < (1u << MTCUR_G_SH),
              "MT_N fits the cursor's 10-bit fields, which do not overlap");
static_assert(mtcur_pos(mtcur_make(MT_N, 0, 0)) == MT_N && mtcur_g(mtcur_make(MT_N, 0, 0)) == 0 && mtcur_g(mtcur_make(0, MT_N, 1)) == MT_N &&
                  mtcur_pos(mtcur_make(0, MT_N, 1)) == 0 && mtcur_row(mtcur_make(0, 0, 1)) == 1u && mtcur_row(mtcur_make(MT_N, MT_N, 0)) == 0u &&
                  mtcur_moved(mtcur_make(1, 2, 1), 3, 4) == mtcur_make(3, 4, 1),
              "cursor word: decode(encode) at the fields' extremes");
static_assert(mtcur_pos(0x826F0123u) == (int)(0x826F0123u & 0x3FF) && mtcur_g(0x826F0123u) == (int)((0x826F0123u >> 16) & 0x3FF) &&
                  mtcur_row(0x826F0123u) == 0x826F0123u >> 31 &&
                  mtcur_moved(0x826F0123u, 5, 9) == ((uint32_t)5 | ((uint32_t)9 << 16) | (0x826F0123u & 0x80000000u)),
              "the cursor codec equals the hand-spelled expressions it replaces");

// Pre-draw record W[PGW] (fjsp_stepdev.h): 0 = no table, or ready, bit 0 | the cursor after the
// pre-drawn orders: pos [1,11), g [11,21), row bit 21 | num_orders [24,31), the orders in S.nxt.
constexpr int PDREC_POS_SH = 1, PDREC_G_SH = 11, PDREC_ROW_SH = 21, PDREC_NORD_SH = 24;
constexpr uint32_t PDREC_NONE = 0u, PDREC_READY = 1u, PDREC_NORD_MASK = 0x7Fu;
FJSP_HD constexpr bool pdrec_ready(uint32_t pg) { return (pg & PDREC_READY) != 0u; }
FJSP_HD constexpr int pdrec_nord(uint32_t pg) { return (int)((pg >> PDREC_NORD_SH) & PDREC_NORD_MASK); }
FJSP_HD constexpr int pdrec_pos(uint32_t pg) { return (int)((pg >> PDREC_POS_SH) & MTCUR_IDX_MASK); }
FJSP_HD constexpr int pdrec_g(uint32_t pg) { return (int)((pg >> PDREC_G_SH) & MTCUR_IDX_MASK); }
FJSP_HD constexpr uint32_t pdrec_row(uint32_t pg) { return (pg >> PDREC_ROW_SH) & 1u; }
FJSP_HD constexpr uint32_t pdrec_make(int pos, int g, uint32_t row, int nord) {
    return PDREC_READY | ((uint32_t)pos << PDREC_POS_SH) | ((uint32_t)g << PDREC_G_SH) | (row << PDREC_ROW_SH) |
           ((uint32_t)nord << PDREC_NORD_SH);
}
// the record's cursor as a cursor word (W3 after a reset from the table)
FJSP_HD constexpr uint32_t pdrec_cursor(uint32_t pg) {
    return ((pg >> PDREC_POS_SH) & MTCUR_IDX_MASK) | (((pg >> PDREC_G_SH) & MTCUR_IDX_MASK) << MTCUR_G_SH) |
           (((pg >> PDREC_ROW_SH) & 1u) << MTCUR_ROW_SH);
}
static_assert(MAX_ORDERS <= (int)PDREC_NORD_MASK && PDREC_NORD_SH + 7 <= 32 && (MTCUR_IDX_MASK << PDREC_POS_SH) < (1u << PDREC_G_SH) &&
                  (MTCUR_IDX_MASK << PDREC_G_SH) < (1u << PDREC_ROW_SH) && PDREC_ROW_SH < PDREC_NORD_SH && PDREC_POS_SH > 0,
              "MAX_ORDERS fits the record's 7-bit field; the record's fields do not overlap");
static_assert(pdrec_ready(pdrec_make(0, 0, 0, 0)) && !pdrec_ready(0u) && pdrec_pos(pdrec_make(MT_N, 0, 0, 0)) == MT_N &&
                  pdrec_g(pdrec_make(MT_N, 0, 0, 0)) == 0 && pdrec_g(pdrec_make(0, MT_N, 0, 0)) == MT_N &&
                  pdrec_row(pdrec_make(0, MT_N, 0, 0)) == 0u && pdrec_row(pdrec_make(0, 0, 1, 0)) == 1u &&
                  pdrec_nord(pdrec_make(0, 0, 1, 0)) == 0 && pdrec_nord(pdrec_make(0, 0, 0, MAX_ORDERS)) == MAX_ORDERS &&
                  pdrec_nord(pdrec_make(MT_N, MT_N, 1, 0x7F)) == 0x7F && pdrec_cursor(pdrec_make(7, MT_N, 1, 30)) == mtcur_make(7, MT_N, 1),
              "pre-draw record: decode(encode) at the fields' extremes");
static_assert(pdrec_make(0x155, 0x26F, 1u, 0x2A) == (1u | ((uint32_t)0x155 << 1) | ((uint32_t)0x26F << 11) | (1u << 21) | ((uint32_t)0x2A << 24)) &&
                  pdrec_cursor(0x2A3377ABu) == (((0x2A3377ABu >> 1) & 0x3FFu) | (((0x2A3377ABu >> 11) & 0x3FFu) << 16) | (((0x2A3377ABu >> 21) & 1u) << 31)),
              "the record codec equals the hand-spelled expressions it replaces");

// The per-lane mailboxes between the sim side and the pre-draw wave (predraw_wave, s_mb[0..3]).
//   sim side, word 0: episode counter of the launch (mod 256) [0,8) | num_orders [8,15);
//             word 1: the env's cursor word W3.
//   pre-draw side, word 2: table ready, bit 0 | the episode it is for [1,9) | its num_orders [9,16);
//             word 3: the cursor word after the table (mtcur_make).
constexpr int SIMMB_NORD_SH = 8, PDMB_EPI_SH = 1, PDMB_NORD_SH = 9;
constexpr uint32_t MB_EPI_MASK = 0xFFu, MB_NORD_MASK = 0x7Fu, PDMB_READY = 1u;
constexpr uint32_t MB_EPI_NONE = MB_EPI_MASK + 1u;   // matches no episode counter
FJSP_HD constexpr int mb_next_epi(int epi) { return (epi + 1) & (int)MB_EPI_MASK; }
FJSP_HD constexpr uint32_t simmb_make(uint32_t epi, uint32_t nord) { return epi | (nord << SIMMB_NORD_SH); }
FJSP_HD constexpr uint32_t simmb_epi(uint32_t si) { return si & MB_EPI_MASK; }
FJSP_HD constexpr int simmb_nord(uint32_t si) { return (int)((si >> SIMMB_NORD_SH) & MB_NORD_MASK); }
FJSP_HD constexpr uint32_t pdmb_make(bool ready, uint32_t epi, uint32_t nord) {
    return (ready ? PDMB_READY : 0u) | (epi << PDMB_EPI_SH) | (nord << PDMB_NORD_SH);
}
FJSP_HD constexpr bool pdmb_ready(uint32_t pr) { return (pr & PDMB_READY) != 0u; }
FJSP_HD constexpr uint32_t pdmb_epi(uint32_t pr) { return (pr >> PDMB_EPI_SH) & MB_EPI_MASK; }
FJSP_HD constexpr int pdmb_nord(uint32_t pr) { return (int)((pr >> PDMB_NORD_SH) & MB_NORD_MASK); }
// the table is ready for this episode of the launch and this table size
FJSP_HD constexpr bool pdmb_ready_for(uint32_t pr, int epi, int nord) {
    return (pr & PDMB_READY) && ((pr >> PDMB_EPI_SH) & MB_EPI_MASK) == (uint32_t)epi && (int)((pr >> PDMB_NORD_SH) & MB_NORD_MASK) == nord;
}
static_assert(MAX_ORDERS <= (int)MB_NORD_MASK && MB_EPI_MASK < (1u << SIMMB_NORD_SH) && PDMB_EPI_SH > 0 &&
                  (MB_EPI_MASK << PDMB_EPI_SH) < (1u << PDMB_NORD_SH) && PDMB_NORD_SH + 7 <= 32,
              "MAX_ORDERS fits the mailboxes' 7-bit fields; the mailbox fields do not overlap");
static_assert(simmb_epi(simmb_make(0xFF, 0)) == 0xFFu && simmb_nord(simmb_make(0xFF, 0)) == 0 && simmb_epi(simmb_make(0, 0x7F)) == 0u &&
                  simmb_nord(simmb_make(0, 0x7F)) == 0x7F && pdmb_ready(pdmb_make(true, 0, 0)) && !pdmb_ready(pdmb_make(false, 0xFF, 0x7F)) &&
                  pdmb_epi(pdmb_make(false, 0xFF, 0)) == 0xFFu && pdmb_nord(pdmb_make(true, 0xFF, 0)) == 0 &&
                  pdmb_nord(pdmb_make(false, 0, 0x7F)) == 0x7F && pdmb_epi(pdmb_make(true, 0, 0x7F)) == 0u &&
                  pdmb_ready_for(pdmb_make(true, 0xFF, MAX_ORDERS), 0xFF, MAX_ORDERS) && !pdmb_ready_for(pdmb_make(false, 3, 30), 3, 30) &&
                  !pdmb_ready_for(pdmb_make(true, 3, 30), 4, 30) && !pdmb_ready_for(pdmb_make(true, 3, 30), 3, 31),
              "mailbox words: decode(encode) at the fields' extremes, and the match");
static_assert(simmb_make(0xA5, 0x2A) == ((uint32_t)0xA5 | ((uint32_t)0x2A << 8)) &&
                  pdmb_make(true, 0xA5, 0x2A) == (1u | (0xA5u << 1) | ((uint32_t)0x2A << 9)) &&
                  pdmb_ready_for(0x55ABu, 0xD5, 0x2A) == ((0x55ABu & 1u) && ((0x55ABu >> 1) & 0xFFu) == (uint32_t)0xD5 && (int)((0x55ABu >> 9) & 0x7Fu) == 0x2A),
              "the mailbox codec equals the hand-spelled expressions it replaces");

// Batched reader of the lazily twisted stream for resets.  A refill of B words starts at the
// 16-byte aligned word pa = pos & ~3 and loads the words it needs as two runs of B/4 + 1 uint4
// (words [pa, pa+B+4) and [pa+396, pa+B+400), wrapped into the row; 624 is a multiple of 4
// so no uint4 straddles the wrap), regenerates the words at or past g, writes the batch back
// as uint4 (words before g are written back unchanged) and returns the B tempered words in
// registers; the pos - pa words before pos are skipped by the consumer.  cnt = words of the
// batch inside the row (a multiple of 4; a batch never crosses the wrap).
constexpr int MTB = 32;

// the two runs of a refill at pa (mt_batch), as uint4
template <int B>
FJSP_HD void mt_load(const uint32_t* __restrict__ roww, int pa, uint4 (&va)[(B + 4) / 4], uint4 (&vc)[(B + 4) / 4]) {
    const uint4* row = reinterpret_cast<const uint4*>(roww);
#pragma unroll
    for (int q = 0; q < (B + 4) / 4; q++) {
        int ia = pa + 4 * q;
        ia = ia >= MT_N ? ia - MT_N : ia;
        int ic = pa + 396 + 4 * q;
        ic = ic >= MT_N ? ic - MT_N : ic;
        ic = ic >= MT_N ? ic - MT_N : ic;
        va[q] = row[ia >> 2];
        vc[q] = row[ic >> 2];
    }
}

// mt_batch on runs already loaded (mt_load at pa = pos & ~3, no store to them since)
template <int B>
FJSP_HD void mt_batch_loaded(uint32_t* __restrict__ roww, int pos, int& g, uint32_t (&v)[B], int& pa, int& cnt,
                             const uint4 (&va)[(B + 4) / 4], const uint4 (&vc)[(B + 4) / 4]) {
    uint4* row = reinterpret_cast<uint4*>(roww);
    pa = pos & ~3;
    cnt = (MT_N - pa) < B ? (MT_N - pa) : B;
    uint32_t a[B + 4], c[B + 4];
#pragma unroll
    for (int q = 0; q < (B + 4) / 4; q++) {
        a[4 * q] = va[q].x; a[4 * q + 1] = va[q].y; a[4 * q + 2] = va[q].z; a[4 * q + 3] = va[q].w;
        c[4 * q] = vc[q].x; c[4 * q + 1] = vc[q].y; c[4 * q + 2] = vc[q].z; c[4 * q + 3] = vc[q].w;
    }
    uint32_t w[B];
#pragma unroll
    for (int j = 0; j < B; j++) {
        const uint32_t y = (a[j] & 0x80000000u) | (a[j + 1] & 0x7fffffffu);   // a[cnt] = word 0 at the wrap
        const uint32_t regen = c[j + 1] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);   // word pa + j + 397
        const uint32_t stale = (uint32_t)((pa + j - g) >> 31);   // all ones iff word pa + j < g (already current)
        w[j] = (regen & ~stale) | (a[j] & stale);   // bitwise: no branch per word
        uint32_t t = w[j];
        t ^= t >> 11;
        t ^= (t << 7) & 0x9d2c5680u;
        t ^= (t << 15) & 0xefc60000u;
        t ^= t >> 18;
        v[j] = t;
    }
#pragma unroll
    for (int q = 0; q < B / 4; q++)
        if (4 * q < cnt) row[(pa >> 2) + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
    if (pa + cnt > g) g = pa + cnt;
}

template <int B>
FJSP_HD void mt_batch(uint32_t* __restrict__ roww, int pos, int& g, uint32_t (&v)[B], int& pa, int& cnt) {
    uint4 va[(B + 4) / 4], vc[(B + 4) / 4];
    mt_load<B>(roww, pos & ~3, va, vc);
    mt_batch_loaded<B>(roww, pos, g, v, pa, cnt, va, vc);
}

// generate_order (FJSPSimulation.py:101-131) as a state machine over the stream: per order
// randint(1, 10) then choice(ProductType) then choice(PackagingColor) (:107,111-112) with
// numpy's masked rejection: rng 8 / mask 15 for the product count (field k = 0), rng 2 /
// mask 3 for type and colour (k = 1, 2).
struct OrderDraw {
    int o, k, np, ty;
    uint32_t last;
};

// Consume words [skip, cnt) of one batch (straight-line selects, no per-draw branch) until
// `num_orders` orders are complete; returns the words consumed.  The order word is stored
// every draw, to slot o (overwritten later by order o's own store) or, once the table is
// complete, as the unchanged last order.
template <int B>
FJSP_HD int draw_orders(const uint32_t (&v)[B], int skip, int cnt, int num_orders, OrderDraw& d, uint32_t* orders,
                        int stride) {
    int used = 0;
#pragma unroll
    for (int j = 0; j < B; j++) {
        const bool act = j >= skip && j < cnt && d.o < num_orders;
        const uint32_t x = v[j] & (d.k == 0 ? 15u : 3u);
        const bool acc = act && x <= (d.k == 0 ? 8u : 2u);
        const bool emit = acc && d.k == 2;
        d.np = (acc && d.k == 0) ? 1 + (int)x : d.np;
        d.ty = (acc && d.k == 1) ? 1 + (int)x : d.ty;
        const uint32_t ow = ow_make(d.np, d.ty, 1 + (int)x);
        d.last = emit ? ow : d.last;
        orders[(d.o < num_orders ? d.o : num_orders - 1) * stride] = d.last;
        d.o += emit ? 1 : 0;
        d.k = acc ? (d.k == 2 ? 0 : d.k + 1) : d.k;
        used += act ? 1 : 0;
    }
    return used;
}

// ---------------------------------------------------------------- the pre-draw lane, in slices
// k_step_ag's PD wave draws an env's next table a slice per step, between two barriers.  A
// refill is one 16-byte aligned group of PD_B words at pa = pos & ~3, in three slices that may
// fall in different steps, in this order:
//   load     the two runs of the group into registers (nothing reads them in that step); the
//            runs of the next group may be loaded as soon as a refill has read its own,
//   refill   regenerate, temper and write the group back on the loaded runs; the tempered
//            words stay in registers (held),
//   consume  the held words through draw_orders; the cursor moves, the table may complete.
// The lazily twisted invariant holds after every slice: words [0, g) are current, pos <= g, and
// the row is that of a one-shot draw stopped at g.  Nothing outside the lane depends on where it
// stopped; start() drops the runs and the held words of an abandoned table.
constexpr int PD_B = 4;
struct PreDrawLane {
    int pos, g, nord;
    OrderDraw d;
    int pf_pa;    // group whose runs are loaded, -1 none
    int hcnt;     // held words' count (the group's words inside the row), 0 none held
    int hpa;      // ... and their group
    uint4 ra[(PD_B + 4) / 4], rc[(PD_B + 4) / 4];
    uint32_t v[PD_B];

    FJSP_HD void start(int num_orders, int pos0, int g0) {
        nord = num_orders;
        pos = pos0;
        g = g0;
        d = OrderDraw{0, 0, 0, 0, 0u};
        pf_pa = -1;
        hcnt = 0;
    }
    FJSP_HD bool done() const { return d.o >= nord; }
    // The group to load next: the one at the cursor, or, while the words of a refill are held,
    // the one after it (a consume that does not complete the table ends at that group, and no
    // word of its runs is stored before its refill), so the runs have the consume's step to land.
    FJSP_HD int next_group() const { return hcnt != 0 ? (hpa + PD_B >= MT_N ? 0 : hpa + PD_B) : (pos & ~3); }
    FJSP_HD bool wants_load() const { return hcnt != 0 ? pf_pa == hpa : pf_pa != (pos & ~3); }
    FJSP_HD bool can_refill() const { return hcnt == 0 && pf_pa == (pos & ~3); }
    FJSP_HD bool can_consume() const { return hcnt != 0; }
    FJSP_HD void load(const uint32_t* __restrict__ work) {
        pf_pa = next_group();
        mt_load<PD_B>(work, pf_pa, ra, rc);
    }
    FJSP_HD void refill(uint32_t* __restrict__ work) {
#ifdef __HIP_DEVICE_COMPILE__
        // The second run stays one 16-byte register tuple from its load to here (all four words
        // count as read): of its words only three are, and a load narrowed to those 12 bytes was
        // copied out of its tuple right behind the load, which waits for it in the loading step.
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 t = {rc[0].x, rc[0].y, rc[0].z, rc[0].w};
        asm volatile("" : "+v"(t));
        rc[0] = make_uint4(t.x, t.y, t.z, t.w);
#endif
        mt_batch_loaded<PD_B>(work, pos, g, v, hpa, hcnt, ra, rc);
    }
    // returns whether the table is complete
    FJSP_HD bool consume(uint32_t* orders, int stride) {
        pos += draw_orders<PD_B>(v, pos - hpa, hcnt, nord, d, orders, stride);
        if (pos == MT_N) { pos = 0; g = 0; }
        hcnt = 0;
        if (done()) pf_pa = -1;
        return done();
    }
};

// Which slices the steps of a launch run (k = the step's index in the launch, the same for every
// lane of the wave, so a step executes only its own slices' instructions): alternating, a refill
// in the even steps and a consume in the odd ones, or both in every step.  The load follows
// whenever the lane wants one (wants_load): alternating, that is behind the refill.
template <bool ALTERNATE>
FJSP_HD bool pd_refill_step(int k) { return !ALTERNATE || (k & 1) == 0; }
template <bool ALTERNATE>
FJSP_HD bool pd_consume_step(int k) { return !ALTERNATE || (k & 1) != 0; }

}  // namespace fjsp

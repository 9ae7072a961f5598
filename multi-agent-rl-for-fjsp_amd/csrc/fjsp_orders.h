// fjsp_orders.h — orders from the caller instead of the MT19937 draw (fjsp_put_orders): the per-env
// work of k_put_orders, written so that the same source compiles for the device (fjsp_hip.hip) and
// for the host (tests/hostsim/orders_shim.cpp, TEST-ONLY).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fjsp_env.h"
#include "fjsp_predraw.h"

namespace fjsp {

// A caller's order word: n | type << 4 | colour << 6 (the low byte of fjsp_env_view.orders), n 1..9,
// type 1..3 (ProductType), colour 1..3 (PackagingColor), every other bit 0.
FJSP_HD bool order_word_ok(uint32_t w) {
    const uint32_t n = w & 15u, ty = (w >> 4) & 3u, co = (w >> 6) & 3u;
    return (w >> 8) == 0u && n >= 1u && n <= 9u && ty != 0u && co != 0u;
}

// One env of fjsp_put_orders.  src: the env's column of the caller's table (row k at src[k * sstride]),
// K its rows, count the rows this env uses.  pgw: the env's pre-draw record W[PGW].
//   append == 0: FJSPSimulation.reset (FJSPSimulation.py:301-320) with these orders in place of the
//                generate_order draws: a fresh episode, the MT cursor W3 as it was.
//   append != 0: count calls of generate_order (FJSPSimulation.py:101-131) between two steps: the
//                orders get the ids norders.. of the running episode and join the pickup queue
//                (orders[next_order:]); nothing else of the env changes.
// Both drop a pre-drawn next table: it is a cache of the stream (an auto-reset without it draws the
// same orders from the same position), and one drawn for another order count is never used.
// Validates first, then writes: returns false, with E, the tables and *pgw untouched, on a count
// outside 0..K, an append past MAX_ORDERS or an invalid word in the env's rows.  The table is read
// in two passes over the rows (lanes of a wave read consecutive words of a row); the second hits L2.
FJSP_HD bool put_orders_env(Env& E, const Tables& T, const Cfg& C, const uint32_t* __restrict__ src, int sstride,
                            int K, int count, int append, uint32_t* pgw) {
    const int base = append ? E.norders() : 0;
    bool ok = count >= 0 && count <= K && base + count <= MAX_ORDERS;
    const int rows = ok ? count : 0;
    for (int k = 0; k < rows; k++) ok = order_word_ok(src[(size_t)k * sstride]) && ok;
    if (!ok) return false;
    if (!append) env_clear(E, C);
    for (int k = 0; k < rows; k++) {
        const uint32_t w = src[(size_t)k * sstride];
        T.orders[(base + k) * T.stride] = ow_make((int)(w & 15u), (int)((w >> 4) & 3u), (int)((w >> 6) & 3u));
    }
    E.set_norders(base + rows);
    *pgw = PDREC_NONE;
    return true;
}

}  // namespace fjsp

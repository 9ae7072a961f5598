// orders_san_main.cpp — TEST-ONLY sanitizer run of the host build of fjsp_orders.h's put_orders_env
// with the state machine (orders_shim.cpp), built with -fsanitize=address,undefined
// (tests/test_orders_host.py).  Worlds on the heap, tables sized exactly: full and empty books, every
// kind of rejected call, appends up to the 64th order and one past it, between steps of the built-in
// heuristic; any sanitizer report aborts the run.
#include <stdlib.h>

#include "orders_shim.cpp"

static uint32_t word(uint32_t n, uint32_t ty, uint32_t co) { return n | (ty << 4) | (co << 6); }

int main() {
    int bad = 0;
    for (int K = 0; K <= MAX_ORDERS; K++) {
        void* world = calloc(1, (size_t)orders_world_bytes());
        // the env's column of a [K][3] table, allocated to the last word the call may read
        const int stride = 3;
        uint32_t* tab = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(K ? (K - 1) * stride + 1 : 1));
        for (int k = 0; k < K; k++) tab[k * stride] = word(1 + (uint32_t)(k * 7 + K) % 9, 1 + (uint32_t)k % 3, 1 + (uint32_t)(k / 3) % 3);
        bad += orders_put(world, tab, stride, K, K, 0) != 1;
        bad += orders_put(world, tab, stride, K, K + 1, 0) != 0;
        bad += orders_put(world, tab, stride, K, -1, 1) != 0;
        bad += orders_world_run(world, 40) != 0;
        // arrivals one by one until the table is full, a step of the heuristic between them
        const uint32_t one = word(9, 2, 2), none = 0, high = one | 0x100u;
        for (int o = K; o < MAX_ORDERS; o++) {
            bad += orders_put(world, &none, 1, 1, 1, 1) != 0;
            bad += orders_put(world, &high, 1, 1, 1, 1) != 0;
            bad += orders_put(world, &one, 1, 1, 1, 1) != 1;
            if (o % 8 == 0) bad += orders_world_run(world, 3) != 0;
        }
        bad += orders_put(world, &one, 1, 1, 1, 1) != 0;   // the 65th
        bad += orders_put(world, &one, 1, 1, 0, 1) != 1;   // nothing arrives
        (void)orders_world_run(world, 200);
        free(tab);
        free(world);
    }
    printf("%d wrong answers\n%s\n", bad, bad ? "FAIL" : "OK");
    return bad ? 1 : 0;
}

// search_san_main.cpp — TEST-ONLY sanitizer run of the host build of fjsp_search.h (search_shim.cpp),
// built with -fsanitize=address,undefined (tests/test_search_host.py).  Worlds, scripts, traces and
// end arrays on the heap, sized exactly: books of 1..64 orders, every eps8 endpoint, scripts shorter
// and longer than the run, inactive lanes, a K that ends before the episode and the launch that
// goes on from there; any sanitizer report aborts the run.
#include <stdlib.h>

#include "search_shim.cpp"

static uint32_t word(uint32_t n, uint32_t ty, uint32_t co) { return n | (ty << 4) | (co << 6); }

int main() {
    int bad = 0;
    const int n = 5;
    const int eps[4] = {0, 38, 128, 256};
    for (int B = 1; B <= MAX_ORDERS; B += 9) {
        for (int ei = 0; ei < 4; ei++) {
            const size_t wb = (size_t)search_world_bytes();
            char* worlds = (char*)calloc(n, wb);
            uint32_t* book = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)B);
            for (int k = 0; k < B; k++) book[k] = word(1 + (uint32_t)(k * 7 + B) % 9, 1 + (uint32_t)k % 3, 1 + (uint32_t)(k / 3) % 3);
            for (int e = 0; e < n; e++) bad += search_world_reset(worlds + e * wb, book, B) != 1;
            // launch 1: K = 25, a script of 12 rows: lane 0 all of it, lane 1 five rows, lane 2 none, lane 3
            // inactive, lane 4 a length past L (clamped)
            const int K1 = 25, L = 12;
            uint8_t* script = (uint8_t*)calloc((size_t)L * 8 * n, 1);
            for (int k = 0; k < L; k++) script[(k * 8 + 0) * n + 0] = script[(k * 8 + 0) * n + 4] = 1;   // the pickup station loads
            const int32_t slen[n] = {L, 5, 0, 3, L + 100};
            const uint8_t active[n] = {1, 1, 1, 0, 1};
            uint8_t* trace = (uint8_t*)malloc((size_t)K1 * 8 * n);
            int32_t* steps = (int32_t*)malloc(sizeof(int32_t) * n);
            uint8_t* flags = (uint8_t*)malloc(n);
            int32_t* oc = (int32_t*)malloc(sizeof(int32_t) * n);
            int32_t* pk = (int32_t*)malloc(sizeof(int32_t) * n);
            double* st = (double*)malloc(sizeof(double) * n);
            search_rollout_host(worlds, n, K1, eps[ei], 99u + (uint64_t)B, 7u, 1u << 12, 0, script, L, slen, active, trace,
                                steps, flags, oc, pk, st);
            int32_t first[n];
            for (int e = 0; e < n; e++) {
                first[e] = steps[e];
                if (e == 3) { bad += steps[e] != -1; continue; }
                bad += steps[e] == 0 || steps[e] < -1 || steps[e] > K1;
                bad += st[e] != 10.0 * (steps[e] < 0 ? K1 : steps[e]);
            }
            free(trace);
            // launch 2: to the episode's end without a script, from where launch 1 stopped
            const int K2 = 201 - K1;
            trace = (uint8_t*)malloc((size_t)K2 * 8 * n);
            search_rollout_host(worlds, n, K2, eps[ei], 99u + (uint64_t)B, 7u, 1u << 12, K1, nullptr, 0, nullptr, active, trace,
                                steps, flags, oc, pk, st);
            for (int e = 0; e < n; e++) {
                if (e == 3) { bad += steps[e] != -1; continue; }
                bad += steps[e] < 1 || steps[e] > K2 || (flags[e] & 3) == 0;
                if (first[e] < 0) bad += st[e] != 10.0 * (K1 + steps[e]);
            }
            // a finished lane run again stops at its first step: it still reports its end
            search_rollout_host(worlds, 1, 1, eps[ei], 1u, 0u, 0u, 0, nullptr, 0, nullptr, nullptr, trace, steps, flags, oc, pk, st);
            bad += steps[0] != 1;
            free(trace); free(steps); free(flags); free(oc); free(pk); free(st); free(script); free(book); free(worlds);
        }
    }
    printf("%d wrong answers\n%s\n", bad, bad ? "FAIL" : "OK");
    return bad ? 1 : 0;
}

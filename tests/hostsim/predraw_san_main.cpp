// predraw_san_main.cpp — TEST-ONLY sanitizer run of the host build of fjsp_predraw.h
// (predraw_shim.cpp), built with -fsanitize=address,undefined (tests/test_predraw_host.py): the
// sweep over table sizes, start cursors and both schedules, every slice an interruption point; any
// sanitizer report aborts the run.
#include "predraw_shim.cpp"

int main() {
    static const int NORD[] = {0, 1, 2, 5, 30, 64};
    static const int CUR[][2] = {{0, 0}, {1, 4}, {3, 624}, {226, 228}, {227, 624}, {228, 232}, {396, 400}, {397, 400},
                                 {620, 624}, {623, 624}, {600, 604}, {100, 624}};
    uint32_t key[MT_N];
    uint32_t x = 20240u;
    for (int i = 0; i < MT_N; i++) { x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)i; key[i] = x; }
    advance(key, 0, MT_N);
    long fails = 0, points = 0;
    for (int no : NORD)
        for (auto& cu : CUR)
            for (int alt = 0; alt < 2; alt++) {
                int64_t out[4];
                pd_sweep(key, cu[0], cu[1], no, alt, 1, out);
                fails += out[0];
                points += out[3];
            }
    printf("predraw sweep: %ld failed checks, %ld interruption points\n", fails, points);
    return fails != 0;
}

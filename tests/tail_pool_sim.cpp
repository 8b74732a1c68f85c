// tail_pool_sim.cpp -- csrc/trl_tailpool.h driven from the command line, for tests/test_tail_pool_cpu.py (host only, no GPU, no HIP).
//   tail_pool_sim S k st BM N      a launch of N candidates: M = N S S rows in tiles of BM
// prints what the conv kernels' pooling epilogue and the fix-up kernel compute from the header, clamped to the launch as they clamp:
//   geom P per cells span ok can_straddle
//   first <first_row(g) for every cell g>
//   straddles <0/1 for every cell g>
//   tile t g0 g1 <second_part(g, t) for g0 <= g < g1>      one line per tile
//   cut b g0 g1                                            one line per tile boundary b >= 1 (a fix-up block)
#include <cstdio>
#include <cstdlib>

#include "trl_tailpool.h"

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const TailPool tp{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
    const int N = atoi(argv[5]);
    printf("geom %d %d %d %d %d %d\n", tp.P(), tp.per(), tp.cells(), tp.span(), (int)tp.ok(), (int)tp.can_straddle());
    if (!tp.ok() || N < 1) return 0;
    const int M = N * tp.per(), gend = N * tp.cells(), tiles = (M + tp.BM - 1) / tp.BM;
    printf("first");
    for (int g = 0; g < gend; g++) printf(" %d", tp.first_row(g));
    printf("\nstraddles");
    for (int g = 0; g < gend; g++) printf(" %d", (int)tp.straddles(g));
    printf("\n");
    for (int t = 0; t < tiles; t++) {
        const int g0 = tp.tile_cell0(t);
        int g1 = tp.tile_cell1(t);
        g1 = g1 < gend ? g1 : gend;
        printf("tile %d %d %d", t, g0, g1);
        for (int g = g0; g < g1; g++) printf(" %d", (int)tp.second_part(g, t));
        printf("\n");
    }
    for (int b = 1; b < tiles; b++) {
        const int g0 = tp.cut_cell0(b);
        int g1 = tp.cut_cell1(b);
        g1 = g1 < gend ? g1 : gend;
        printf("cut %d %d %d\n", b, g0, g1);
    }
    return 0;
}

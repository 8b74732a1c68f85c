// defer_sim.cpp -- the confirm queue's capacity arithmetic (csrc/trl_capacity.h) and its block in the arena (csrc/trl_arena.h),
// driven from stdin for tests/test_pnet_defer_cpu.py (host only, no GPU, no HIP).  Commands, one per line:
//   new <forced>                     a fresh context's queue state, "pnet_defer_cap" = forced (0: the policy)
//   call <mtiles> <applicable> <need> <guard>
//                                    one call on content that confirms `need` M-tiles of `mtiles`: attempts through trl_caps_plan's
//                                    companion trl_defer_plan and trl_caps_check until the check asks for no re-run.  Every attempt
//                                    sizes the queue's block over a counting arena and carves it from a real one of exactly that size
//                                    (red zones of `guard` bytes), writes every byte of the slots the device would fill and checks
//                                    the red zone behind the block (layouts above 64 MiB are counted only).
//                                    -> one "attempt cap bytes retry hold frac_bits" line per attempt, then "done attempts"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "trl_arena.h"
#include "trl_capacity.h"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

int main() {
    CascadeCaps caps;
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "new") {
            int forced;
            if (!(in >> forced)) return 2;
            caps = CascadeCaps();
            caps.defer.forced = forced;
        } else if (cmd == "call") {
            long long mtiles, need;
            int applicable;
            size_t guard;
            if (!(in >> mtiles >> applicable >> need >> guard)) return 2;
            int attempts = 0;
            for (;;) {
                DeferCaps& d = caps.defer;
                d.mtiles = mtiles;
                d.cap = trl_defer_plan(d, mtiles, applicable != 0);
                // the dry run and the carve: a block in front (the flags), the queue, a block behind (the spill pool)
                auto layout = [&](Arena& A, char** q) {
                    A.reset("lists");
                    void* f = A.alloc(TRL_NFLAGS * 4);
                    *q = (char*)trl_defer_carve(A, d.cap);
                    void* s = A.alloc(1000);
                    return f && s && (d.cap == 0) == (*q == nullptr);
                };
                Arena count = Arena::counter(guard);
                char* q = nullptr;
                if (!layout(count, &q)) return 3;
                size_t bytes = (size_t)d.cap * TRL_DEFER_SLOT;
                if (count.off <= (64u << 20)) {              // (larger layouts are counted only: the test machine need not hold them)
                    std::vector<char> mem(count.off, (char)0xA5);
                    Arena real = Arena::over(mem.data(), mem.size());
                    real.guard = guard;
                    if (!layout(real, &q)) return 4;               // the count is enough ...
                    if (real.off != count.off) return 5;           // ... and exact
                    if (d.cap > 0) {
                        const long long filled = need < d.cap ? need : d.cap;   // a slot index at or past the capacity stores nothing
                        for (long long sl = 0; sl < filled; sl++) memset(q + (size_t)sl * TRL_DEFER_SLOT, 0, TRL_DEFER_SLOT);
                        if ((size_t)(q - mem.data()) % 256 != 0) return 6;
                        for (size_t i = 0; i < guard; i++) if (q[bytes + i] != (char)0xA5) return 7;   // the red zone behind the queue
                        if (guard && (real.blocks.size() != 3 || real.blocks[1].off != (size_t)(q - mem.data()) || real.blocks[1].bytes != bytes)) return 8;
                    }
                }
                int32_t f[TRL_NFLAGS] = {0};
                if (d.cap > 0) { f[FLG_DEFER] = need > d.cap; f[FLG_DEFER_N] = (int32_t)need; }
                LvLayout lay;
                const CapsVerdict v = trl_caps_check(caps, f, 1, lay);
                attempts++;
                printf("attempt %d %zu %d %d %" PRIu32 "\n", d.cap, bytes, v.retry, d.hold, bits(d.frac));
                if (!v.retry) break;
                if (attempts > 12) return 9;
            }
            printf("done %d\n", attempts);
        } else {
            return 2;
        }
    }
    return 0;
}

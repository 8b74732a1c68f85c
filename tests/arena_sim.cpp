// arena_sim.cpp -- csrc/trl_arena.h alone, driven by a script on stdin (tests/test_arena_cpu.py).
//
//   arena_sim <guard> <cap | "count">
//
// cap: a real arena of that many bytes over a base pointer that is never dereferenced; "count": a counting arena.  Operations, one
// per line:
//   alloc <bytes>   -> "a <offset | null> <off> <high>"
//   reset           -> "r <off> <high>"           (off = 0)
//   rewind <k>      -> "r <off> <high>"           (back to the value `off` had right after the k-th alloc since the last reset;
//                                                   k = 0: the value it had at the reset)
//   counter         -> "c <guard> <counting>"     (Arena::counter(guard) of this arena's guard: what the library sizes it with)
//   blocks          -> "b <n> <off>:<bytes> ..."  (the recorded blocks)
//   over <0|1> <bytes> <want> -> "o <cap> <guard> <counting> <offset | null>"   (Arena::over(null or a base, bytes): what the library
//                                                   lays over a caller's workspace, and one alloc of <want> bytes from it)
// The rewind callback prints "w <mark> <site> <blocks recorded when it ran>" before the offset moves.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trl_arena.h"

static void on_rewind(Arena& a, size_t mark, const char* site, void* owner) {
    printf("w %zu %s %zu\n", mark, site, a.blocks.size());
    if (owner != (void*)&a) abort();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const size_t guard = strtoull(argv[1], nullptr, 10);
    Arena a;
    static char token;                       // base + offset is only ever turned back into the offset
    if (!strcmp(argv[2], "count")) a = Arena::counter(guard);
    else { a = Arena::over(&token, strtoull(argv[2], nullptr, 10)); a.guard = guard; a.on_rewind = on_rewind; a.owner = &a; }
    std::vector<size_t> marks{0};            // off after the k-th alloc since the last reset
    char op[32];
    while (scanf("%31s", op) == 1) {
        if (!strcmp(op, "alloc")) {
            unsigned long long n;
            if (scanf("%llu", &n) != 1) return 2;
            void* p = a.alloc((size_t)n);
            if (!p) printf("a null %zu %zu\n", a.off, a.high);
            else if (a.counting) { if (p != (void*)&a) return 3; printf("a count %zu %zu\n", a.off, a.high); }
            else printf("a %" PRIuPTR " %zu %zu\n", (uintptr_t)p - (uintptr_t)a.base, a.off, a.high);
            marks.push_back(a.off);
        } else if (!strcmp(op, "reset")) {
            a.reset("reset");
            marks.assign(1, 0);
            printf("r %zu %zu\n", a.off, a.high);
        } else if (!strcmp(op, "rewind")) {
            unsigned long long k;
            if (scanf("%llu", &k) != 1 || k >= marks.size()) return 2;
            a.rewind(marks[k], "rewind");
            marks.resize(k + 1);
            printf("r %zu %zu\n", a.off, a.high);
        } else if (!strcmp(op, "counter")) {
            const Arena c = Arena::counter(a.guard);
            printf("c %zu %d\n", c.guard, (int)c.counting);
        } else if (!strcmp(op, "over")) {
            int has;
            unsigned long long n, want;
            if (scanf("%d %llu %llu", &has, &n, &want) != 3) return 2;
            Arena o = Arena::over(has ? &token : nullptr, (size_t)n);
            if (o.base != (has ? &token : nullptr) || o.off || o.high || !o.blocks.empty() || o.on_rewind || o.owner) return 3;
            void* p = o.alloc((size_t)want);
            if (p) printf("o %zu %zu %d %" PRIuPTR "\n", o.cap, o.guard, (int)o.counting, (uintptr_t)p - (uintptr_t)o.base);
            else printf("o %zu %zu %d null\n", o.cap, o.guard, (int)o.counting);
        } else if (!strcmp(op, "blocks")) {
            printf("b %zu", a.blocks.size());
            for (const Arena::Block& b : a.blocks) printf(" %zu:%zu", b.off, b.bytes);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}

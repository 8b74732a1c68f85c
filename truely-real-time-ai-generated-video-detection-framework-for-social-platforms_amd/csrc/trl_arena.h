// trl_arena.h -- the bump allocator every workspace is carved by.  Plain C++17, no HIP header: tests/arena_sim.cpp includes it alone.
#pragma once
#include <cstddef>
#include <vector>

// bump allocator over one device allocation.  Every workspace is sized by a dry run of the code that carves it over a COUNTING arena
// (no base, never full, the same alignment): code handed one launches nothing and does not dereference what alloc returns (a token).
//
// guard (bytes, a multiple of 256; 0 = off, the shipped behaviour): every block is followed by `guard` bytes that belong to no
// block -- a red zone -- and the next block still starts on a 256-byte boundary, so the gap behind a block is >= guard and
// < guard + 256.  The red zone counts as used (`off` and `high` include it), so a counting arena with the same guard still counts
// exactly what the real one carves.  While the guard is on, a real arena remembers the blocks handed out since the last rewind and
// tells its owner before each rewind (on_rewind: the red-zone sweep of trl_redzone.hip looks at the gaps before the layout goes away).
struct Arena {
    struct Block { size_t off, bytes; };
    char* base = nullptr;
    size_t cap = 0, off = 0;
    size_t high = 0;          // largest off since it was last zeroed (a reset() keeps it)
    bool counting = false;
    size_t guard = 0;
    std::vector<Block> blocks;                                         // guard != 0, real arena: the live blocks, in address order
    void (*on_rewind)(Arena& a, size_t mark, const char* site, void* owner) = nullptr;   // before off moves down to `mark`
    void* owner = nullptr;

    // the counting arena that sizes an arena with this guard
    static Arena counter(size_t guard) { Arena a; a.counting = true; a.guard = guard; return a; }
    // a real arena over `bytes` bytes at `mem` that somebody else owns (a caller's workspace); a null `mem` holds nothing
    static Arena over(const void* mem, size_t bytes) { Arena a; a.base = (char*)const_cast<void*>(mem); a.cap = mem ? bytes : 0; return a; }

    // site: a short label of the call site, for the sweep's report
    void reset(const char* site = "reset") { rewind(0, site); }
    // back to an earlier value of `off`: the blocks below it stay
    void rewind(size_t mark, const char* site = "rewind") {
        if (guard && !counting) {
            if (on_rewind) on_rewind(*this, mark, site, owner);
            while (!blocks.empty() && blocks.back().off >= mark) blocks.pop_back();
        }
        off = mark;
    }
    void* alloc(size_t bytes) {
        size_t a = (off + 255) & ~(size_t)255;
        if (!counting && a + bytes + guard > cap) return nullptr;
        off = a + bytes + guard;
        if (off > high) high = off;
        if (guard && !counting) blocks.push_back({a, bytes});
        return counting ? (void*)this : base + a;
    }
};

// trl_capacity.h -- the cascade's optimistic capacities (five list / batch capacities and the fused PNet's confirm queue): their state,
// the plan of an attempt, the feedback after it.
// Host arithmetic only (integers and floats in, integers and floats out): plain C++17, no HIP header, so a host compiler builds it
// for tests/capacity_sim.cpp.  Built with -ffp-contract=off like the library: every float expression below is the operation
// sequence it shows.
//
// Every call runs on optimistic capacities -- record slots per pyramid level, rows per frame, the spill pool of the NMS kernels, the
// R-Net batch, the O-Net batch -- and is re-run when one overflows, which is what lets the detector take any input
// (detect_face() has no candidate limit).  trl_caps_plan() sizes an attempt, the kernels report in the FLG_* words what they
// needed, trl_caps_check() raises what was too small or lets every hint settle towards what recent calls needed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

enum { TRL_NFLAGS = 64 };            // int32 words of CascadeBufs::flags (copied to pinned host memory behind every call)
// The words: a capacity of the attempt was too small (level record list, per-frame list, R-/O-Net batch, spill pool) and what the
// attempt measured (the R-/O-Net candidate totals, the largest per-frame and per-level counts, the spill bytes asked for)
enum { FLG_LEVEL = 0, FLG_FRAME = 1, FLG_T2 = 2, FLG_T3 = 3, FLG_T2N = 4, FLG_T3N = 5, FLG_FRAME_MAX = 6, FLG_SPILL = 7,
       FLG_SPILL_CUR = 8 /* u64 */, FLG_SPILL_LISTS = 10, FLG_LEVEL_MAX = 16 /* [32] */ };
// ... and of the fused PNet's confirm queue (below): it was too small, and the M-tiles the launch asked slots for
enum { FLG_DEFER = 11, FLG_DEFER_N = 12 };

// Candidate lists of one call.  Level l of every frame owns capl[l] record slots (never more than the level has cells); a frame's
// records are contiguous: record (f, l, slot) = lvl_rec[f * S + rec0[l] + slot], S = sum of capl.  The per-frame box lists of
// stages 1-3 hold capF rows.  (Passed to the list kernels by value.)
struct LvLayout {
    int L = 0, S = 0;
    int capl[32] = {0}, rec0[32] = {0};
};

// "Raise on overflow, settle with decay": a hint follows mul * measured / per + add.  An overflow takes that value at once; a call
// that fitted grows to it at once too, and otherwise decays by `decay` per call, never below `floor` (a hint put below its floor by
// hand stays where it is).
struct CapRule { float mul, add, decay, floor; };
inline float trl_cap_follow(const CapRule& r, float cur, float measured, float per, bool overflow) {
    const float want = r.mul * measured / per + r.add;
    if (overflow) return want;
    const float d = r.decay * cur;
    return want > d ? want : (d > r.floor ? d : (cur < r.floor ? cur : r.floor));
}

// The fused PNet's confirm queue (trl_pnet.hip): the persistent kernel screens every conv3 M-tile (32 cells)
// and queues the few that may hold a candidate; a second kernel runs the exact chain on them.  A slot holds what that kernel
// reads: a header {frame, level, ty, tx, mt} and the M-tile's 4 x 18 conv2 cells of 17 floats.  The queue is a block of the
// cascade workspace, `cap` slots; cap == 0: the attempt runs the exact chain inline, in the persistent kernel.
//   start   START slots per M-tile of the launch (+ 64).  The most crowded of the five audited configurations
//           (profiles/pnet_screen_audit.json, configs[4]) confirms ~20 % of its M-tiles; the flagship one 6.7 %.
//           A launch whose every M-tile fits FULL_BYTES gets a slot per M-tile instead: a queue that small is not worth the risk
//           of a re-run (a few frames; the start fraction decides from ~10 frames of 720p on)
//   growth  the slot counter keeps counting past the capacity, so one overflow measures the need N: the re-run gets 1.25 N (+ 64)
//   bound   N beyond BOUND of the M-tiles: the queue would carry the conv2 tile of most of the map through memory (4.9 KB per
//           M-tile, against 2.4 KB of it in the tile): the next HOLD PNet attempts (the re-run is the first) take the inline path, then the queue is
//           tried again (one PNet attempt lost per HOLD calls on content that confirms everywhere, none that oscillates)
// A call that fitted lets the hint follow the need like every other capacity.
enum { TRL_DEFER_HDR = 32, TRL_DEFER_BLOCK = 72 * 17 * 4, TRL_DEFER_SLOT = TRL_DEFER_HDR + TRL_DEFER_BLOCK };   // bytes
static_assert(TRL_DEFER_SLOT % 16 == 0, "slots are copied in 16-byte words");
struct DeferCaps {
    static constexpr float START = 0.25f, BOUND = 0.5f;
    static constexpr CapRule RULE = {1.25f, 0.f, 0.97f, 0.f};   // (the floor is START, applied by trl_defer_plan)
    static constexpr int HOLD = 256;
    static constexpr long long FULL_SLOTS = (64ll << 20) / TRL_DEFER_SLOT;  // 13,617 slots
    static constexpr long long MAX_SLOTS = (4ll << 30) / TRL_DEFER_SLOT;   // a queue never exceeds 4 GiB; a need beyond it is past the bound
    float frac = 0.f;               // slots per M-tile recent calls needed (0: none measured yet)
    int hold = 0;                    // > 0: calls that still take the inline path
    int forced = 0;                  // > 0: slots in place of the START floor (trl_debug_option "pnet_defer_cap")
    int cap = 0; long long mtiles = 0;   // the attempt in progress (trl_defer_plan's result and argument)
};
// slots of an attempt over `mtiles` M-tiles; applicable: the launch can defer at all (screen on, a DEFER instantiation of the net)
inline int trl_defer_plan(const DeferCaps& d, long long mtiles, bool applicable) {
    if (!applicable || mtiles <= 0 || d.hold > 0) return 0;
    long long want = d.forced > 0 ? d.forced : (long long)(DeferCaps::START * (float)mtiles) + 64;
    if (d.forced <= 0 && want < DeferCaps::FULL_SLOTS) want = DeferCaps::FULL_SLOTS;   // (clamped to the M-tiles below)
    const long long hint = d.frac > 0.f ? (long long)(d.frac * (float)mtiles) + 64 : 0;
    if (hint > want) want = hint;
    if (want > mtiles) want = mtiles;            // every M-tile queued: cannot overflow
    if (want > DeferCaps::MAX_SLOTS) want = DeferCaps::MAX_SLOTS;
    return (int)want;
}
// the queue's block: the same call sizes it (a counting arena) and carves it
template <class ArenaT> inline void* trl_defer_carve(ArenaT& A, int cap) { return cap > 0 ? A.alloc((size_t)cap * TRL_DEFER_SLOT) : nullptr; }
// after an attempt that ran on d.cap > 0 slots and queued `need` M-tiles.  true: the queue was too small, run PNet again
inline bool trl_defer_check(DeferCaps& d, bool overflow, int need) {
    const float per = (float)(d.mtiles > 0 ? d.mtiles : 1);
    if ((float)need > DeferCaps::BOUND * per || (long long)(1.25f * (float)need) + 64 > DeferCaps::MAX_SLOTS) d.hold = DeferCaps::HOLD;
    else d.frac = trl_cap_follow(DeferCaps::RULE, d.frac, (float)need, per, overflow);
    return overflow;
}

struct CascadeCaps {
    static constexpr float T_START[2] = {160.f, 48.f};   // R-Net / O-Net candidates per frame of a fresh context
    // ~25 % head-room over the largest batch / list seen, 3 % decay per call.  Batches settle no lower than their start values; the
    // lists' floor is the configured start capacity, applied by trl_caps_plan (hints below it are ignored), so theirs is 0 here.
    static constexpr CapRule T_RULE[2] = {{1.25f, 1.f, 0.97f, T_START[0]}, {1.25f, 1.f, 0.97f, T_START[1]}};
    static constexpr CapRule LIST_RULE = {1.25f, 4.f, 0.97f, 0.f};

    float t_per_frame[2] = {T_START[0], T_START[1]};   // R-Net / O-Net batch: candidates per frame (index = stage - 2 = flag slot)
    float lvl_hint[32] = {0}, frame_hint = 0.f;        // largest per-level count / per-frame stage-1 total recent calls needed
    size_t spill_hint = 0;                             // spill workspace, bytes
    int cap_t[2] = {0, 0};           // batch capacities of the call in progress (trl_caps_plan)
    DeferCaps defer;                 // the fused PNet's confirm queue
    int resume_stage = 0;            // 2 / 3: the next attempt of the call in progress starts at that stage (trl_caps_check)
    int last_attempts = 0;           // attempts the last call took (test hook)
};

// Capacities of one attempt.  Lists: the configured start values, raised to the hints, never beyond what the geometry can produce
// (level l has cells[l] = oh x ow cells; a frame's stage-1 list is a subset of its cells) -- so a frame small enough cannot
// overflow at all.  Batches: hint * n + 64, at most every row of every frame list.
struct CascadePlan { LvLayout lay; int capF = 0; int cap_t[2] = {0, 0}; };
inline int trl_cap_list(long long start, float hint, long long cells) {
    long long want = start;
    if ((long long)hint > want) want = (long long)hint;
    if (want > cells) want = cells;
    if (want < 4) want = 4;
    return (int)((want + 3) & ~3ll);
}
inline CascadePlan trl_caps_plan(const CascadeCaps& k, int cap_level, int cap_frame, const long long* cells, int L, int n) {
    CascadePlan p;
    LvLayout& G = p.lay;
    G.L = L;
    long long cells_total = 0;
    for (int l = 0; l < L; l++) {
        G.capl[l] = trl_cap_list(cap_level, k.lvl_hint[l], cells[l]);
        G.rec0[l] = G.S;
        G.S += G.capl[l];
        cells_total += cells[l];
    }
    p.capF = trl_cap_list(cap_frame, k.frame_hint, cells_total);
    const long long lim = (long long)n * p.capF;
    for (int s = 0; s < 2; s++) {
        const long long want = (long long)(k.t_per_frame[s] * n) + 64;
        p.cap_t[s] = (int)(want < lim ? want : lim);
    }
    return p;
}

// After an attempt: f = its TRL_NFLAGS words, lay = the layout it ran on.  retry: a capacity was too small -- a level's record list,
// a frame's box list, the spill workspace, or the R-/O-Net batch -- and has been raised to what the attempt measured; the caller
// runs the call again from `resume_stage` (0: from the start).  The first overflow in stage order decides: every word the stages
// behind it wrote comes from truncated lists and is not read.
struct CapsVerdict { int retry, resume_stage; };
inline CapsVerdict trl_caps_check(CascadeCaps& k, const int32_t* f, int n, const LvLayout& lay) {
    const int L = lay.L;
    k.resume_stage = 0;
    unsigned long long spill_used = 0;
    memcpy(&spill_used, f + FLG_SPILL_CUR, 8);
    // PNet's confirm queue first: M-tiles that found no slot were not run, so the level lists and everything behind them are incomplete
    if (k.defer.cap > 0 && trl_defer_check(k.defer, f[FLG_DEFER] != 0, f[FLG_DEFER_N])) return {1, 0};
    if (f[FLG_LEVEL]) {                                  // every later stage ran on truncated lists: their totals mean nothing
        long long sum = 0;
        for (int l = 0; l < L; l++) {
            const float want = trl_cap_follow(CascadeCaps::LIST_RULE, k.lvl_hint[l], (float)f[FLG_LEVEL_MAX + l], 1.f, true);
            if (f[FLG_LEVEL_MAX + l] > lay.capl[l] && want > k.lvl_hint[l]) k.lvl_hint[l] = want;
            sum += f[FLG_LEVEL_MAX + l];
        }
        // a frame's stage-1 list is a subset of its candidates: when the per-frame lists of the batch stay under 8 GB at that bound,
        // grow them in the same step (one attempt less for crowded content; otherwise the next attempt measures the real total).
        // Not trl_cap_follow: the bound itself, no head-room
        if ((float)sum > k.frame_hint && (double)sum * 132.0 * (double)n < 8e9) k.frame_hint = (float)sum;
        return {1, 0};
    }
    const float frame_max = (float)f[FLG_FRAME_MAX];
    if (f[FLG_SPILL]) {                                  // lists that found no workspace were dropped: later totals are incomplete
        k.spill_hint = (size_t)spill_used * 2 + (16u << 20);   // not trl_cap_follow: bytes in integers, twice the need + 16 MiB
        if (f[FLG_FRAME]) k.frame_hint = trl_cap_follow(CascadeCaps::LIST_RULE, k.frame_hint, frame_max, 1.f, true);
        return {1, 0};
    }
    if (f[FLG_FRAME]) { k.frame_hint = trl_cap_follow(CascadeCaps::LIST_RULE, k.frame_hint, frame_max, 1.f, true); return {1, 0}; }
    // R-Net's batch first: O-Net ran on an incomplete stage 2 then, its total is meaningless.  The stages in front of the one
    // that overflowed are intact: the re-run starts behind them
    for (int s = 0; s < 2; s++)
        if (f[FLG_T2 + s]) {
            k.t_per_frame[s] = trl_cap_follow(CascadeCaps::T_RULE[s], k.t_per_frame[s], (float)f[FLG_T2N + s], (float)n, true);
            return {1, k.resume_stage = 2 + s};
        }
    // the call fitted.  Follow the content: grow at once, decay towards what recent batches needed, so one crowded batch does not
    // inflate every later call's launches and workspace for the life of the context
    for (int s = 0; s < 2; s++)
        k.t_per_frame[s] = trl_cap_follow(CascadeCaps::T_RULE[s], k.t_per_frame[s], (float)f[FLG_T2N + s], (float)n, false);
    for (int l = 0; l < L; l++)
        k.lvl_hint[l] = trl_cap_follow(CascadeCaps::LIST_RULE, k.lvl_hint[l], (float)f[FLG_LEVEL_MAX + l], 1.f, false);
    k.frame_hint = trl_cap_follow(CascadeCaps::LIST_RULE, k.frame_hint, frame_max, 1.f, false);
    if (k.defer.cap == 0 && k.defer.hold > 0) k.defer.hold--;
    {   // not trl_cap_follow: bytes in integers, 25 % head-room and 1/32 decay by shifts, and a pool under 1 MiB is given up
        const size_t want = (size_t)spill_used + (spill_used >> 2), d = k.spill_hint - (k.spill_hint >> 5);
        k.spill_hint = spill_used ? (want > d ? want : d) : (d > (1u << 20) ? d : 0);
    }
    return {0, 0};
}

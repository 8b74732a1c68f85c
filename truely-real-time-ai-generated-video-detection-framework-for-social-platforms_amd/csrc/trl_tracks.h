// trl_tracks.h -- every decision of the face tracker, for host and device alike:
// k_track_update (trl_tracks.hip) and tests/tracks_main.cpp run this code.  What is NOT here is arithmetic on embeddings: a
// pair's similarity is an input (the kernel computes it with trl_wave_dot512, the host program reads it from a table).
//
// Per frame f, in this order (the caller composes them; each step's rule is the function's):
//   trl_tk_cut         at a frame flagged as a shot boundary, every track ends and frees its slot
//   trl_tk_age         a track with f - last_frame - 1 > max_age ends and frees its slot
//   trl_tk_pair_key    the key of a (live track, detection) pair, NaN when the pair is not admissible
//   trl_tk_greedy      repeat: match the admissible pair of an unmatched track and an unmatched detection with the largest key;
//                      ties to the lower track id, then the lower detection index
//   trl_tk_matched     the matched track takes the detection and makes one step of the drift state machine
//   trl_tk_create      unmatched detections in ascending index start tracks: the free slot of the lowest index, else the slot of
//                      the track not matched or created in this frame with the smallest (last_frame, id), which ends
//   trl_tk_row         a touched track's row of the table
#pragma once
#include <stdint.h>

#include "trl_hd.h"

#define TRL_TK_SLOTS 64
#define TRL_TK_ROW 8              // int32 per table row
#define TRL_TK_NO_SIM 2.0f        // "no comparison": the drift kernels' sentinel

// One slot, 64 bytes.  An all-zero slot is free, so a zero-filled state is a clip's start.
struct TrlTkSlot {
    int32_t used, id, first_frame, last_frame, n_obs, run, hits;
    int32_t src;                  // row of the current window whose embedding is the track's; -1: the state's copy (set per call)
    float box[4];
    float n2;                     // dot512(trk, trk) of that embedding
    int32_t pad[3];
};

struct TrlTkHead {
    long long frames_seen;
    int32_t next_id, dropped, table_overflow, pad[3];
};

// The whole state: the header, the slots, then each slot's embedding.
#define TRL_TK_EMB_OFFSET (sizeof(TrlTkHead) + TRL_TK_SLOTS * sizeof(TrlTkSlot))
#define TRL_TK_STATE_BYTES (TRL_TK_EMB_OFFSET + TRL_TK_SLOTS * 512 * sizeof(float))

// torchvision's box_iou in float32, one rounding per operation (build with -ffp-contract=off): trl_cascade.hip's non-MIN overlap.
TRL_HD float trl_tk_iou(const float* a, const float* b) {
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    const float x1 = a[0] > b[0] ? a[0] : b[0], y1 = a[1] > b[1] ? a[1] : b[1];
    const float x2 = a[2] < b[2] ? a[2] : b[2], y2 = a[3] < b[3] ? a[3] : b[3];
    float w = x2 - x1, h = y2 - y1;
    w = w > 0.f ? w : 0.f;        // (a NaN coordinate makes an area NaN as well, and with it the quotient)
    h = h > 0.f ? h : 0.f;
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}

// A track is live at frame f iff f - last_frame - 1 <= max_age (64-bit: max_age = INT32_MAX never ends a track)
TRL_HD bool trl_tk_live(long long f, int32_t last_frame, int32_t max_age) {
    return f - (long long)last_frame - 1 <= (long long)max_age;
}

// The IoU half of admissibility; a pair that fails it needs no similarity.
TRL_HD bool trl_tk_iou_ok(float iou, float iou_min) { return iou_min <= 0.f || iou >= iou_min; }

// The pair's key -- sim with embeddings, iou without -- or NaN when the pair is not admissible.  NaN fails every comparison, so
// a NaN iou fails iou >= iou_min, a NaN sim fails sim >= sim_min, and a NaN key (iou_min <= 0, no embeddings) is returned as it is.
TRL_HD float trl_tk_pair_key(float iou, float sim, bool has_emb, float iou_min, float sim_min) {
    const float none = __builtin_nanf("");
    if (!trl_tk_iou_ok(iou, iou_min)) return none;
    if (!has_emb) return iou;
    return sim >= sim_min ? sim : none;
}

// model.py:62-66,70 -- one comparison of the state machine (drift_scan_kernel's two lines); returns the frame's flag
TRL_HD int trl_tk_step(int32_t* run, int32_t* hits, float sim) {
    *run = (sim < 0.99f) ? *run + 1 : 0;
    if (*run > 15) { *hits += 1; return 1; }
    return 0;
}

// {first_frame, last_frame, n_obs, run, hits, slot (-1 once ended), 0, 0} at row `id`; nothing for an id past the table
TRL_HD void trl_tk_row(const TrlTkSlot& s, int slot, int32_t* table, int table_cap) {
    if (!table || s.id >= table_cap) return;
    int32_t* r = table + (long long)s.id * TRL_TK_ROW;
    r[0] = s.first_frame; r[1] = s.last_frame; r[2] = s.n_obs; r[3] = s.run; r[4] = s.hits; r[5] = slot; r[6] = 0; r[7] = 0;
}

// Ageing of one slot at frame f: a track that is not live ends.
TRL_HD void trl_tk_age(TrlTkSlot& s, long long f, int32_t max_age, int32_t* table, int table_cap) {
    if (!s.used || trl_tk_live(f, s.last_frame, max_age)) return;
    trl_tk_row(s, -1, table, table_cap);
    s.used = 0;
}

// A cut at this frame (trl_track_update_cuts), before ageing and pairing: a track ends exactly as an aged-out track ends.
TRL_HD void trl_tk_cut(TrlTkSlot& s, int32_t* table, int table_cap) {
    if (!s.used) return;
    trl_tk_row(s, -1, table, table_cap);
    s.used = 0;
}

// ---- greedy matching -------------------------------------------------------------------------------------------------------------
struct TrlTkCand {
    float key;
    int32_t id, det, slot;        // slot < 0: no candidate
};

TRL_HD TrlTkCand trl_tk_no_cand() {
    TrlTkCand c;
    c.key = 0.f; c.id = 0; c.det = 0; c.slot = -1;
    return c;
}

// a is taken before b: the larger key (float comparison: -0 == +0), then the lower track id, then the lower detection index
TRL_HD bool trl_tk_cand_before(const TrlTkCand& a, const TrlTkCand& b) {
    if (a.slot < 0) return false;
    if (b.slot < 0) return true;
    if (a.key != b.key) return a.key > b.key;
    if (a.id != b.id) return a.id < b.id;
    return a.det < b.det;
}

// The first candidate of detection `det`'s column: key[slot * ld + det] over the slots of `avail` (bit s: slot s is live and not
// matched yet; slot_id[s] is its track's id).  The walk is over the set bits: a frame with three live tracks looks at three keys.
TRL_HD TrlTkCand trl_tk_column_first(const float* key, int ld, const int32_t* slot_id, unsigned long long avail, int det) {
    TrlTkCand best = trl_tk_no_cand();
    while (avail) {
        const int s = __builtin_ctzll(avail);
        avail &= avail - 1;
        const float k = key[s * ld + det];
        if (k != k) continue;
        TrlTkCand c;
        c.key = k; c.id = slot_id[s]; c.det = det; c.slot = s;
        if (trl_tk_cand_before(c, best)) best = c;
    }
    return best;
}

// The greedy matching by NL lanes that call this together; lane l owns the detections l, l + NL, ... of nd <= 64, `live` has bit s
// set for every live slot.  Each lane keeps the first candidate of its columns; a round takes the first of them all --
// `W::first(c)` returns, to every lane, the first of the lanes' arguments in trl_tk_cand_before's order -- and only the columns
// whose candidate sat on the matched track look again.  det_slot[d] receives the slot matched to detection d, -1 for none.
// On the host NL = 1 and W::first is the identity.
template <int NL, class W>
TRL_HD void trl_tk_greedy(W& w, int lane, const float* key, int ld, const int32_t* slot_id, unsigned long long live, int nd,
                             int32_t* det_slot) {
    constexpr int PER = TRL_TK_SLOTS / NL;
    TrlTkCand cand[PER];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < PER; i++) {
        const int d = lane + i * NL;
        cand[i] = d < nd ? trl_tk_column_first(key, ld, slot_id, live, d) : trl_tk_no_cand();
        if (d < nd) det_slot[d] = -1;
    }
    for (;;) {
        TrlTkCand mine = cand[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 1; i < PER; i++)
            if (trl_tk_cand_before(cand[i], mine)) mine = cand[i];
        const TrlTkCand b = w.first(mine);
        if (b.slot < 0) break;
        live &= ~(1ull << b.slot);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < PER; i++) {
            const int d = lane + i * NL;
            if (d == b.det) {
                det_slot[d] = b.slot;
                cand[i] = trl_tk_no_cand();
            } else if (cand[i].slot == b.slot) {
                cand[i] = trl_tk_column_first(key, ld, slot_id, live, d);
            }
        }
    }
}

// ---- what a frame does to the slots ----------------------------------------------------------------------------------------------
// A matched track takes the detection (box, n2 = dot512(det, det), src = its row) at frame f; with embeddings it makes one step
// of the state machine with the pair's similarity.  Returns the detection's flag.
TRL_HD int trl_tk_matched(TrlTkSlot& s, const float* box, float n2, int32_t src, long long f, float sim, bool has_emb) {
    s.box[0] = box[0]; s.box[1] = box[1]; s.box[2] = box[2]; s.box[3] = box[3];
    s.n2 = n2;
    s.src = src;
    s.last_frame = (int32_t)f;
    s.n_obs += 1;
    return has_emb ? trl_tk_step(&s.run, &s.hits, sim) : 0;
}

// The slot a new track takes at frame f: the free slot of the lowest index; else the slot of the track that was neither matched nor
// created in this frame (those have last_frame == f) with the smallest last_frame, ties to the smallest id.  -1: none (more than
// 64 detections in a frame, which the caller excludes).
TRL_HD int trl_tk_choose_slot(const TrlTkSlot* slots, long long f) {
    int victim = -1;
    for (int s = 0; s < TRL_TK_SLOTS; s++) {
        if (!slots[s].used) return s;
        if (slots[s].last_frame == (int32_t)f) continue;
        if (victim < 0 || slots[s].last_frame < slots[victim].last_frame ||
            (slots[s].last_frame == slots[victim].last_frame && slots[s].id < slots[victim].id))
            victim = s;
    }
    return victim;
}

// Every unmatched detection (det_slot[d] < 0) of the frame's first nd, in ascending d, starts a track with the next id.  box / n2
// are indexed by d, row0 is the frame's first row in the window; det_slot[d] receives the new track's slot and track[row0 + d] its id.
// An evicted track ends: its row is written with slot -1.  A new id past the table adds to table_overflow.
TRL_HD void trl_tk_create(TrlTkSlot* slots, TrlTkHead& head, int32_t* det_slot, int nd, const float* box, const float* n2, int row0,
                             long long f, int32_t* table, int table_cap, int32_t* track) {
    for (int d = 0; d < nd; d++) {
        if (det_slot[d] >= 0) continue;
        const int s = trl_tk_choose_slot(slots, f);
        if (s < 0) { track[row0 + d] = -1; continue; }
        TrlTkSlot& t = slots[s];
        if (t.used) trl_tk_row(t, -1, table, table_cap);
        t.used = 1;
        t.id = head.next_id++;
        t.first_frame = t.last_frame = (int32_t)f;
        t.n_obs = 1;
        t.run = t.hits = 0;
        t.src = row0 + d;
        t.box[0] = box[4 * d]; t.box[1] = box[4 * d + 1]; t.box[2] = box[4 * d + 2]; t.box[3] = box[4 * d + 3];
        t.n2 = n2 ? n2[d] : 0.f;
        if (t.id >= table_cap) head.table_overflow++;
        det_slot[d] = s;
        track[row0 + d] = t.id;
    }
}

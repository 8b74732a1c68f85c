// trl_tracks.hip -- the face tracker: which face of sampled frame t is which face of frame t - 1, with model.py's drift state
// machine per person.  trl_track_update_cuts (trl_track_update is it without cut flags),
// trl_track_scores; context-free like the gallery.
//
// The decisions are trl_tracks.h's (shared with tests/tracks_main.cpp); this file adds the arithmetic on embeddings
// (trl_wave_dot512, drift_sims_kernel's expression), the schedule and the hand-over between windows.  Refusals and the device
// lookup are trl_host.h's.
#include "trl_host.h"
#include "trl_tracks.h"

static_assert(TRL_TK_SLOTS == TRL_TRACK_SLOTS, "slot count");
static_assert(TRL_TK_STATE_BYTES == TRL_TRACK_STATE_BYTES, "track state layout");
static_assert(sizeof(TrlTkSlot) == 64 && sizeof(TrlTkHead) == 32, "track state layout");

namespace {

constexpr int TK_THREADS = 1024;                 // 16 waves on one CU: the dots wait on L2, more waves hide more of it
constexpr int TK_WAVES = TK_THREADS / 64;

// trl_tk_greedy's W on the device: the xor butterfly over the 64 lanes.  The order is total over distinct detections and every
// "none" equals every other, so all lanes end with the same candidate.
struct TkWave {
    __device__ __forceinline__ TrlTkCand first(TrlTkCand c) const {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            TrlTkCand o;
            o.key = __shfl_xor(c.key, off, 64);
            o.id = __shfl_xor(c.id, off, 64);
            o.det = __shfl_xor(c.det, off, 64);
            o.slot = __shfl_xor(c.slot, off, 64);
            if (trl_tk_cand_before(o, c)) c = o;
        }
        return c;
    }
};

// Lanes of ONE wave hand LDS values to each other without a workgroup barrier: the wave's LDS operations are issued in program
// order, so all this has to do is keep the compiler from moving them across the hand-over.
__device__ __forceinline__ void tk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One workgroup walks the window's frames of ONE tracker: frame t's matching needs frame t - 1's tracks.
//   LDS   key[64][64]   the pair matrix, row = slot, column = detection: the key, NaN = not admissible
//         slots, head   the state's header and slots for the length of the call; the slots' embeddings stay in global memory
//                       (64 x 2 KB, L2-resident), and a track matched in this window reads its embedding from the window's own
//                       row (TrlTkSlot::src) -- the state's copy is written once, at the end of the call
// No pointer is __restrict__: state, table and outputs are read and written by different lanes across barriers.
__global__ __launch_bounds__(TK_THREADS) void k_track_update(char* state, const float* boxes, const int32_t* counts, const uint8_t* cuts, int n,
                                                              int m,                                                              const float* emb, float iou_min, float sim_min, int max_age,
                                                              int32_t* track, float* sim_out, uint8_t* flag_out, int32_t* table,
                                                              int table_cap) {
    __shared__ float key[TRL_TK_SLOTS * TRL_TK_SLOTS];
    __shared__ TrlTkSlot slots[TRL_TK_SLOTS];
    __shared__ TrlTkHead head;
    __shared__ float dbox[TRL_TK_SLOTS * 4];
    __shared__ float dn2[TRL_TK_SLOTS];
    __shared__ int32_t det_slot[TRL_TK_SLOTS];
    __shared__ int32_t slot_id[TRL_TK_SLOTS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool has_emb = emb != nullptr;
    float* state_emb = (float*)(state + TRL_TK_EMB_OFFSET);
    {
        const int32_t* src = (const int32_t*)state;
        int32_t* hd = (int32_t*)&head;
        int32_t* sl = (int32_t*)slots;
        if (tid < (int)(sizeof(TrlTkHead) / 4)) hd[tid] = src[tid];
        for (int i = tid; i < (int)(TRL_TK_SLOTS * sizeof(TrlTkSlot) / 4); i += TK_THREADS) sl[i] = src[sizeof(TrlTkHead) / 4 + i];
    }
    __syncthreads();
    if (tid < TRL_TK_SLOTS) slots[tid].src = -1;          // (rows of an earlier window mean nothing here)
    const long long f0 = head.frames_seen;
    __syncthreads();

    int off = 0;                                          // the frame's first row: the exclusive prefix sum of counts, in every thread
    for (int t = 0; t < n; t++) {
        const long long f = f0 + t;
        int c = counts[t];
        if (c < 0) c = 0;
        if (c > m - off) c = m - off;                     // rows past the tensors are not there
        const int nd = c < TRL_TK_SLOTS ? c : TRL_TK_SLOTS;
        // detections past the first 64: no track
        for (int d = nd + tid; d < c; d += TK_THREADS) {
            track[off + d] = -1;
            sim_out[off + d] = TRL_TK_NO_SIM;
            flag_out[off + d] = 0;
        }
        // 1. a cut ends every track; ageing.  Wave 0 alone owns the slots between the last barrier of a frame and the first of the
        // next: no barrier there.
        if (wave == 0) {
            if (lane == 0) head.dropped += c - nd;
            if (cuts && cuts[t]) trl_tk_cut(slots[lane], table, table_cap);
            trl_tk_age(slots[lane], f, max_age, table, table_cap);
            slot_id[lane] = slots[lane].used ? slots[lane].id : -1;
            for (int i = lane; i < nd * 4; i += 64) dbox[i] = boxes[(size_t)off * 4 + i];
        }
        __syncthreads();
        const unsigned long long live = __ballot(slot_id[lane] >= 0);
        // 2. pairs.  Without embeddings the key is the IoU: a lane per pair.
        if (!has_emb) {
            if (live)
                for (int p = tid; p < TRL_TK_SLOTS * TRL_TK_SLOTS; p += TK_THREADS) {
                    const int s = p >> 6, d = p & 63;
                    if (d < nd && ((live >> s) & 1)) key[p] = trl_tk_pair_key(trl_tk_iou(slots[s].box, dbox + 4 * d), 0.f, false, iou_min, sim_min);
                }
        } else {
            // dot512(det, det) of every detection: what a matched or new track keeps as its dot512(trk, trk)
            for (int d = wave; d < nd; d += TK_WAVES) {
                const float* e = emb + (size_t)(off + d) * 512;
                const float v = trl_wave_dot512(e, e, lane);
                if (lane == 0) dn2[d] = v;
            }
            // a wave per track, its row in registers; lane d holds the pair (track, d) and its IoU, and the wave walks the pairs
            // that pass the IoU test (the set bits of the ballot), one dot each.  dot512(det, det) comes from the row the dot has
            // loaded anyway, so this pass does not wait for the one above; the tracks go to the waves from the last wave down, so
            // that with few faces the two passes' loads are in flight together.
            for (int s = TK_WAVES - 1 - wave; s < TRL_TK_SLOTS; s += TK_WAVES) {
                if (!((live >> s) & 1)) continue;
                const float iou = lane < nd ? trl_tk_iou(slots[s].box, dbox + 4 * lane) : 0.f;
                unsigned long long todo = __ballot(lane < nd && trl_tk_iou_ok(iou, iou_min));
                float k = __builtin_nanf("");
                if (todo) {
                    const int32_t src = slots[s].src;
                    const float* tp = src >= 0 ? emb + (size_t)src * 512 : state_emb + (size_t)s * 512;
                    float tv[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) tv[i] = tp[lane + 64 * i];
                    const float nt = sqrtf(slots[s].n2);
                    while (todo) {
                        const int d = __builtin_ctzll(todo);
                        todo &= todo - 1;
                        const float* dp = emb + (size_t)(off + d) * 512;
                        float dv[8], a = 0.f, dd = 0.f;   // trl_wave_dot512(det, trk), trl_wave_dot512(det, det)
#pragma unroll
                        for (int i = 0; i < 8; i++) dv[i] = dp[lane + 64 * i];
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            a = __builtin_fmaf(dv[i], tv[i], a);
                            dd = __builtin_fmaf(dv[i], dv[i], dd);
                        }
#pragma unroll
                        for (int o = 32; o >= 1; o >>= 1) {
                            a = a + __shfl_xor(a, o, 64);
                            dd = dd + __shfl_xor(dd, o, 64);
                        }
                        const float sim = a / (sqrtf(dd) * nt);
                        if (lane == d) k = trl_tk_pair_key(iou, sim, true, iou_min, sim_min);
                    }
                }
                if (lane < nd) key[s * TRL_TK_SLOTS + lane] = k;
            }
        }
        __syncthreads();
        if (wave == 0) {
            // 3. greedy matching by one wave, a lane per detection
            TkWave w;
            trl_tk_greedy<64>(w, lane, key, TRL_TK_SLOTS, slot_id, live, nd, det_slot);
            // 4. matched tracks (distinct slots: a lane each)
            if (lane < nd) {
                const int s = det_slot[lane];
                float so = TRL_TK_NO_SIM;
                int fl = 0;
                if (s >= 0) {
                    const float k = key[s * TRL_TK_SLOTS + lane];
                    fl = trl_tk_matched(slots[s], dbox + 4 * lane, has_emb ? dn2[lane] : 0.f, off + lane, f, k, has_emb);
                    if (has_emb) so = k;
                    track[off + lane] = slots[s].id;
                }
                sim_out[off + lane] = so;
                flag_out[off + lane] = (uint8_t)fl;
            }
            tk_wave_sync();
            // 5. new tracks: ids and slots go by ascending detection index, one lane
            if (lane == 0) trl_tk_create(slots, head, det_slot, nd, dbox, has_emb ? dn2 : nullptr, off, f, table, table_cap, track);
            tk_wave_sync();
            // 6. the rows of the tracks touched by this frame
            if (slots[lane].used && slots[lane].last_frame == (int32_t)f) trl_tk_row(slots[lane], lane, table, table_cap);
            tk_wave_sync();
        }
        off += c;
    }
    __syncthreads();
    // rows past the sum of counts
    for (int i = off + tid; i < m; i += TK_THREADS) {
        track[i] = -1;
        sim_out[i] = TRL_TK_NO_SIM;
        flag_out[i] = 0;
    }
    // hand-over: the embedding of every track matched or created in this window
    if (has_emb)
        for (int s = wave; s < TRL_TK_SLOTS; s += TK_WAVES) {
            const int32_t src = slots[s].src;
            if (!slots[s].used || src < 0) continue;
#pragma unroll
            for (int i = 0; i < 8; i++) state_emb[(size_t)s * 512 + lane + 64 * i] = emb[(size_t)src * 512 + lane + 64 * i];
        }
    __syncthreads();
    if (tid < TRL_TK_SLOTS) slots[tid].src = -1;
    if (tid == 0) head.frames_seen = f0 + n;
    __syncthreads();
    {
        int32_t* dst = (int32_t*)state;
        const int32_t* hd = (const int32_t*)&head;
        const int32_t* sl = (const int32_t*)slots;
        if (tid < (int)(sizeof(TrlTkHead) / 4)) dst[tid] = hd[tid];
        for (int i = tid; i < (int)(TRL_TK_SLOTS * sizeof(TrlTkSlot) / 4); i += TK_THREADS) dst[sizeof(TrlTkHead) / 4 + i] = sl[i];
    }
}

// Per table row the score of its track (model.py:86-95 with the track's run and hits); the clip's score is the largest, the
// lowest id among equals.  One workgroup.
__global__ __launch_bounds__(256) void k_track_scores(const char* state, const int32_t* table, int table_cap, long long frame_count, int fps,
                                                      int32_t* score, int32_t* summary) {
    __shared__ unsigned long long best;
    const TrlTkHead* head = (const TrlTkHead*)state;
    const int next_id = head->next_id;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int i = threadIdx.x; i < table_cap; i += blockDim.x) {
        int sc = 0;
        if (i < next_id) {
            long long total;
            sc = trl_drift_score_value(table[(size_t)i * TRL_TK_ROW + 4], table[(size_t)i * TRL_TK_ROW + 3], frame_count, fps, &total);
            const unsigned long long k = ((unsigned long long)sc << 32) | (unsigned)(0x7fffffff - i);   // larger score, then lower id
            if (k > mine) mine = k;
        }
        score[i] = sc;
    }
    if (mine) atomicMax(&best, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        summary[0] = best ? (int32_t)(best >> 32) : 0;
        summary[1] = best ? 0x7fffffff - (int32_t)(best & 0xffffffffu) : -1;
        summary[2] = next_id;
        summary[3] = head->dropped;
    }
}

}  // namespace

namespace {
// both entries; `who` is the one that was called
int tk_update(const char* who, void* d_state, const float* d_boxes, const int32_t* d_counts, const uint8_t* d_cut, int n, int m,
              const float* d_emb, float iou_min, float sim_min, int max_age, int32_t* d_track, float* d_sim, uint8_t* d_flag, int32_t* d_table,
              int table_cap, void* stream) {
    if (n < 0 || m < 0 || max_age < 0 || table_cap < 0) {
        trl_set_error("%s: n = %d, m = %d, max_age = %d, table_cap = %d", who, n, m, max_age, table_cap);
        return TRL_ERR_INVALID;
    }
    if (iou_min != iou_min || sim_min != sim_min) return trl_refuse(who, "a NaN threshold");
    if (!d_state || ((uintptr_t)d_state & 7)) return trl_refuse(who, "the state is null or not 8-byte aligned");
    if ((n > 0 && !d_counts) || (m > 0 && (!d_boxes || !d_track || !d_sim || !d_flag)) || (table_cap > 0 && !d_table))
        return trl_refuse(who, "null argument");
    TRL_CHECK(trl_device_of(d_state));
    k_track_update<<<1, TK_THREADS, 0, (hipStream_t)stream>>>((char*)d_state, d_boxes, d_counts, d_cut, n, m, d_emb, iou_min, sim_min, max_age,
                                                             d_track, d_sim, d_flag, d_table, table_cap);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
}  // namespace

extern "C" int trl_track_update_cuts(void* d_state, const float* d_boxes, const int32_t* d_counts, const uint8_t* d_cut, int n, int m,
                                     const float* d_emb, float iou_min, float sim_min, int max_age, int32_t* d_track, float* d_sim,
                                     uint8_t* d_flag, int32_t* d_table, int table_cap, void* stream) {
    return tk_update("trl_track_update_cuts", d_state, d_boxes, d_counts, d_cut, n, m, d_emb, iou_min, sim_min, max_age, d_track, d_sim, d_flag,
                     d_table, table_cap, stream);
}

// no cut flags: the same call
extern "C" int trl_track_update(void* d_state, const float* d_boxes, const int32_t* d_counts, int n, int m, const float* d_emb, float iou_min,
                                float sim_min, int max_age, int32_t* d_track, float* d_sim, uint8_t* d_flag, int32_t* d_table, int table_cap,
                                void* stream) {
    return tk_update("trl_track_update", d_state, d_boxes, d_counts, nullptr, n, m, d_emb, iou_min, sim_min, max_age, d_track, d_sim, d_flag,
                     d_table, table_cap, stream);
}

extern "C" int trl_track_scores(const void* d_state, const int32_t* d_table, int table_cap, long long frame_count, int fps, int32_t* d_score,
                                int32_t* d_summary, void* stream) {
    if (table_cap < 0) { trl_set_error("trl_track_scores: table_cap = %d", table_cap); return TRL_ERR_INVALID; }
    if (!d_state || !d_summary || (table_cap > 0 && (!d_table || !d_score))) return trl_refuse("trl_track_scores", "null argument");
    TRL_CHECK(trl_device_of(d_state));
    k_track_scores<<<1, 256, 0, (hipStream_t)stream>>>((const char*)d_state, d_table, table_cap, frame_count, fps, d_score, d_summary);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

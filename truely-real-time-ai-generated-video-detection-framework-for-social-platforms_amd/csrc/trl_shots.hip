// trl_shots.hip -- shot boundaries ("Shots"; section 7, f-15): the signature of every sampled frame where it lies
// on the device, the distance of two signatures, and the cut flags and shot ids of a clip carried across windows.  The rules are
// trl_shots.h's; this file is their schedule.  Context-free, like the gallery and face quality.
//
// k_shots_hist: the grid is (4 rows of regions x slots) x frames.  A band -- consecutive rows inside ONE row of regions -- is one
// contiguous run of bytes of the frame; a workgroup strides over its slot's bands and reads each as 16-byte words at aligned
// addresses, lanes on consecutive words (the bytes of the first and last word that lie outside the band are masked, so the frames
// may sit at any byte address).  A byte's column band and channel come from its position in the row, kept per lane as a running
// (x, c) pair: one modulo per word, none per byte.  The 4 x 3 x 32 counters of the row of regions live in LDS THIRTY-TWO TIMES,
// word = counter * 32 + (lane & 31): the bank of every LDS atomic is the lane's, whatever the pixels are, so a constant frame --
// every lane on one counter -- has the LDS traffic of noise.  At the end the copies are summed (each thread walks them rotated by
// its index: conflict-free again) and stored as the workgroup's partial in the caller's workspace: no global atomics, no memset.
// k_shots_sum: out[f][i][.] = the sum of the slots' partials.  Integers: the order is irrelevant.
// k_shots_dist: a wave per pair; lane l < 48 takes (region l / 3, channel l % 3) through trl_shots_channel_emd, the three channels
// meet by shuffles, lane 0 runs trl_shots_distance_of.  k_shots_scan: one wave walks the window 64 frames at a time: the ballot of
// the frames at or above the threshold, min_shot over its set bits, the shot ids by popcount; it leaves the state for the next window.
#include "trl_host.h"
#include "trl_shots.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_COPIES = 32;
constexpr int SH_ROW = TRL_SHOTS_GRID * TRL_SHOTS_CHANNELS * TRL_SHOTS_BINS;    // 384 counters of a row of regions
constexpr int SH_SLOTS_MAX = 16;
constexpr int SH_GRID_TARGET = 2048;                                            // workgroups a call aims at

// how a call is cut: rows per band, slots per row of regions
struct ShPlan {
    int band_rows, slots;
};
ShPlan sh_plan(int n, int H, int max_band_rows) {
    const int hmax = (H + TRL_SHOTS_GRID - 1) / TRL_SHOTS_GRID;                // rows of the tallest row of regions
    const int frames = n > 0 ? n : 1;
    int want = (SH_GRID_TARGET + TRL_SHOTS_GRID * frames - 1) / (TRL_SHOTS_GRID * frames);
    if (want > SH_SLOTS_MAX) want = SH_SLOTS_MAX;
    ShPlan p;
    p.band_rows = max_band_rows ? max_band_rows : (hmax + want - 1) / want;
    if (p.band_rows > hmax) p.band_rows = hmax;
    const int bands = (hmax + p.band_rows - 1) / p.band_rows;
    p.slots = bands < want ? bands : want;
    return p;
}

// one 32-bit word of a 16-byte load: bytes at band offsets o .. o + 3, row position (x, c) of the first
template <bool CHECK>
__device__ __forceinline__ void sh_word(unsigned w, int o, int len, int& x, int& c, int rb, int b1, int b2, int b3, int* mine) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int j = (x >= b1) + (x >= b2) + (x >= b3);
        const int bin = (w >> (8 * t + 3)) & 31;
        if (!CHECK || (unsigned)(o + t) < (unsigned)len) atomicAdd(mine + ((j * 3 + c) * TRL_SHOTS_BINS + bin) * SH_COPIES, 1);
        x++, c++;
        if (x == rb) x = 0, c = 0;
        else if (c == 3) c = 0;
    }
}

__device__ __forceinline__ void sh_chunk(uint4 v, int o, int len, int rb, int b1, int b2, int b3, int* mine) {
    int x = (o + 2 * rb) % rb, c = x % 3;                                       // (o >= -15, rb >= 12)
    if (o >= 0 && o + 16 <= len) {
        sh_word<false>(v.x, o, len, x, c, rb, b1, b2, b3, mine);
        sh_word<false>(v.y, o + 4, len, x, c, rb, b1, b2, b3, mine);
        sh_word<false>(v.z, o + 8, len, x, c, rb, b1, b2, b3, mine);
        sh_word<false>(v.w, o + 12, len, x, c, rb, b1, b2, b3, mine);
    } else {
        sh_word<true>(v.x, o, len, x, c, rb, b1, b2, b3, mine);
        sh_word<true>(v.y, o + 4, len, x, c, rb, b1, b2, b3, mine);
        sh_word<true>(v.z, o + 8, len, x, c, rb, b1, b2, b3, mine);
        sh_word<true>(v.w, o + 12, len, x, c, rb, b1, b2, b3, mine);
    }
}

// blockIdx.x = 4 * slot + i, blockIdx.y = frame; part[frame][i][slot][384]
__global__ __launch_bounds__(SH_THREADS) void k_shots_hist(const uint8_t* __restrict__ frames, int H, int W, int band_rows, int slots,
                                                           int32_t* __restrict__ part) {
    __shared__ int hist[SH_ROW * SH_COPIES];                                    // 48 KiB
    const int tid = threadIdx.x;
    const int i = blockIdx.x & 3, slot = blockIdx.x >> 2;
    const size_t f = blockIdx.y;
    for (int k = tid; k < SH_ROW * SH_COPIES; k += SH_THREADS) hist[k] = 0;
    __syncthreads();
    const int rb = 3 * W;
    const int b1 = 3 * trl_shots_edge(W, 1), b2 = 3 * trl_shots_edge(W, 2), b3 = 3 * trl_shots_edge(W, 3);
    const int r0 = trl_shots_edge(H, i), r1 = trl_shots_edge(H, i + 1);
    const uint8_t* fb = frames + f * (size_t)H * (size_t)rb;
    int* mine = hist + (tid & (SH_COPIES - 1));
    for (int y0 = r0 + slot * band_rows; y0 < r1; y0 += slots * band_rows) {
        const int y1 = y0 + band_rows < r1 ? y0 + band_rows : r1;
        const uint8_t* p0 = fb + (size_t)y0 * (size_t)rb;
        const int len = (y1 - y0) * rb;                                         // <= 4096 * 49152 bytes
        const int mis = (int)((uintptr_t)p0 & 15);
        const uint4* q = reinterpret_cast<const uint4*>(p0 - mis);
        const int chunks = (mis + len + 15) >> 4;
        for (int k = tid; k < chunks; k += 2 * SH_THREADS) {                     // two loads in flight per lane
            const bool two = k + SH_THREADS < chunks;
            const uint4 va = q[k];
            uint4 vb = make_uint4(0, 0, 0, 0);
            if (two) vb = q[k + SH_THREADS];
            sh_chunk(va, 16 * k - mis, len, rb, b1, b2, b3, mine);
            if (two) sh_chunk(vb, 16 * (k + SH_THREADS) - mis, len, rb, b1, b2, b3, mine);
        }
    }
    __syncthreads();
    int32_t* out = part + ((f * TRL_SHOTS_GRID + i) * (size_t)slots + slot) * SH_ROW;
    for (int k = tid; k < SH_ROW; k += SH_THREADS) {
        int s = 0;
#pragma unroll
        for (int r = 0; r < SH_COPIES; r++) s += hist[k * SH_COPIES + ((r + k) & (SH_COPIES - 1))];
        out[k] = s;
    }
}

// sig[f][4 i + j][c][b] = sum over the slots of part[f][i][slot][j][c][b]
__global__ __launch_bounds__(SH_THREADS) void k_shots_sum(const int32_t* __restrict__ part, long long total, int slots,
                                                          int32_t* __restrict__ sig) {
    const long long e = (long long)blockIdx.x * SH_THREADS + threadIdx.x;       // f * 1536 + i * 384 + k
    if (e >= total) return;
    const long long fi = e / SH_ROW;
    const int k = (int)(e % SH_ROW);
    const int32_t* p = part + (size_t)fi * (size_t)slots * SH_ROW + k;
    int s = 0;
    for (int v = 0; v < slots; v++) s += p[(size_t)v * SH_ROW];
    sig[e] = s;
}

// the distance of signatures a and b by one wave; the result is lane 0's
__device__ __forceinline__ float sh_wave_distance(const int32_t* a, const int32_t* b, int H, int W, int drop, int lane) {
    long long d = 0;
    if (lane < TRL_SHOTS_REGIONS * TRL_SHOTS_CHANNELS) d = trl_shots_channel_emd(a + lane * TRL_SHOTS_BINS, b + lane * TRL_SHOTS_BINS);
    long long dr[TRL_SHOTS_REGIONS];
#pragma unroll
    for (int r = 0; r < TRL_SHOTS_REGIONS; r++) dr[r] = __shfl(d, 3 * r, 64) + __shfl(d, 3 * r + 1, 64) + __shfl(d, 3 * r + 2, 64);
    return trl_shots_distance_of(dr, H, W, drop);
}

__global__ __launch_bounds__(SH_THREADS) void k_shots_dist(const int32_t* __restrict__ a, const int32_t* __restrict__ b, long long pairs,
                                                           int H, int W, int drop, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (SH_THREADS / 64);
    for (long long p = (long long)blockIdx.x * (SH_THREADS / 64) + (threadIdx.x >> 6); p < pairs; p += waves) {
        const float v = sh_wave_distance(a + (size_t)p * TRL_SHOTS_SIG, b + (size_t)p * TRL_SHOTS_SIG, H, W, drop, lane);
        if (lane == 0) dist[p] = v;
    }
}

// dist[t] of the window's frames: frame 0 against the state's signature (2.0 at a clip's start), frame t against frame t - 1
__global__ __launch_bounds__(SH_THREADS) void k_shots_window_dist(const TrlShotsState* __restrict__ state, const int32_t* __restrict__ sig,
                                                                  int n, int H, int W, int drop, float* __restrict__ dist) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * (SH_THREADS / 64) + (threadIdx.x >> 6);
    if (t >= n) return;
    if (t == 0 && state->frames_seen == 0) {
        if (lane == 0) dist[0] = TRL_SHOTS_NO_DIST;
        return;
    }
    const int32_t* prev = t == 0 ? state->sig : sig + (size_t)(t - 1) * TRL_SHOTS_SIG;
    const float v = sh_wave_distance(prev, sig + (size_t)t * TRL_SHOTS_SIG, H, W, drop, lane);
    if (lane == 0) dist[t] = v;
}

// one wave: the cut flags and shot ids of the window, and the state the next window starts from
__global__ __launch_bounds__(64) void k_shots_scan(TrlShotsState* state, const int32_t* __restrict__ sig, const float* __restrict__ dist,
                                                   int n, float threshold, int min_shot, uint8_t* __restrict__ cut,
                                                   int32_t* __restrict__ shot) {
    const int lane = threadIdx.x;
    const long long f0 = state->frames_seen;
    long long last_cut = state->last_cut, cuts = state->cuts;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        const float d = t < n ? dist[t] : TRL_SHOTS_NO_DIST;
        unsigned long long cand = __ballot(trl_shots_is_cut(d, threshold, 0, 0, 0, min_shot)), mask = 0;      // (min_shot aside)
        const long long before = cuts;
        while (cand) {
            const int l = __builtin_ctzll(cand);
            cand &= cand - 1;
            if (cuts == 0 || f0 + base + l - last_cut >= (long long)min_shot) mask |= 1ull << l, last_cut = f0 + base + l, cuts++;
        }
        if (t < n) {
            cut[t] = (uint8_t)((mask >> lane) & 1);
            shot[t] = (int32_t)(before + __popcll(mask & (~0ull >> (63 - lane))));
        }
    }
    __syncthreads();                                                            // (every lane has read the header)
    for (int k = lane; k < TRL_SHOTS_SIG; k += 64) state->sig[k] = sig[(size_t)(n - 1) * TRL_SHOTS_SIG + k];
    if (lane == 0) state->frames_seen = f0 + n, state->last_cut = last_cut, state->cuts = cuts;
}

// the workspace of a call: the workgroups' partials, [n][4][slots][384] int32.  trl_shots_workspace is a dry run of this
bool sh_carve(Arena& a, int n, int slots, int32_t** part) {
    *part = (int32_t*)a.alloc((size_t)(n > 0 ? n : 1) * TRL_SHOTS_GRID * (size_t)slots * SH_ROW * sizeof(int32_t));
    return *part != nullptr;
}

}  // namespace

extern "C" size_t trl_shots_workspace(int n, int H, int W, int max_band_rows) {
    if (n < 0 || n > TRL_SHOTS_MAX_FRAMES || !trl_shots_dim_ok(H, W) || max_band_rows < 0) return 0;
    Arena a = Arena::counter(0);
    int32_t* part;
    sh_carve(a, n, sh_plan(n, H, max_band_rows).slots, &part);
    return a.high;
}

extern "C" int trl_frame_signatures(const uint8_t* d_frames, int n, int H, int W, int max_band_rows, void* d_ws, size_t ws_bytes,
                                    int32_t* d_sig, void* stream) {
    const char* who = "trl_frame_signatures";
    if (n < 0 || n > TRL_SHOTS_MAX_FRAMES) return trl_refuse(who, "n outside 0..65535");
    if (!trl_shots_dim_ok(H, W)) return trl_refuse(who, "H or W outside 4..16384");
    if (max_band_rows < 0) return trl_refuse(who, "max_band_rows < 0");
    if (n == 0) return TRL_OK;
    if (!d_frames || !d_sig) return trl_refuse(who, "null argument");
    if (!d_ws) return trl_refuse(who, "null workspace");
    const ShPlan plan = sh_plan(n, H, max_band_rows);
    Arena a = Arena::over(d_ws, ws_bytes);
    int32_t* part;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, sh_carve(a, n, plan.slots, &part), [&] { return trl_shots_workspace(n, H, W, max_band_rows); }))
        return TRL_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_device_of(d_ws));
    k_shots_hist<<<dim3((unsigned)(TRL_SHOTS_GRID * plan.slots), (unsigned)n), SH_THREADS, 0, s>>>(d_frames, H, W, plan.band_rows, plan.slots,
                                                                                                   part);
    TRL_LAUNCH_CHECK();
    const long long total = (long long)n * TRL_SHOTS_SIG;
    k_shots_sum<<<(unsigned)((total + SH_THREADS - 1) / SH_THREADS), SH_THREADS, 0, s>>>(part, total, plan.slots, d_sig);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_signature_distance(const int32_t* d_a, const int32_t* d_b, long long pairs, int H, int W, int drop, float* d_dist,
                                      void* stream) {
    const char* who = "trl_signature_distance";
    if (pairs < 0) return trl_refuse(who, "pairs < 0");
    if (!trl_shots_dim_ok(H, W)) return trl_refuse(who, "H or W outside 4..16384");
    if (!trl_shots_drop_ok(drop)) return trl_refuse(who, "drop outside 0..15");
    if (pairs == 0) return TRL_OK;
    if (!d_a || !d_b || !d_dist) return trl_refuse(who, "null argument");
    TRL_CHECK(trl_device_of(d_dist));
    long long wgs = (pairs + SH_THREADS / 64 - 1) / (SH_THREADS / 64);
    if (wgs > 65536) wgs = 65536;                                               // (the waves stride over the rest)
    k_shots_dist<<<(unsigned)wgs, SH_THREADS, 0, (hipStream_t)stream>>>(d_a, d_b, pairs, H, W, drop, d_dist);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_shots_update(void* d_state, const int32_t* d_sig, int n, int H, int W, const trl_shots_params* params, float* d_dist,
                                uint8_t* d_cut, int32_t* d_shot, void* stream) {
    const char* who = "trl_shots_update";
    if (n < 0) return trl_refuse(who, "n < 0");
    if (!trl_shots_dim_ok(H, W)) return trl_refuse(who, "H or W outside 4..16384");
    const trl_shots_params prm = params ? *params : trl_shots_defaults();
    if (!trl_shots_params_ok(prm)) return trl_refuse(who, "a threshold that is not finite, drop outside 0..15 or min_shot < 1");
    if (!d_state || ((uintptr_t)d_state & 7)) return trl_refuse(who, "the state is null or not 8-byte aligned");
    if (n == 0) return TRL_OK;
    if (!d_sig || !d_dist || !d_cut || !d_shot) return trl_refuse(who, "null argument");
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_device_of(d_state));
    k_shots_window_dist<<<(unsigned)((n + SH_THREADS / 64 - 1) / (SH_THREADS / 64)), SH_THREADS, 0, s>>>((const TrlShotsState*)d_state, d_sig, n, H,
                                                                                                         W, prm.drop, d_dist);
    TRL_LAUNCH_CHECK();
    k_shots_scan<<<1, 64, 0, s>>>((TrlShotsState*)d_state, d_sig, d_dist, n, prm.threshold, prm.min_shot, d_cut, d_shot);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

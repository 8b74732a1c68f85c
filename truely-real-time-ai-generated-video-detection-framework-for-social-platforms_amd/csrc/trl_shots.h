// trl_shots.h -- the rules of shot boundaries ("Shots"; section 7, f-15), for host and device alike: the kernels
// of trl_shots.hip and tests/shots_main.cpp run this code, tests/shots_ref.py is its reference.
//
// Every quantity is an INTEGER COUNT or ONE DOUBLE DIVISION, so the bits depend on no banding of a frame, no arrival order, no
// stream, no split of a clip into windows and on nothing a workspace held before.
//
//   signature   of a frame u8 [H][W][3] (channels as stored), 4 <= H, W <= 16384: sig[16][3][32] int32.  Region r = 4 i + j covers
//               rows H i / 4 .. H (i + 1) / 4 - 1 and columns W j / 4 .. W (j + 1) / 4 - 1 (integer division); N_r is its pixel
//               count; sig[r][c][v >> 3] += 1 for every pixel of the region and every channel c
//   distance    of two signatures of the same H x W: per region, with cumulative counts C[c][k] = sum_{b <= k} sig[r][c][b],
//               d_r = sum_c sum_{k = 0 .. 30} |Ca[c][k] - Cb[c][k]| (int64: the 1-D earth mover's distance in bins); the regions in
//               the order (d_r ascending, r ascending), the first 16 - drop kept (the most-changed regions are a moving person,
//               not a cut); D = sum of the kept d_r, M = sum of the kept 93 N_r; dist = (float)((double)D / (double)M) in [0, 1]
//   cuts        dist[t] of a clip's first frame is 2.0 ("no comparison", the drift kernels' sentinel);
//               cut[t] = dist[t] != 2.0 && dist[t] >= threshold && t - last_cut >= min_shot, last_cut the clip's frame of the last
//               cut, -min_shot before the first (the rule never suppresses a first cut); shot[t] = the cuts at frames <= t
//
// The defaults of trl_shots_params are PLACEHOLDERS, not calibrated figures: no labelled set of edited clips has been measured.
#pragma once
#include <stdint.h>

#include "../../include/truely_hip.h"
#include "trl_hd.h"

enum { TRL_SHOTS_GRID = 4, TRL_SHOTS_REGIONS = 16, TRL_SHOTS_CHANNELS = 3, TRL_SHOTS_BINS = 32, TRL_SHOTS_SIG = 16 * 3 * 32 };
#define TRL_SHOTS_MIN_DIM 4
#define TRL_SHOTS_MAX_DIM 16384
#define TRL_SHOTS_MAX_FRAMES 65535           /* frames of one trl_frame_signatures call */
#define TRL_SHOTS_NO_DIST 2.0f               /* "no comparison" */

// The state of a clip: an all-zero state is a clip's start.
struct TrlShotsState {
    long long frames_seen, last_cut, cuts, pad;
    int32_t sig[TRL_SHOTS_SIG];              // the signature of frame frames_seen - 1
};
static_assert(sizeof(TrlShotsState) == TRL_SHOTS_STATE_BYTES, "shots state layout");

TRL_HD trl_shots_params trl_shots_defaults() {
    trl_shots_params p;
    p.threshold = 0.12f, p.drop = 4, p.min_shot = 1;
    return p;
}
TRL_HD bool trl_shots_dim_ok(int H, int W) {
    return H >= TRL_SHOTS_MIN_DIM && H <= TRL_SHOTS_MAX_DIM && W >= TRL_SHOTS_MIN_DIM && W <= TRL_SHOTS_MAX_DIM;
}
TRL_HD bool trl_shots_drop_ok(int drop) { return drop >= 0 && drop < TRL_SHOTS_REGIONS; }
TRL_HD bool trl_shots_params_ok(const trl_shots_params& p) {
    return p.threshold - p.threshold == 0.f && trl_shots_drop_ok(p.drop) && p.min_shot >= 1;
}

// ---- regions ------------------------------------------------------------------------------------------------------------------------
// the first row (column) of band i of a side of `len` pixels; i = 4 gives len
TRL_HD int trl_shots_edge(int len, int i) { return len * i / TRL_SHOTS_GRID; }
// the band of pixel x
TRL_HD int trl_shots_band(int len, int x) {
    return (x >= trl_shots_edge(len, 1)) + (x >= trl_shots_edge(len, 2)) + (x >= trl_shots_edge(len, 3));
}
TRL_HD long long trl_shots_region_pixels(int H, int W, int r) {
    const int i = r / TRL_SHOTS_GRID, j = r % TRL_SHOTS_GRID;
    return (long long)(trl_shots_edge(H, i + 1) - trl_shots_edge(H, i)) * (long long)(trl_shots_edge(W, j + 1) - trl_shots_edge(W, j));
}

// The counts of rows y0 .. y1 - 1 of a frame, added to sig: the host's schedule (the kernel takes bands of a row of regions through
// LDS).  Any split of 0 .. H - 1 into such bands gives the same totals.
inline void trl_shots_accumulate(const uint8_t* frame, int H, int W, int y0, int y1, int32_t* sig) {
    for (int y = y0; y < y1; y++) {
        const int i = trl_shots_band(H, y);
        for (int x = 0; x < W; x++) {
            const int r = TRL_SHOTS_GRID * i + trl_shots_band(W, x);
            const uint8_t* p = frame + ((size_t)y * (size_t)W + (size_t)x) * 3;
            for (int c = 0; c < TRL_SHOTS_CHANNELS; c++) sig[(r * TRL_SHOTS_CHANNELS + c) * TRL_SHOTS_BINS + (p[c] >> 3)] += 1;
        }
    }
}

// ---- distance -----------------------------------------------------------------------------------------------------------------------
// one channel of one region: sum_{k = 0 .. 30} |Ca[k] - Cb[k]| over the 32 bins at a and b
TRL_HD long long trl_shots_channel_emd(const int32_t* a, const int32_t* b) {
    long long ca = 0, cb = 0, d = 0;
    for (int k = 0; k < TRL_SHOTS_BINS - 1; k++) {
        ca += a[k], cb += b[k];
        d += ca > cb ? ca - cb : cb - ca;
    }
    return d;
}
// the regions' d_r -> the distance: region r is kept iff fewer than 16 - drop regions come before it in (d_r, r) order
TRL_HD float trl_shots_distance_of(const long long* d, int H, int W, int drop) {
    long long D = 0, M = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < TRL_SHOTS_REGIONS; r++) {
        int before = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int q = 0; q < TRL_SHOTS_REGIONS; q++) before += d[q] < d[r] || (d[q] == d[r] && q < r);
        if (before < TRL_SHOTS_REGIONS - drop) D += d[r], M += 93 * trl_shots_region_pixels(H, W, r);
    }
    return (float)((double)D / (double)M);
}
// the host's schedule of a whole pair
inline float trl_shots_distance(const int32_t* a, const int32_t* b, int H, int W, int drop) {
    long long d[TRL_SHOTS_REGIONS];
    for (int r = 0; r < TRL_SHOTS_REGIONS; r++) {
        d[r] = 0;
        for (int c = 0; c < TRL_SHOTS_CHANNELS; c++) {
            const int o = (r * TRL_SHOTS_CHANNELS + c) * TRL_SHOTS_BINS;
            d[r] += trl_shots_channel_emd(a + o, b + o);
        }
    }
    return trl_shots_distance_of(d, H, W, drop);
}

// ---- cuts ---------------------------------------------------------------------------------------------------------------------------
// frame t of the clip (its distance to frame t - 1: dist) is a cut; `cuts` and `last_cut` are the clip's so far.  Before the first cut
// last_cut counts as -min_shot, which t - last_cut >= min_shot always passes.
TRL_HD bool trl_shots_is_cut(float dist, float threshold, long long t, long long cuts, long long last_cut, int min_shot) {
    return dist != TRL_SHOTS_NO_DIST && dist >= threshold && (cuts == 0 || t - last_cut >= (long long)min_shot);
}
// The clip's next n frames by their signatures: the host's schedule of trl_shots_update (the kernels take a wave per frame for the
// distances and one wave for the scan).
inline void trl_shots_window(TrlShotsState& st, const int32_t* sig, int n, int H, int W, const trl_shots_params& prm, float* dist,
                             uint8_t* cut, int32_t* shot) {
    for (int t = 0; t < n; t++) {
        const int32_t* cur = sig + (size_t)t * TRL_SHOTS_SIG;
        const long long f = st.frames_seen;
        dist[t] = f == 0 ? TRL_SHOTS_NO_DIST : trl_shots_distance(st.sig, cur, H, W, prm.drop);
        cut[t] = trl_shots_is_cut(dist[t], prm.threshold, f, st.cuts, st.last_cut, prm.min_shot);
        if (cut[t]) st.last_cut = f, st.cuts++;
        shot[t] = (int32_t)st.cuts;
        for (int k = 0; k < TRL_SHOTS_SIG; k++) st.sig[k] = cur[k];
        st.frames_seen = f + 1;
    }
}

// trl_quality.h -- the rules of face quality ("Face quality"; section 7, f-14), for host and device alike: the
// kernels of trl_quality.hip and tests/quality_main.cpp run this code, tests/quality_ref.py is its reference.
//
// Every measure is either an INTEGER SUM over the source pixels of a face's rectangle or a SHORT FLOAT CHAIN in the order written
// below, made of + - * / sqrt alone.  Integers add associatively, so the raw sums -- and everything computed from them -- are the
// same bits for any banding of the rectangle, any arrival order and any stream; there is no transcendental function, so no host and
// device libm to disagree.  Every float operation rounds once (the build has -ffp-contract=off).
//
// The two image rules are OpenCV's as recalled, UNPINNED (no cv2 where this was written): the luma is the 8-bit COLOR_BGR2GRAY,
// the Laplacian is cv2.Laplacian(gray_crop, CV_64F) with ksize=1 and the default reflect-101 border.
//
// The defaults of trl_quality_params are PLACEHOLDERS, not calibrated figures: no labelled set of good and bad faces has been
// measured.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/truely_hip.h"
#include "trl_hd.h"

enum { TRL_QUALITY_RAW = 8, TRL_QUALITY_FEAT = 12, TRL_QUALITY_BINS = 256 };
// raw[8], int64
enum { TRL_QR_N = 0, TRL_QR_SY, TRL_QR_SY2, TRL_QR_SL, TRL_QR_SL2, TRL_QR_DARK, TRL_QR_BRIGHT, TRL_QR_WIDTH };
// feat[12], float32
enum { TRL_QF_QUALITY = 0, TRL_QF_SHARPNESS, TRL_QF_MEAN_LUMA, TRL_QF_DARK_FRAC, TRL_QF_BRIGHT_FRAC, TRL_QF_CONTRAST, TRL_QF_YAW,
       TRL_QF_PITCH, TRL_QF_ROLL, TRL_QF_IOD, TRL_QF_P05, TRL_QF_P95 };
#define TRL_QUALITY_MAX_DIM 16384            /* H and W of a frame: a rectangle's row of luma fits the kernels' LDS three times */
#define TRL_QUALITY_MAX_ROWS (1LL << 24)     /* face rows of one call */

TRL_HD trl_quality_params trl_quality_defaults() {
    trl_quality_params p;
    p.sharp_ref = 100.f, p.clip_ref = 0.5f, p.contrast_ref = 64.f, p.yaw_ref = 1.f, p.pitch_ref = 1.f, p.size_ref = 80.f;
    return p;
}
// every reference is a divisor: finite and > 0
TRL_HD bool trl_quality_ref_ok(float v) { return v > 0.f && v - v == 0.f; }
TRL_HD bool trl_quality_params_ok(const trl_quality_params& p) {
    return trl_quality_ref_ok(p.sharp_ref) && trl_quality_ref_ok(p.clip_ref) && trl_quality_ref_ok(p.contrast_ref) &&
           trl_quality_ref_ok(p.yaw_ref) && trl_quality_ref_ok(p.pitch_ref) && trl_quality_ref_ok(p.size_ref);
}

// ---- the rectangle ------------------------------------------------------------------------------------------------------------------
// clamp((int)v, 0, len) of an integral float v, without converting what an int cannot hold
TRL_HD int trl_quality_clamp(float v, int len) { return v <= 0.f ? 0 : v >= (float)len ? len : (int)v; }
// rect = X0, Y0, X1, Y1: columns X0 .. X1 - 1 and rows Y0 .. Y1 - 1 of frame frame_of.  0 (and a zero rect) for no face: a frame
// index outside 0 .. n - 1, a NaN or infinite coordinate, or an empty rectangle
TRL_HD int trl_quality_rect(int frame_of, int n, int H, int W, const float* box, int* rect) {
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    if (frame_of < 0 || frame_of >= n) return 0;
    if (!(box[0] - box[0] == 0.f && box[1] - box[1] == 0.f && box[2] - box[2] == 0.f && box[3] - box[3] == 0.f)) return 0;
    const int X0 = trl_quality_clamp(__builtin_floorf(box[0]), W), X1 = trl_quality_clamp(__builtin_ceilf(box[2]), W);
    const int Y0 = trl_quality_clamp(__builtin_floorf(box[1]), H), Y1 = trl_quality_clamp(__builtin_ceilf(box[3]), H);
    if (X1 <= X0 || Y1 <= Y0) return 0;
    rect[0] = X0, rect[1] = Y0, rect[2] = X1, rect[3] = Y1;
    return 1;
}

// ---- the pixel rules ----------------------------------------------------------------------------------------------------------------
TRL_HD int trl_quality_luma(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }
// reflect-101 inside 0 .. len - 1 for i in -1 .. len: -1 -> 1, len -> len - 2; a single sample is its own neighbour
TRL_HD int trl_quality_reflect(int i, int len) { return len == 1 ? 0 : i < 0 ? 1 : i >= len ? len - 2 : i; }
TRL_HD int trl_quality_laplacian(int c, int up, int down, int left, int right) { return up + down + left + right - 4 * c; }

// The sums of rows y0 .. y1 - 1 of the rectangle (rows of the RECTANGLE: 0 .. h - 1), added to hist[256], *sl and *sl2: the host's
// schedule (the kernels take a band through LDS).  Any split of 0 .. h - 1 into such bands gives the same totals.
inline void trl_quality_accumulate(const uint8_t* frame, int W, const int* rect, int y0, int y1, int32_t* hist, long long* sl,
                                   long long* sl2) {
    const int w = rect[2] - rect[0], h = rect[3] - rect[1];
    for (int y = y0; y < y1; y++)
        for (int x = 0; x < w; x++) {
            int v[5];
            const int yy[5] = {y, trl_quality_reflect(y - 1, h), trl_quality_reflect(y + 1, h), y, y};
            const int xx[5] = {x, x, x, trl_quality_reflect(x - 1, w), trl_quality_reflect(x + 1, w)};
            for (int i = 0; i < 5; i++) {
                const uint8_t* p = frame + ((size_t)(rect[1] + yy[i]) * (size_t)W + (size_t)(rect[0] + xx[i])) * 3;
                v[i] = trl_quality_luma(p[0], p[1], p[2]);
            }
            const int L = trl_quality_laplacian(v[0], v[1], v[2], v[3], v[4]);
            hist[v[0]] += 1;
            *sl += L;
            *sl2 += (long long)L * L;
        }
}

// ---- the raw integers ---------------------------------------------------------------------------------------------------------------
// N, the sums of Y and Y^2 and the clipped counts are functions of the histogram (the kernels read them off it): raw[0 .. 7], p[0]
// = p05 and p[1] = p95.  p05 is the smallest v with 20 cum(v) >= N, p95 the smallest with 20 cum(v) >= 19 N.
TRL_HD void trl_quality_raw(const int32_t* hist, long long sl, long long sl2, int width, long long* raw, int* p) {
    long long n = 0, sy = 0, sy2 = 0, dark = 0, bright = 0;
    for (int v = 0; v < TRL_QUALITY_BINS; v++) {
        const long long c = hist[v];
        n += c, sy += c * v, sy2 += c * v * v;
        if (v <= 15) dark += c;
        if (v >= 240) bright += c;
    }
    long long cum = 0;
    p[0] = p[1] = -1;
    for (int v = 0; v < TRL_QUALITY_BINS; v++) {
        cum += hist[v];
        if (p[0] < 0 && 20 * cum >= n) p[0] = v;
        if (p[1] < 0 && 20 * cum >= 19 * n) p[1] = v;
    }
    raw[TRL_QR_N] = n, raw[TRL_QR_SY] = sy, raw[TRL_QR_SY2] = sy2, raw[TRL_QR_SL] = sl, raw[TRL_QR_SL2] = sl2;
    raw[TRL_QR_DARK] = dark, raw[TRL_QR_BRIGHT] = bright, raw[TRL_QR_WIDTH] = width;
}

// ---- the float chains ---------------------------------------------------------------------------------------------------------------
// pose[4] = yaw, pitch, roll, iod from pts = x0..x4, y0..y4 (left eye, right eye, nose, mouth left, mouth right).  Ratios, not
// angles: there is no atan.  With e = eyeR - eyeL and "iod^2" the sum e.e BEFORE its square root:
//   iod = sqrtf(e.e);  roll = e.y / iod;  yaw = 2 ((nose - eyeL).e / e.e) - 1
//   pitch = 2 ((nose - eyeMid).v / v.v) - 1,  v = mouthMid - eyeMid, the mids (a + b) * 0.5f
// a dot product is (ax * bx) + (ay * by).  All four are NaN when a point is not finite or e.e or v.v is 0.
TRL_HD void trl_quality_pose(const float* pts, float* pose) {
    const float nan = __builtin_nanf("");
    pose[0] = pose[1] = pose[2] = pose[3] = nan;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 10; i++) finite = finite && pts[i] - pts[i] == 0.f;
    if (!finite) return;
    const float ex = pts[1] - pts[0], ey = pts[6] - pts[5];
    const float e2 = ex * ex + ey * ey;
    const float mx = (pts[0] + pts[1]) * 0.5f, my = (pts[5] + pts[6]) * 0.5f;
    const float vx = (pts[3] + pts[4]) * 0.5f - mx, vy = (pts[8] + pts[9]) * 0.5f - my;
    const float v2 = vx * vx + vy * vy;
    if (e2 == 0.f || v2 == 0.f) return;
    const float iod = __builtin_sqrtf(e2);
    const float t = ((pts[2] - pts[0]) * ex + (pts[7] - pts[5]) * ey) / e2;
    const float u = ((pts[2] - mx) * vx + (pts[7] - my) * vy) / v2;
    pose[0] = 2.f * t - 1.f;
    pose[1] = 2.f * u - 1.f;
    pose[2] = ey / iod;
    pose[3] = iod;
}

TRL_HD float trl_quality_unit_min(float v) { return v > 1.f ? 1.f : v; }            // min(v, 1)
TRL_HD float trl_quality_pos(float v) { return v > 0.f ? v : 0.f; }                  // max(0, v); NaN -> 0
TRL_HD float trl_quality_abs(float v) { return v < 0.f ? -v : v; }

// One face: feat[12] from its raw integers, the percentiles, its rectangle's height and its points (read when has_pts).  status 0:
// all +0.
//   sharpness  = (float)((double)SL2 / N - ((double)SL / N) * ((double)SL / N))                     the variance of the Laplacian
//   mean_luma  = (float)((double)SY / N);  dark_frac, bright_frac = (float)((double)count / N);  contrast = (float)(p95 - p05)
//   q_sharp    = min(max(0, sharpness) / sharp_ref, 1)          (the double chain can end a rounding below 0)
//   q_expo     = max(0, 1 - (dark_frac + bright_frac) / clip_ref) * min(contrast / contrast_ref, 1)
//   q_pose     = max(0, 1 - |yaw| / yaw_ref) * max(0, 1 - |pitch| / pitch_ref);  0 when either is NaN, 1 without points
//   q_size     = min((float)min(w, h) / size_ref, 1)
//   quality    = ((q_sharp * q_expo) * q_pose) * q_size
TRL_HD void trl_quality_features(int status, const long long* raw, const int* p, int height, bool has_pts, const float* pts,
                                    const trl_quality_params& prm, float* feat) {
#pragma unroll
    for (int i = 0; i < TRL_QUALITY_FEAT; i++) feat[i] = 0.f;
    if (!status) return;
    const double n = (double)raw[TRL_QR_N];
    const double a = (double)raw[TRL_QR_SL2] / n, b = (double)raw[TRL_QR_SL] / n;
    const double bb = b * b;
    const float sharp = (float)(a - bb);
    const float mean = (float)((double)raw[TRL_QR_SY] / n);
    const float dark = (float)((double)raw[TRL_QR_DARK] / n), bright = (float)((double)raw[TRL_QR_BRIGHT] / n);
    const float contrast = (float)(p[1] - p[0]);
    const float nan = __builtin_nanf("");
    float pose[4] = {nan, nan, nan, nan};
    float q_pose = 1.f;
    if (has_pts) {
        trl_quality_pose(pts, pose);
        q_pose = trl_quality_pos(1.f - trl_quality_abs(pose[0]) / prm.yaw_ref) * trl_quality_pos(1.f - trl_quality_abs(pose[1]) / prm.pitch_ref);
    }
    const float q_sharp = trl_quality_unit_min(trl_quality_pos(sharp) / prm.sharp_ref);
    const float q_expo = trl_quality_pos(1.f - (dark + bright) / prm.clip_ref) * trl_quality_unit_min(contrast / prm.contrast_ref);
    const int width = (int)raw[TRL_QR_WIDTH];
    const float q_size = trl_quality_unit_min((float)(width < height ? width : height) / prm.size_ref);
    feat[TRL_QF_QUALITY] = q_sharp * q_expo * q_pose * q_size;
    feat[TRL_QF_SHARPNESS] = sharp, feat[TRL_QF_MEAN_LUMA] = mean, feat[TRL_QF_DARK_FRAC] = dark, feat[TRL_QF_BRIGHT_FRAC] = bright;
    feat[TRL_QF_CONTRAST] = contrast;
    feat[TRL_QF_YAW] = pose[0], feat[TRL_QF_PITCH] = pose[1], feat[TRL_QF_ROLL] = pose[2], feat[TRL_QF_IOD] = pose[3];
    feat[TRL_QF_P05] = (float)p[0], feat[TRL_QF_P95] = (float)p[1];
}

// ---- best shots -----------------------------------------------------------------------------------------------------------------------
// The best row of a group is the one with the largest trl_best_key(quality, absolute row) (trl_bestkey.h): the larger quality, ties as
// floats (-0 == +0) to the lower row, a NaN never a candidate, key 0 for none.

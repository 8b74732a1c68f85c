// trl_extract.hip -- facenet-pytorch 2.6.0 face extraction (MTCNN.forward after detect): select_boxes and extract_face
// (crop with margin, crop_resize by input kind, post-processing), batched and device-resident.
//
// Semantics restated from the feature issue "Add MTCNN face extraction on the GPU" (facenet-pytorch 2.6.0, recalled: no copy of
// the library is installed), test restatement tests/extract_ref.py:
//   k_pick_faces   : select_boxes(threshold 0.9, center_weight 2.0), one frame per thread, ties -> last tied box in detect's order
//   k_extract_plan : one workgroup per face: the crop box (margin in f64 from the f32 box, clamp, int()), the row status and the
//                    separable coefficient tables of the resampler (Pillow BILINEAR, OpenCV INTER_AREA) into a workspace
//   k_extract      : one workgroup per (face, band of output rows): torch = imresample (area) per pixel through trl_area_pixel
//                    (the code trl_crops.hip's k_crop_area_std runs), cv2 integer scales = block means, else the two separable passes with the
//                    horizontal pass staged in LDS, chunk by chunk of the vertical taps.  Pillow's Image.resize runs the vertical
//                    pass first for a crop more than 100 times as tall as wide that it shrinks vertically (ih > 100 * iw and
//                    S < ih; both passes round to 8 bits, so the order shows in the bytes): such a crop takes that order here
// The double-precision coefficient arithmetic relies on -ffp-contract=off (csrc/Makefile), like the rest of the library.
#include "trl_ctx.h"
#include <float.h>

namespace {

constexpr int XB = 256;                 // threads of an extraction workgroup
constexpr int XBAND = 8;                // output rows per workgroup
constexpr int XACC = 12;                // output values of one row per thread: 3 * 1024 / 256
constexpr int XTMP = 16384;             // LDS words for horizontal-pass rows (64 KB)
constexpr int HDR = 8;                  // plan header words: x0 y0 iw ih status mode kx ky (mode: CV_* for cv2, PIL_* for pil)

enum { R_TORCH = 0, R_PIL = 1, R_CV2 = 2 };
enum { CV_FAST = 0, CV_AREA = 1, CV_LINEAR = 2 };
enum { PIL_HFIRST = 0, PIL_VFIRST = 1 };

// ---- select_boxes --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pick_faces(int n, int max_faces, const float* __restrict__ boxes, const float* __restrict__ probs,
                                                   const int32_t* __restrict__ counts, int W, int H, int method, float thr, double cw,
                                                   int32_t* __restrict__ pick) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    int k = counts[f];
    k = k < 0 ? 0 : (k > max_faces ? max_faces : k);
    const float* b = boxes + (size_t)f * max_faces * 4;
    const float* p = probs + (size_t)f * max_faces;
    int best = -1;
    double bk = 0.;
    for (int q = 0; q < k; q++) {
        const float* bq = b + 4 * q;
        const float area = (bq[2] - bq[0]) * (bq[3] - bq[1]);
        double key;
        if (method == 1) key = (double)p[q];
        else if (method == 3) {
            const double dx = (double)((bq[0] + bq[2]) / 2.f) - (double)W / 2., dy = (double)((bq[1] + bq[3]) / 2.f) - (double)H / 2.;
            key = (double)area - (dx * dx + dy * dy) * cw;
        } else {
            if (method == 2 && !(p[q] > thr)) continue;
            key = (double)area;                                    // exact: f32 -> f64
        }
        if (best < 0 || key >= bk) { best = q; bk = key; }        // >=: the last tied box wins (reversed stable argsort)
    }
    pick[f] = best;
}

// ---- coefficient tables ------------------------------------------------------------------------------------------------------
// One axis of n source pixels -> S outputs.  lo[o], cnt[o]: the source taps of output o; w[o * K + t]: tap weights (int bits of
// Pillow's 22-bit fixed point, f32 bits of OpenCV's resizeArea table, or the 2048-scaled shorts of OpenCV's linear path).
__device__ void pil_axis(int n, int S, int K, int32_t* lo, int32_t* cnt, int32_t* w) {
    const double scale = (double)n / S, fs = scale > 1. ? scale : 1., ss = 1. / fs;
    for (int o = threadIdx.x; o < S; o += blockDim.x) {
        const double center = (o + 0.5) * scale;
        int a = (int)(center - fs + 0.5), b = (int)(center + fs + 0.5);
        a = a < 0 ? 0 : a;
        b = b > n ? n : b;
        int c = b - a;
        c = c > K ? K : c;                                     // never: K bounds 2*fs+1 (host)
        double ww = 0.;
        for (int t = 0; t < c; t++) {
            const double x = fabs(((double)(t + a) - center + 0.5) * ss);
            ww += x < 1. ? 1. - x : 0.;
        }
        for (int t = 0; t < c; t++) {
            const double x = fabs(((double)(t + a) - center + 0.5) * ss);
            double k = x < 1. ? 1. - x : 0.;
            if (ww != 0.) k /= ww;
            w[o * K + t] = k < 0. ? (int32_t)(-0.5 + k * 4194304.) : (int32_t)(0.5 + k * 4194304.);
        }
        lo[o] = a; cnt[o] = c;
    }
}

// OpenCV 4.x computeResizeAreaTab (scale = 1 / (S / n), as resize() forms it), one output per thread, taps in table order.
__device__ void cv_area_axis(int n, int S, int K, int32_t* lo, int32_t* cnt, int32_t* w) {
    const double scale = 1. / ((double)S / n);
    for (int o = threadIdx.x; o < S; o += blockDim.x) {
        const double f1 = o * scale, f2 = f1 + scale;
        const double cell = scale < n - f1 ? scale : n - f1;
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        s2 = s2 < n - 1 ? s2 : n - 1;
        s1 = s1 < s2 ? s1 : s2;
        int c = 0, a = s1;
        if (s1 - f1 > 1e-3) { a = s1 - 1; w[o * K + c++] = __float_as_int((float)((s1 - f1) / cell)); }
        for (int s = s1; s < s2 && c < K; s++) w[o * K + c++] = __float_as_int((float)(1.0 / cell));
        if (f2 - s2 > 1e-3 && c < K) {
            const double r = f2 - s2 < 1. ? f2 - s2 : 1.;
            w[o * K + c++] = __float_as_int((float)((r < cell ? r : cell) / cell));
        }
        lo[o] = a; cnt[o] = c;
    }
}

// OpenCV's generic resize with INTER_AREA coefficients (an axis that is upscaled): sx = floor(o * scale),
// fx = (o + 1) - (sx + 1) * inv_scale, fx <= 0 ? 0 : fx - floor(fx), shorts (1 - fx) * 2048, fx * 2048; the right edge clamps.
__device__ void cv_linear_axis(int n, int S, int K, int32_t* lo, int32_t* cnt, int32_t* w) {
    const double inv = (double)S / n, scale = 1. / inv;
    for (int o = threadIdx.x; o < S; o += blockDim.x) {
        int sx = (int)floor(o * scale);
        float fx = (float)((o + 1) - (sx + 1) * inv);
        fx = fx <= 0.f ? 0.f : fx - (float)(int)floorf(fx);
        if (sx >= n - 1) { sx = n - 1; fx = 0.f; }
        lo[o] = sx; cnt[o] = 2;
        w[o * K] = (int32_t)__builtin_rintf((1.f - fx) * 2048.f);
        w[o * K + 1] = (int32_t)__builtin_rintf(fx * 2048.f);
    }
}

__global__ __launch_bounds__(256) void k_extract_plan(int n, int H, int W, const int32_t* __restrict__ frame_of, const float* __restrict__ boxes,
                                                      int S, int margin, int resample, int Kx, int Ky, int32_t* __restrict__ plan,
                                                      int32_t* __restrict__ status) {
    const int r = blockIdx.x;
    int32_t* P = plan + (size_t)r * (HDR + (size_t)S * (4 + Kx + Ky));
    __shared__ int32_t hd[HDR];
    if (threadIdx.x == 0) {
        const int f = frame_of[r];
        int x0 = 0, y0 = 0, x1 = 0, y1 = 0, st = 0;
        if (f >= 0 && f < n) {
            // extract_face: margin * (x2 - x1) / (S - margin) in f64 from the f32 box; int(max(x1 - mx/2, 0)), int(min(x2 + mx/2, W))
            const float bx1 = boxes[4 * r], by1 = boxes[4 * r + 1], bx2 = boxes[4 * r + 2], by2 = boxes[4 * r + 3];
            const double mx = (double)margin * (double)(bx2 - bx1) / (double)(S - margin);
            const double my = (double)margin * (double)(by2 - by1) / (double)(S - margin);
            const double a0 = (double)bx1 - mx / 2., b0 = (double)by1 - my / 2., a1 = (double)bx2 + mx / 2., b1 = (double)by2 + my / 2.;
            x0 = (int)(a0 > 0. ? a0 : 0.); y0 = (int)(b0 > 0. ? b0 : 0.);
            x1 = (int)(a1 < (double)W ? a1 : (double)W); y1 = (int)(b1 < (double)H ? b1 : (double)H);
            st = (x1 > x0 && y1 > y0) ? 1 : -1;
        }
        const int iw = st == 1 ? x1 - x0 : 0, ih = st == 1 ? y1 - y0 : 0;
        int mode = CV_FAST, kx = 0, ky = 0;
        if (st == 1 && resample == R_CV2) {
            // resize(): scale = 1 / inv_scale; resizeAreaFast when both are >= 1 and within DBL_EPSILON of integers
            const double sx = 1. / ((double)S / iw), sy = 1. / ((double)S / ih);
            kx = (int)__builtin_rint(sx); ky = (int)__builtin_rint(sy);
            if (sx >= 1. && sy >= 1.) mode = (fabs(sx - kx) < DBL_EPSILON && fabs(sy - ky) < DBL_EPSILON) ? CV_FAST : CV_AREA;
            else mode = CV_LINEAR;
        }
        // Image.resize (Pillow 12.2, Image.py): "if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]" resizes vertically first
        if (st == 1 && resample == R_PIL) mode = (ih > iw * 100 && S < ih) ? PIL_VFIRST : PIL_HFIRST;
        hd[0] = x0; hd[1] = y0; hd[2] = iw; hd[3] = ih; hd[4] = st; hd[5] = mode; hd[6] = kx; hd[7] = ky;
        if (status) status[r] = st;
    }
    __syncthreads();
    if (threadIdx.x < HDR) P[threadIdx.x] = hd[threadIdx.x];
    if (hd[4] != 1 || resample == R_TORCH || (resample == R_CV2 && hd[5] == CV_FAST)) return;
    int32_t* X = P + HDR;
    int32_t* Y = X + (size_t)S * (2 + Kx);
    if (resample == R_PIL) {
        pil_axis(hd[2], S, Kx, X, X + S, X + 2 * S);
        pil_axis(hd[3], S, Ky, Y, Y + S, Y + 2 * S);
    } else if (hd[5] == CV_AREA) {
        cv_area_axis(hd[2], S, Kx, X, X + S, X + 2 * S);
        cv_area_axis(hd[3], S, Ky, Y, Y + S, Y + 2 * S);
    } else {
        cv_linear_axis(hd[2], S, Kx, X, X + S, X + 2 * S);
        cv_linear_axis(hd[3], S, Ky, Y, Y + S, Y + 2 * S);
    }
}

__device__ __forceinline__ float post(float v, int post_process) { return post_process ? (v - 127.5f) / 128.0f : v; }

__global__ __launch_bounds__(XB) void k_extract(int H, int W, const uint8_t* __restrict__ frames, const int32_t* __restrict__ frame_of, int S,
                                                int resample, int post_process, int Kx, int Ky, const int32_t* __restrict__ plan,
                                                float* __restrict__ out) {
    __shared__ int32_t tmp[XTMP];
    const int r = blockIdx.y;
    const int32_t* P = plan + (size_t)r * (HDR + (size_t)S * (4 + Kx + Ky));
    const int oy0 = blockIdx.x * XBAND, oy1 = oy0 + XBAND < S ? oy0 + XBAND : S;
    const int rowlen = 3 * S;
    float* o = out + (size_t)r * S * rowlen;
    const int x0 = P[0], y0 = P[1], iw = P[2], ih = P[3], st = P[4], mode = P[5];
    if (st != 1) {                                            // no face / empty crop: zeros
        for (int e = oy0 * rowlen + threadIdx.x; e < oy1 * rowlen; e += XB) o[e] = 0.f;
        return;
    }
    const uint8_t* fp = frames + (size_t)frame_of[r] * H * W * 3;
    if (resample == R_TORCH) {                                // imresample (area) + .byte(): k_crop_area_std's pixel
        for (int q = oy0 * S + threadIdx.x; q < oy1 * S; q += XB) {
            const int oy = q / S, ox = q - oy * S;
            float v[3];
            trl_area_pixel(fp, W, x0, y0, iw, ih, S, ox, oy, v);
            o[3 * q] = post(v[0], post_process); o[3 * q + 1] = post(v[1], post_process); o[3 * q + 2] = post(v[2], post_process);
        }
        return;
    }
    if (resample == R_CV2 && mode == CV_FAST) {               // resizeAreaFast: integer block sums
        const int kx = P[6], ky = P[7];
        const float inv = 1.f / (float)(kx * ky);
        for (int e = oy0 * rowlen + threadIdx.x; e < oy1 * rowlen; e += XB) {
            const int oy = e / rowlen, q = e - oy * rowlen, ox = q / 3, c = q - 3 * ox;
            int s = 0;
            for (int y = 0; y < ky; y++) {
                const uint8_t* row = fp + ((size_t)(y0 + oy * ky + y) * W + x0 + (size_t)ox * kx) * 3 + c;
                for (int x = 0; x < kx; x++) s += row[3 * x];
            }
            int v;
            if (kx == 2 && ky == 2) v = (s + 2) >> 2;
            else {
                v = (int)__builtin_rintf((float)s * inv);
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
            }
            o[e] = post((float)v, post_process);
        }
        return;
    }
    // separable passes: per output row, the horizontal pass of its vertical taps goes to LDS (in chunks of T rows), then every
    // thread accumulates its output values of the row over those taps in tap order
    const int32_t *Xlo = P + HDR, *Xcnt = Xlo + S, *Xw = Xlo + 2 * S;
    const int32_t *Ylo = Xlo + (size_t)S * (2 + Kx), *Ycnt = Ylo + S, *Yw = Ylo + 2 * S;
    if (resample == R_PIL && mode == PIL_VFIRST) {
        // vertical pass first: ih > 100 * iw and ih <= 16383 leave iw <= 163 columns, so the vertically filtered row (3 * iw
        // values, rounded and clipped to 8 bits) is one short LDS row and the vertical taps need no chunks
        const int srclen = 3 * iw;
        for (int oy = oy0; oy < oy1; oy++) {
            const int ylo = Ylo[oy], ycnt = Ycnt[oy];
            const int32_t* yw = Yw + (size_t)oy * Ky;
            __syncthreads();                                  // the previous row's readers are done
            for (int e = threadIdx.x; e < srclen; e += XB) {
                const uint8_t* col = fp + ((size_t)(y0 + ylo) * W + x0) * 3 + e;
                int a = 1 << 21;
                for (int t = 0; t < ycnt; t++) a += yw[t] * (int)col[(size_t)t * W * 3];
                a >>= 22;
                tmp[e] = a < 0 ? 0 : (a > 255 ? 255 : a);
            }
            __syncthreads();
            float* orow = o + (size_t)oy * rowlen;
            for (int p = threadIdx.x; p < rowlen; p += XB) {
                const int ox = p / 3, c = p - 3 * ox, xl = Xlo[ox], xc = Xcnt[ox];
                const int32_t* xw = Xw + (size_t)ox * Kx;
                int a = 1 << 21;
                for (int t = 0; t < xc; t++) a += xw[t] * tmp[3 * (xl + t) + c];
                a >>= 22;
                orow[p] = post((float)(a < 0 ? 0 : (a > 255 ? 255 : a)), post_process);
            }
        }
        return;
    }
    const int T = XTMP / rowlen;
    const int kind = resample == R_PIL ? 0 : (mode == CV_AREA ? 1 : 2);
    for (int oy = oy0; oy < oy1; oy++) {
        const int ylo = Ylo[oy], ycnt = Ycnt[oy];
        const int32_t* yw = Yw + (size_t)oy * Ky;
        int ia[XACC];
        float fa[XACC];
#pragma unroll
        for (int k = 0; k < XACC; k++) { ia[k] = kind == 0 ? (1 << 21) : 0; fa[k] = 0.f; }
        for (int t0 = 0; t0 < ycnt; t0 += T) {
            const int tc = ycnt - t0 < T ? ycnt - t0 : T;
            __syncthreads();                                  // the previous chunk's readers are done
            for (int e = threadIdx.x; e < tc * rowlen; e += XB) {
                const int tt = e / rowlen, q = e - tt * rowlen, ox = q / 3, c = q - 3 * ox;
                int sy = ylo + t0 + tt;
                sy = sy < ih - 1 ? sy : ih - 1;
                const uint8_t* row = fp + ((size_t)(y0 + sy) * W + x0) * 3 + c;
                const int xl = Xlo[ox], xc = Xcnt[ox];
                const int32_t* xw = Xw + (size_t)ox * Kx;
                if (kind == 0) {                              // Pillow: 22-bit fixed point, rounded and clipped to 8 bits
                    int a = 1 << 21;
                    for (int t = 0; t < xc; t++) a += xw[t] * (int)row[3 * (xl + t)];
                    a >>= 22;
                    tmp[e] = a < 0 ? 0 : (a > 255 ? 255 : a);
                } else if (kind == 1) {                       // OpenCV resizeArea: f32 sums in table order
                    float a = 0.f;
                    for (int t = 0; t < xc; t++) a = a + (float)row[3 * (xl + t)] * __int_as_float(xw[t]);
                    tmp[e] = __float_as_int(a);
                } else {                                      // OpenCV linear fixed point (right edge clamped)
                    int a = 0;
                    for (int t = 0; t < xc; t++) {
                        const int sx = xl + t < iw - 1 ? xl + t : iw - 1;
                        a += (int)row[3 * sx] * xw[t];
                    }
                    tmp[e] = a;
                }
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < XACC; k++) {
                const int p = threadIdx.x + k * XB;
                if (p < rowlen) {
                    for (int tt = 0; tt < tc; tt++) {
                        const int wv = yw[t0 + tt], hv = tmp[tt * rowlen + p];
                        if (kind == 0) ia[k] += wv * hv;
                        else if (kind == 1) fa[k] = fa[k] + __int_as_float(wv) * __int_as_float(hv);
                        else ia[k] += (wv * (hv >> 4)) >> 16;
                    }
                }
            }
        }
        float* orow = o + (size_t)oy * rowlen;
#pragma unroll
        for (int k = 0; k < XACC; k++) {
            const int p = threadIdx.x + k * XB;
            if (p < rowlen) {
                int v;
                if (kind == 0) v = ia[k] >> 22;
                else if (kind == 1) v = (int)__builtin_rintf(fa[k]);  // saturate_cast<uchar>: round half to even
                else v = (ia[k] + 2) >> 2;
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
                orow[p] = post((float)v, post_process);
            }
        }
    }
}

}  // namespace

extern "C" {

int trl_select_faces(trl_ctx* c, int n, const float* d_boxes, const float* d_probs, const int32_t* d_counts, int H, int W, int method,
                     float threshold, double center_weight, int32_t* d_pick, void* stream) {
    TRL_CHECK(trl_check_idle(c));
    if (!d_boxes || !d_probs || !d_counts || !d_pick) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    if (n <= 0 || n > 65535 || H < 1 || W < 1 || method < 0 || method > 3) {
        trl_set_error("bad selection n=%d H=%d W=%d method=%d", n, H, W, method);
        return TRL_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    TRL_HIP(hipSetDevice(c->cfg.device));
    k_pick_faces<<<(n + 63) / 64, 64, 0, s>>>(n, c->cfg.max_faces, d_boxes, d_probs, d_counts, W, H, method, threshold, center_weight, d_pick);
    TRL_LAUNCH_CHECK();
    return trl_gate_record(c, s);
}

int trl_extract_faces(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, const int32_t* d_frame_of, const float* d_boxes, int m,
                      int S, int margin, int resample, int post_process, float* d_out, int32_t* d_status, void* stream) {
    TRL_CHECK(trl_check_idle(c));
    if (!d_frames || ((!d_frame_of || !d_boxes || !d_out) && m != 0)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    if (n <= 0 || n > 65535 || H < 1 || W < 1 || H > 16383 || W > 16383 || m < 0 || m > 65535) {
        trl_set_error("bad extraction batch n=%d H=%d W=%d m=%d", n, H, W, m);
        return TRL_ERR_INVALID;
    }
    if (S < 1 || S > 1024 || margin < 0 || margin >= S || resample < 0 || resample > 2 || (post_process != 0 && post_process != 1)) {
        trl_set_error("bad extraction parameters S=%d margin=%d resample=%d post_process=%d (1 <= S <= 1024, 0 <= margin < S)", S, margin,
                      resample, post_process);
        return TRL_ERR_INVALID;
    }
    if (m == 0) return TRL_OK;
    hipStream_t s = (hipStream_t)stream;
    TRL_HIP(hipSetDevice(c->cfg.device));
    // taps per output: Pillow <= 2 * max(n / S, 1) + 1, OpenCV's area table <= ceil(n / S) + 2, its linear path 2
    const int fx = (W + S - 1) / S, fy = (H + S - 1) / S;
    const int Kx = 2 * (fx > 1 ? fx : 1) + 3, Ky = 2 * (fy > 1 ? fy : 1) + 3;
    const size_t words = HDR + (size_t)S * (4 + Kx + Ky);
    TRL_CHECK(trl_scratch_begin(c, (size_t)m * words * 4 + 4096));   // stream order: earlier users of the scratch arena are done before these kernels run
    int32_t* plan = (int32_t*)c->scratch.alloc((size_t)m * words * 4);
    if (!plan) { trl_set_error("arena exhausted"); return TRL_ERR_STATE; }
    k_extract_plan<<<m, 256, 0, s>>>(n, H, W, d_frame_of, d_boxes, S, margin, resample, Kx, Ky, plan, d_status);
    TRL_LAUNCH_CHECK();
    k_extract<<<dim3((S + XBAND - 1) / XBAND, m), XB, 0, s>>>(H, W, d_frames, d_frame_of, S, resample, post_process, Kx, Ky, plan, d_out);
    TRL_LAUNCH_CHECK();
    TRL_CHECK(trl_gate_record(c, s));
    return trl_rz_end(c, "extract_faces");
}

}  // extern "C"

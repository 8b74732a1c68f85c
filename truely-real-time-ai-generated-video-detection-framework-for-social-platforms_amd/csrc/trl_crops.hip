// trl_crops.hip -- the face crops between the cascade and the embedder (gfx950): the largest face's rectangle (or its five
// landmarks) of every frame -> the embedder's input.  Three modes: model.py's cv2.resize to 80 x 80, facenet-pytorch's
// extract_face (area resample + fixed_image_standardization), and this project's landmark-aligned crop.
#include "trl_ctx.h"

namespace {

// model.py:55-58: frame[y0:y1, x0:x1] -> cv2.resize(.., (80,80)) INTER_LINEAR (u8 fixed point) -> /255
__device__ __forceinline__ int sat_short_round(float v) {
    int r = (int)__builtin_rintf(v);
    return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}
__global__ __launch_bounds__(256) void k_crop_resize80(const uint8_t* __restrict__ frames, int H, int W, const int32_t* __restrict__ rect,
                                                       const uint8_t* __restrict__ valid, float* __restrict__ out) {
    constexpr int O = 80;
    __shared__ int xofs[O], xofs1[O], a0[O], a1[O], ys0[O], ys1[O], b0[O], b1[O];
    const int f = blockIdx.x;
    float* o = out + (size_t)f * O * O * 3;
    if (!valid[f]) {
        for (int p = threadIdx.x; p < O * O * 3; p += blockDim.x) o[p] = 0.f;
        return;
    }
    const int x0 = rect[4 * f], y0 = rect[4 * f + 1], sw = rect[4 * f + 2] - x0, sh = rect[4 * f + 3] - y0;
    const double scale_x = 1. / ((double)O / sw), scale_y = 1. / ((double)O / sh);
    if (threadIdx.x < O) {
        const int d = threadIdx.x;
        float fx = (float)((d + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        xofs[d] = sx; xofs1[d] = sx + 1 > sw - 1 ? sw - 1 : sx + 1;
        a0[d] = sat_short_round((1.f - fx) * 2048.f); a1[d] = sat_short_round(fx * 2048.f);
    } else if (threadIdx.x < 2 * O) {
        const int d = threadIdx.x - O;
        float fy = (float)((d + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= sy;
        b0[d] = sat_short_round((1.f - fy) * 2048.f); b1[d] = sat_short_round(fy * 2048.f);
        ys0[d] = sy < 0 ? 0 : (sy > sh - 1 ? sh - 1 : sy);
        ys1[d] = sy + 1 < 0 ? 0 : (sy + 1 > sh - 1 ? sh - 1 : sy + 1);
    }
    __syncthreads();
    const uint8_t* fp = frames + ((size_t)f * H + y0) * W * 3 + (size_t)x0 * 3;
    for (int p = threadIdx.x; p < O * O * 3; p += blockDim.x) {
        const int c = p % 3, dx = (p / 3) % O, dy = p / (3 * O);
        const uint8_t* S0 = fp + (size_t)ys0[dy] * W * 3;
        const uint8_t* S1 = fp + (size_t)ys1[dy] * W * 3;
        const int r0 = S0[xofs[dx] * 3 + c] * a0[dx] + S0[xofs1[dx] * 3 + c] * a1[dx];
        const int r1 = S1[xofs[dx] * 3 + c] * a0[dx] + S1[xofs1[dx] * 3 + c] * a1[dx];
        int v = (((b0[dy] * (r0 >> 4)) >> 16) + ((b1[dy] * (r1 >> 4)) >> 16) + 2) >> 2;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        o[p] = (float)v / 255.0f;   // to_tensor
    }
}

// SURVEY 8(f)-4 native embedding mode: facenet-pytorch extract_face() for tensor input = crop -> imresample (area)
// to SxS -> .byte() (truncation) -> fixed_image_standardization (x-127.5)/128, optionally BGR -> RGB.
__global__ __launch_bounds__(256) void k_crop_area_std(const uint8_t* __restrict__ frames, int H, int W, const int32_t* __restrict__ rect,
                                                       const uint8_t* __restrict__ valid, int S, int rgb, float* __restrict__ out) {
    const int f = blockIdx.y;
    float* o = out + (size_t)f * S * S * 3;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S * S) return;
    if (!valid[f]) { o[3 * p] = 0.f; o[3 * p + 1] = 0.f; o[3 * p + 2] = 0.f; return; }
    const int x0 = rect[4 * f], y0 = rect[4 * f + 1], iw = rect[4 * f + 2] - x0, ih = rect[4 * f + 3] - y0;
    const int oy = p / S, ox = p - oy * S;
    float b[3];
    trl_area_pixel(frames + (size_t)f * H * W * 3, W, x0, y0, iw, ih, S, ox, oy, b);
    o[3 * p + (rgb ? 2 : 0)] = (b[0] - 127.5f) / 128.0f;
    o[3 * p + 1] = (b[1] - 127.5f) / 128.0f;
    o[3 * p + (rgb ? 0 : 2)] = (b[2] - 127.5f) / 128.0f;
}

// SURVEY 8(f)-4 "landmark-aligned" embedding mode (trl_config.embed_mode 3; this project's own definition, restated in
// oracle/trl_oracle.c orc_crop_aligned): least-squares similarity from the scaled 112x112 five-point template to the face's
// O-Net landmarks, estimated as the inverse map (double, fixed operation order), bilinear sample of the u8 frame with
// replicated borders (float), (v-127.5)/128, optional BGR -> RGB.  One thread per output pixel; every thread of a face
// recomputes the six transform parameters (60 flops) rather than paying a second launch.
__constant__ double TPL_X[5] = {54.706571428571436, 105.04542857142857, 80.036, 59.35614285714286, 101.04271428571428};
__constant__ double TPL_Y[5] = {73.85185714285714, 73.57342857142856, 102.48085714285713, 131.9507142857143, 131.72014285714286};
__global__ __launch_bounds__(256) void k_crop_aligned(const uint8_t* __restrict__ frames, int H, int W, const float* __restrict__ pts0,
                                                      const uint8_t* __restrict__ valid, int S, int rgb, float* __restrict__ out) {
    const int f = blockIdx.y;
    float* o = out + (size_t)f * S * S * 3;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S * S) return;
    if (!valid[f]) { o[3 * p] = 0.f; o[3 * p + 1] = 0.f; o[3 * p + 2] = 0.f; return; }
    const float* pts = pts0 + 10 * f;
    double tx = 0., ty = 0., px = 0., py = 0.;
#pragma unroll
    for (int j = 0; j < 5; j++) { tx += TPL_X[j]; ty += TPL_Y[j]; px += (double)pts[j]; py += (double)pts[5 + j]; }
    tx = tx / 5.; ty = ty / 5.; px = px / 5.; py = py / 5.;
    double sdd = 0., sde = 0., scr = 0.;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const double dx = TPL_X[j] - tx, dy = TPL_Y[j] - ty, ex = (double)pts[j] - px, ey = (double)pts[5 + j] - py;
        sdd = sdd + (dx * dx + dy * dy);
        sde = sde + (dx * ex + dy * ey);
        scr = scr + (dx * ey - dy * ex);
    }
    const double a = sde / sdd, b = scr / sdd;
    const int v = p / S, u = p - v * S;
    const double du = (double)u - tx, dv = (double)v - ty;
    const double x = (a * du - b * dv) + px, y = (b * du + a * dv) + py;
    const double xf = floor(x), yf = floor(y);
    const float fx = (float)(x - xf), fy = (float)(y - yf);
    const double xc = (xf >= -1.) ? (xf > (double)W ? (double)W : xf) : -1., yc = (yf >= -1.) ? (yf > (double)H ? (double)H : yf) : -1.;   // NaN -> -1
    int x0 = (int)xc, y0 = (int)yc, x1 = x0 + 1, y1 = y0 + 1;
    x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0); x1 = x1 < 0 ? 0 : (x1 > W - 1 ? W - 1 : x1);
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0); y1 = y1 < 0 ? 0 : (y1 > H - 1 ? H - 1 : y1);
    const uint8_t* fp = frames + (size_t)f * H * W * 3;
    const uint8_t *r0 = fp + (size_t)y0 * W * 3, *r1 = fp + (size_t)y1 * W * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float p00 = (float)r0[x0 * 3 + c], p01 = (float)r0[x1 * 3 + c], p10 = (float)r1[x0 * 3 + c], p11 = (float)r1[x1 * 3 + c];
        const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
        const float val = top + fy * (bot - top);
        o[3 * p + (rgb ? 2 - c : c)] = (val - 127.5f) / 128.0f;
    }
}

}  // namespace

int trl_launch_crop_area_std(const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid, int S,
                             bool rgb, float* d_faces, hipStream_t s) {
    if (n <= 0) return TRL_OK;
    k_crop_area_std<<<dim3((S * S + 255) / 256, n), 256, 0, s>>>(d_frames, H, W, d_rect, d_valid, S, rgb ? 1 : 0, d_faces);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
int trl_launch_crop_aligned(const uint8_t* d_frames, int n, int H, int W, const float* d_pts0, const uint8_t* d_valid, int S, bool rgb,
                            float* d_faces, hipStream_t s) {
    if (n <= 0) return TRL_OK;
    k_crop_aligned<<<dim3((S * S + 255) / 256, n), 256, 0, s>>>(d_frames, H, W, d_pts0, d_valid, S, rgb ? 1 : 0, d_faces);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
int trl_launch_crop_resize80(const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid,
                             float* d_faces, hipStream_t s) {
    if (n <= 0) return TRL_OK;
    k_crop_resize80<<<n, 256, 0, s>>>(d_frames, H, W, d_rect, d_valid, d_faces);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

// trl_annotate.hip -- the annotation of run()'s output video (server/model.py:67-74) drawn on device frames.
//
// k_draw paints, on u8 BGR frames in device memory, exactly the bytes annotate.py's own rasteriser (the branch taken without
// OpenCV: rectangle, put_text, _blend_segment) paints on a host frame, so that the frames can stay on the device between the
// colour conversion and the JPEG encoder.  Per listed frame: the rectangle (four opaque fills), then the text, a list of
// anti-aliased thick segments blended one after the other -- after each segment the pixel is rounded back to a byte and the
// next segment reads that byte.  The host (annotate.draw_list) lays the text out in float64 and hands over six float32 numbers
// per segment, which is how numpy's weak Python scalars enter annotate.py's float32 array expressions; the kernel repeats that
// expression operation by operation in float32 (the Makefile's -ffp-contract=off keeps products and sums apart, the division is
// hipcc's correctly rounded default) with numpy's float32 hypot -- glibc's correctly rounded hypotf -- as
// (float)sqrt((double)x*x + (double)y*y): both squares are exact in double and the sum and the root are rounded once each;
// float32 sqrt(x*x + y*y) differs from hypotf on about one pair in six.  tests/test_annotate_cpu.py pins the rules on the CPU.
//
// One thread per pixel of the region a frame's list can touch: three byte loads, three byte stores, no two threads share a
// byte.  A frame's region is split in two so that a face box far from the caption does not cost the area between them:
// part 1 is the box of the text (rectangle first, then the segments), part 0 the box of the rectangle minus part 1.
// The work is tiny beside the encoder's (a caption is ~300 segments over ~450x40 pixels); frames without a note get no thread.
#include "trl_host.h"

#include <cmath>
#include <string.h>

#include <vector>

namespace {

struct DevSeg {                     // 40 bytes
    float x0, y0, dx, dy, L2, reach;
    int xa, ya, xb, yb;             // pixels outside this inclusive box have coverage 0 (a superset of _blend_segment's box)
};

struct DevFrame {                   // 120 bytes
    long long offset;               // of the frame in the batch, bytes
    int fill[4][4];                 // the rectangle's fills clipped to the frame: xa, ya, xb, yb inclusive (xa > xb: empty)
    int part[2][4];                 // 0: box of the fills, 1: box of the text; inclusive, xa > xb: empty
    int seg_begin, seg_end;
    unsigned rect_bgr, text_bgr;    // b | g << 8 | r << 16
};

constexpr int TW = 32, TH = 8;      // pixels per workgroup
constexpr int SEG_CHUNK = 256;      // segments staged in LDS at a time

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// np.clip(np.rint(reg * (1 - a) + colour * a), 0, 255).astype(np.uint8)
__device__ __forceinline__ float blend(float reg, float ia, float col, float a) {
    const float p = reg * ia;
    const float q = col * a;
    return fminf(fmaxf(rintf(p + q), 0.0f), 255.0f);
}

__global__ __launch_bounds__(TW * TH) void k_draw(uint8_t* __restrict__ bgr, int W, const DevFrame* __restrict__ frames,
                                                  const DevSeg* __restrict__ segs, int entry0) {
    __shared__ DevSeg lseg[SEG_CHUNK];
    const DevFrame* fr = frames + entry0 + blockIdx.z;
    const int part = blockIdx.y;
    const int bx0 = fr->part[part][0], by0 = fr->part[part][1], bx1 = fr->part[part][2], by1 = fr->part[part][3];
    if (bx0 > bx1 || by0 > by1) return;
    const int tiles_x = (bx1 - bx0) / TW + 1, tiles_y = (by1 - by0) / TH + 1;
    if (blockIdx.x >= (unsigned)(tiles_x * tiles_y)) return;                   // (uniform per workgroup: the barriers below are safe)
    const int x = bx0 + (int)(blockIdx.x % tiles_x) * TW + (int)(threadIdx.x % TW);
    const int y = by0 + (int)(blockIdx.x / tiles_x) * TH + (int)(threadIdx.x / TW);
    bool live = x <= bx1 && y <= by1;
    if (part == 0 && live) {                                                   // the text's box belongs to part 1
        const int tx0 = fr->part[1][0], ty0 = fr->part[1][1], tx1 = fr->part[1][2], ty1 = fr->part[1][3];
        if (x >= tx0 && x <= tx1 && y >= ty0 && y <= ty1) live = false;
    }
    uint8_t* px = bgr + fr->offset + ((size_t)y * W + x) * 3;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    bool dirty = false;
    if (live) {
        bool in = false;
#pragma unroll
        for (int k = 0; k < 4; k++)
            in = in || (x >= fr->fill[k][0] && y >= fr->fill[k][1] && x <= fr->fill[k][2] && y <= fr->fill[k][3]);
        if (in) {
            const unsigned c = fr->rect_bgr;
            v0 = (float)(c & 0xFF); v1 = (float)((c >> 8) & 0xFF); v2 = (float)((c >> 16) & 0xFF);
            dirty = true;
        } else if (part == 1) {
            v0 = (float)px[0]; v1 = (float)px[1]; v2 = (float)px[2];
        }
    }
    if (part == 1) {
        const unsigned c = fr->text_bgr;
        const float c0 = (float)(c & 0xFF), c1 = (float)((c >> 8) & 0xFF), c2 = (float)((c >> 16) & 0xFF);
        const float xx = (float)x, yy = (float)y;
        const int s_end = fr->seg_end;
        for (int s0 = fr->seg_begin; s0 < s_end; s0 += SEG_CHUNK) {
            const int cn = min(SEG_CHUNK, s_end - s0);
            __syncthreads();
            for (int i = threadIdx.x; i < cn; i += TW * TH) lseg[i] = segs[s0 + i];
            __syncthreads();
            if (!live) continue;
            for (int i = 0; i < cn; i++) {
                const int xa = lseg[i].xa, ya = lseg[i].ya, xb = lseg[i].xb, yb = lseg[i].yb;
                if (x < xa || x > xb || y < ya || y > yb) continue;
                const float x0 = lseg[i].x0, y0 = lseg[i].y0, dx = lseg[i].dx, dy = lseg[i].dy, L2 = lseg[i].L2;
                float t = 0.0f;
                if (L2 > 0.0f) {
                    const float ux = (xx - x0) * dx;
                    const float uy = (yy - y0) * dy;
                    t = clip01((ux + uy) / L2);
                }
                const float tx = t * dx, ty = t * dy;
                const float ex = xx - (x0 + tx), ey = yy - (y0 + ty);
                const double ex2 = (double)ex * (double)ex, ey2 = (double)ey * (double)ey;
                const float d = (float)sqrt(ex2 + ey2);
                const float a = clip01(lseg[i].reach - d);
                if (a > 0.0f) {                                               // a == 0 gives the byte back unchanged
                    const float ia = 1.0f - a;
                    v0 = blend(v0, ia, c0, a); v1 = blend(v1, ia, c1, a); v2 = blend(v2, ia, c2, a);
                    dirty = true;
                }
            }
        }
    }
    if (live && dirty) {
        px[0] = (uint8_t)(int)v0; px[1] = (uint8_t)(int)v1; px[2] = (uint8_t)(int)v2;
    }
}

inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// box |= other (both inclusive; an empty box has xa > xb)
inline void grow(int* box, const int* o) {
    if (o[0] > o[2] || o[1] > o[3]) return;
    if (box[0] > box[2] || box[1] > box[3]) { memcpy(box, o, 4 * sizeof(int)); return; }
    box[0] = std::min(box[0], o[0]); box[1] = std::min(box[1], o[1]);
    box[2] = std::max(box[2], o[2]); box[3] = std::max(box[3], o[3]);
}

}  // namespace

extern "C" size_t trl_draw_workspace(int n_frames, int n_segs) {
    if (n_frames < 0 || n_segs < 0) return 0;
    return (size_t)n_frames * sizeof(DevFrame) + (size_t)n_segs * sizeof(DevSeg) + 256;
}

extern "C" int trl_draw(uint8_t* d_bgr, int n, long long frame_stride, int H, int W, const trl_draw_frame* frames, int n_frames,
                        const trl_draw_seg* segs, int n_segs, void* d_work, size_t work_bytes, void* stream) {
    if (n_frames < 0 || n_segs < 0 || n < 0) { trl_set_error("trl_draw: negative count"); return TRL_ERR_INVALID; }
    if (n_frames == 0) return TRL_OK;
    if (!d_bgr || !frames || (n_segs > 0 && !segs) || !d_work) { trl_set_error("trl_draw: null argument"); return TRL_ERR_INVALID; }
    if (H < 1 || W < 1 || n < 1) { trl_set_error("trl_draw: n = %d frames of %d x %d", n, H, W); return TRL_ERR_INVALID; }
    if (frame_stride < (long long)H * W * 3) {
        trl_set_error("trl_draw: frame stride %lld < %d x %d x 3", frame_stride, H, W);
        return TRL_ERR_INVALID;
    }
    if (((uintptr_t)d_work & 15) || work_bytes < trl_draw_workspace(n_frames, n_segs)) {
        trl_set_error("trl_draw: workspace of %zu bytes (need %zu, 16-byte aligned)", work_bytes, trl_draw_workspace(n_frames, n_segs));
        return TRL_ERR_INVALID;
    }
    // ---- the device lists, built and checked in full before anything is queued ------------------------------------------------
    const size_t fbytes = (size_t)n_frames * sizeof(DevFrame), sbytes = (size_t)n_segs * sizeof(DevSeg);
    static thread_local std::vector<unsigned char> host;   // (kept between calls: the source of the copy below never dangles)
    host.resize(fbytes + sbytes);
    DevFrame* df = reinterpret_cast<DevFrame*>(host.data());
    DevSeg* ds = reinterpret_cast<DevSeg*>(host.data() + fbytes);
    for (int i = 0; i < n_segs; i++) {
        const trl_draw_seg& s = segs[i];
        if (!(std::isfinite(s.x0) && std::isfinite(s.y0) && std::isfinite(s.dx) && std::isfinite(s.dy) && std::isfinite(s.L2) && std::isfinite(s.reach)) ||
            s.L2 < 0.0f || s.reach < 0.0f) {
            trl_set_error("trl_draw: segment %d is not finite", i);
            return TRL_ERR_INVALID;
        }
        // coverage is clip(reach - distance, 0, 1): zero at `reach` pixels or more from the segment.  One more pixel covers the
        // rounding of the float32 end point x0 + dx; annotate.py's own box (half + 1 = reach + 0.5 from the float64 ends) lies inside.
        const double xe = (double)s.x0 + s.dx, ye = (double)s.y0 + s.dy, m = (double)s.reach + 1.0;
        const double lim = 1e9;
        DevSeg& o = ds[i];
        o.x0 = s.x0; o.y0 = s.y0; o.dx = s.dx; o.dy = s.dy; o.L2 = s.L2; o.reach = s.reach;
        o.xa = (int)clampll((long long)floor(std::max(-lim, std::min(lim, std::min((double)s.x0, xe) - m))), 0, (long long)W);
        o.ya = (int)clampll((long long)floor(std::max(-lim, std::min(lim, std::min((double)s.y0, ye) - m))), 0, (long long)H);
        o.xb = (int)clampll((long long)ceil(std::max(-lim, std::min(lim, std::max((double)s.x0, xe) + m))), -1, (long long)W - 1);
        o.yb = (int)clampll((long long)ceil(std::max(-lim, std::min(lim, std::max((double)s.y0, ye) + m))), -1, (long long)H - 1);
    }
    std::vector<unsigned char> seen((size_t)n, 0);
    unsigned max_tiles = 0;
    for (int i = 0; i < n_frames; i++) {
        const trl_draw_frame& f = frames[i];
        if (f.frame < 0 || f.frame >= n) { trl_set_error("trl_draw: entry %d names frame %d of %d", i, f.frame, n); return TRL_ERR_INVALID; }
        if (seen[f.frame]) { trl_set_error("trl_draw: frame %d is listed twice (draw it in two calls)", f.frame); return TRL_ERR_INVALID; }
        seen[f.frame] = 1;
        if (f.seg_begin < 0 || f.seg_end < f.seg_begin || f.seg_end > n_segs) {
            trl_set_error("trl_draw: entry %d has segments %d..%d of %d", i, f.seg_begin, f.seg_end, n_segs);
            return TRL_ERR_INVALID;
        }
        if (f.thickness < 0) { trl_set_error("trl_draw: entry %d has thickness %d", i, f.thickness); return TRL_ERR_INVALID; }
        DevFrame& o = df[i];
        o.offset = (long long)f.frame * frame_stride;
        o.seg_begin = f.seg_begin; o.seg_end = f.seg_end;
        o.rect_bgr = f.rect_bgr[0] | (f.rect_bgr[1] << 8) | (f.rect_bgr[2] << 16);
        o.text_bgr = f.text_bgr[0] | (f.text_bgr[1] << 8) | (f.text_bgr[2] << 16);
        for (int p = 0; p < 2; p++) { o.part[p][0] = o.part[p][1] = 0; o.part[p][2] = o.part[p][3] = -1; }
        for (int k = 0; k < 4; k++) { o.fill[k][0] = o.fill[k][1] = 0; o.fill[k][2] = o.fill[k][3] = -1; }
        if (f.thickness > 0) {                             // annotate.rectangle: four inclusive fills, each clipped to the frame
            const long long x0 = std::min(f.x0, f.x1), x1 = std::max(f.x0, f.x1), y0 = std::min(f.y0, f.y1), y1 = std::max(f.y0, f.y1);
            const long long h = f.thickness / 2;
            const long long r[4][4] = {{x0 - h, y0 - h, x1 + h, y0 + h}, {x0 - h, y1 - h, x1 + h, y1 + h},
                                       {x0 - h, y0 - h, x0 + h, y1 + h}, {x1 - h, y0 - h, x1 + h, y1 + h}};
            for (int k = 0; k < 4; k++) {
                const long long xa = std::max(r[k][0], 0LL), ya = std::max(r[k][1], 0LL);
                const long long xb = std::min(r[k][2], (long long)W - 1), yb = std::min(r[k][3], (long long)H - 1);
                if (xa <= xb && ya <= yb) {
                    o.fill[k][0] = (int)xa; o.fill[k][1] = (int)ya; o.fill[k][2] = (int)xb; o.fill[k][3] = (int)yb;
                    grow(o.part[0], o.fill[k]);
                }
            }
        }
        for (int s = f.seg_begin; s < f.seg_end; s++) grow(o.part[1], &ds[s].xa);
        for (int p = 0; p < 2; p++)
            if (o.part[p][0] <= o.part[p][2] && o.part[p][1] <= o.part[p][3]) {
                const long long t = (long long)((o.part[p][2] - o.part[p][0]) / TW + 1) * ((o.part[p][3] - o.part[p][1]) / TH + 1);
                if (t > 0xFFFFFFLL)       // (grid.x * 256 threads must stay below 2^32)
                    { trl_set_error("trl_draw: region too large"); return TRL_ERR_INVALID; }
                max_tiles = std::max(max_tiles, (unsigned)t);
            }
    }
    if (max_tiles == 0) return TRL_OK;                     // every entry lies outside its frame
    TRL_CHECK(trl_device_of(d_bgr));
    hipStream_t s = (hipStream_t)stream;
    // pageable source: the runtime stages it before the call returns; the copy itself is ordered on `stream`
    TRL_HIP(hipMemcpyAsync(d_work, host.data(), host.size(), hipMemcpyHostToDevice, s));
    const DevFrame* wf = reinterpret_cast<const DevFrame*>(d_work);
    const DevSeg* ws = reinterpret_cast<const DevSeg*>((const unsigned char*)d_work + fbytes);
    for (int e0 = 0; e0 < n_frames; e0 += 65535) {
        const int cn = std::min(65535, n_frames - e0);
        hipLaunchKernelGGL(k_draw, dim3(max_tiles, 2, cn), dim3(TW * TH), 0, s, d_bgr, W, wf, ws, e0);
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

// Baseline-JPEG decoder for Motion-JPEG input: n files in device memory -> n u8 BGR frames, byte-identical to
// np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1] (libjpeg-turbo's default path: JDCT_ISLOW, fancy upsampling, no merged
// upsampling, RGB out).  tests/jpegd_ref.py states the rules in numpy and tests/test_jpegd_cpu.py pins them to Pillow.
//
//   host            markers up to SOS (trl_jpegd_parse.h), decode tables, and for DRI streams only a memchr pass that finds the
//                   restart markers.  The entropy-coded bytes of a stream without DRI are never walked on the host.
//   k_jpegd_huff    one wave per (frame, restart interval) segment; the frame's six Huffman tables are staged in LDS by the
//                   whole wave, lane 0 runs jpegd_decode_segment (trl_jpegd_huff.h) and writes the non-zero coefficients as
//                   int16 into the zeroed coefficient slot of its frame.  The batch supplies the parallelism.
//   k_jpegd_idct    one thread per 8x8 block: dequantise, jidctint.c's jpeg_idct_islow, u8 sample planes padded to whole MCUs.
//                   A block that reaches a value at which jidctint.c's arithmetic on a long, this kernel's wrapping 32-bit
//                   arithmetic and a saturating 16-bit SIMD IDCT can part (no encoder makes one from pixels) marks the frame
//                   irregular: the gate of DESIGN.md section 7.
//   k_jpegd_color   one thread per pixel: jdsample.c's h2v2 / h2v1 fancy upsampling on the component's own width and height,
//                   jdcolor.c's 16-bit-fixed YCbCr -> RGB, three bytes written once.  Frames whose status is not 0 are skipped.
//
// A frame that is not attempted (status 1) or whose entropy decode or coefficients are irregular (status 2) has no byte written; the caller
// decodes it with Pillow.  All work is queued on the caller's stream, nothing is allocated inside a call, and the call
// synchronises once, to read the statuses.
#include "trl_common.h"
#include "trl_jpegd_huff.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace {

constexpr int kMaxTabSets = 16;                     // distinct (DHT, DQT) sets per call; a clip normally has one
constexpr size_t kSegCap = (size_t)1 << 20;         // segments per call, at most
constexpr size_t kChunkBudget = (size_t)384 << 20;  // coefficient + plane workspace

struct JdFrame {
    int32_t tabset, hs, vs, pad;
};
__constant__ __attribute__((aligned(16))) uint8_t c_zigzag[64] = TRL_ZIGZAG_LIST;   // trl_zigzag.h, through the parser's header

constexpr int kHuffBytes = 6 * (int)sizeof(JdHuff);

__global__ __launch_bounds__(64) void k_jpegd_huff(const uint8_t* __restrict__ files, const JdSeg* __restrict__ segs,
                                                   const JdFrame* __restrict__ frames, const JdTables* __restrict__ tabs, int H, int W,
                                                   int f0, int16_t* __restrict__ coef, size_t coef_stride, int* __restrict__ status) {
    __shared__ uint4 sh[kHuffBytes / 16 + 4];
    const JdSeg sg = segs[blockIdx.x];
    const JdFrame fr = frames[sg.frame];
    const uint4* src = (const uint4*)tabs[fr.tabset].h;
    for (int i = threadIdx.x; i < kHuffBytes / 16; i += 64) sh[i] = src[i];
    if (threadIdx.x < 4) sh[kHuffBytes / 16 + threadIdx.x] = ((const uint4*)c_zigzag)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    const JdGeom g = jd_geom(H, W, fr.hs, fr.vs);
    const uint8_t* p = files + sg.off;
    const int st = jpegd_decode_segment(p, p + sg.len, sg.expect, (const JdHuff*)sh, (const uint8_t*)(sh + kHuffBytes / 16), g, sg.mcu0,
                                        sg.nmcu, coef + (size_t)(sg.frame - f0) * coef_stride);
    if (st != JD_ST_OK) atomicMax(&status[sg.frame], st);
}

// jpeg_idct_islow's butterfly (jidctint.c: CONST_BITS 13), in 32-bit arithmetic that wraps; SHIFT = 11 for the column pass
// (CONST_BITS - PASS1_BITS) and 18 for the row pass (CONST_BITS + PASS1_BITS + 3).
template <int SHIFT>
__device__ __forceinline__ void jd_idct_1d(const uint32_t (&x)[8], int (&o)[8]) {
    typedef uint32_t u;
    u z2 = x[2], z3 = x[6];
    u z1 = (z2 + z3) * 4433u;
    u tmp2 = z1 + z3 * (u)(-15137);
    u tmp3 = z1 + z2 * 6270u;
    u tmp0 = (x[0] + x[4]) << 13, tmp1 = (x[0] - x[4]) << 13;
    const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7]; tmp1 = x[5]; tmp2 = x[3]; tmp3 = x[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    u z4 = tmp1 + tmp3;
    const u z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (u)(-7373); z2 *= (u)(-20995);
    z3 = z3 * (u)(-16069) + z5;
    z4 = z4 * (u)(-3196) + z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr u rnd = 1u << (SHIFT - 1);
    o[0] = (int)(tmp10 + tmp3 + rnd) >> SHIFT; o[7] = (int)(tmp10 - tmp3 + rnd) >> SHIFT;
    o[1] = (int)(tmp11 + tmp2 + rnd) >> SHIFT; o[6] = (int)(tmp11 - tmp2 + rnd) >> SHIFT;
    o[2] = (int)(tmp12 + tmp1 + rnd) >> SHIFT; o[5] = (int)(tmp12 - tmp1 + rnd) >> SHIFT;
    o[3] = (int)(tmp13 + tmp0 + rnd) >> SHIFT; o[4] = (int)(tmp13 - tmp0 + rnd) >> SHIFT;
}

__device__ __forceinline__ uint32_t jd_range_limit(int v) {      // sample_range_limit + CENTERJSAMPLE, index v & RANGE_MASK
    int s = v & 1023;
    s = s >= 512 ? s - 1024 : s;
    return (uint32_t)min(max(s + 128, 0), 255);
}

// One 1-D pass's inputs: true where a sum that jidctint.c forms from them before it multiplies (x0 +- x4, x2 + x6, and among the
// odd inputs x7 + x1, x5 + x3, x7 + x3, x5 + x1 and the sum of all four) may leave int16.  The inputs are exact and, in pass 1,
// below 2^23 in magnitude, so the tests themselves cannot wrap.
__device__ __forceinline__ bool jd_pass_wide(const int (&x)[8]) {
    return abs(x[0]) + abs(x[4]) > 32767 || abs(x[2]) + abs(x[6]) > 32767 || abs(x[1]) + abs(x[3]) + abs(x[5]) + abs(x[7]) > 32767;
}

__global__ __launch_bounds__(64) void k_jpegd_idct(const int16_t* __restrict__ coef, size_t coef_stride, const JdFrame* __restrict__ frames,
                                                   const JdTables* __restrict__ tabs, int H, int W, int f0, uint8_t* __restrict__ planes,
                                                   size_t plane_stride, int* __restrict__ status) {
    const int fi = blockIdx.y, f = f0 + fi;
    if (status[f] != 0) return;
    const JdFrame fr = frames[f];
    const JdGeom g = jd_geom(H, W, fr.hs, fr.vs);
    const int blk = blockIdx.x * 64 + threadIdx.x;
    if (blk >= g.nblocks) return;
    const int c = blk >= g.base[2] ? 2 : blk >= g.base[1] ? 1 : 0;
    const int rel = blk - g.base[c];
    const int by = rel / g.bw[c], bx = rel - by * g.bw[c];
    const uint4* cp = (const uint4*)(coef + (size_t)fi * coef_stride + (size_t)blk * 64);
    const uint4* qp = (const uint4*)tabs[fr.tabset].quant[c];
    int v[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 cw = cp[r], qw = qp[r];
        const uint32_t cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[r][2 * j] = (int)(int16_t)(cs[j] & 0xFFFF) * (int)(qs[j] & 0xFFFF);      // |int16 x u16| < 2^31: exact
            v[r][2 * j + 1] = (int)(int16_t)(cs[j] >> 16) * (int)(qs[j] >> 16);
        }
    }
    // The gate ("The IDCT gate"): every test is made on exact values, before anything can have wrapped.
    bool wide = false;
    int ws[8][8];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        const int in[8] = {v[0][col], v[1][col], v[2][col], v[3][col], v[4][col], v[5][col], v[6][col], v[7][col]};
        wide |= jd_pass_wide(in);
        const uint32_t x[8] = {(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3],
                               (uint32_t)in[4], (uint32_t)in[5], (uint32_t)in[6], (uint32_t)in[7]};
        int o[8];
        jd_idct_1d<11>(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            wide |= (uint32_t)(o[r] + 32768) > 65535u;                  // the workspace as a 16-bit quantity (dc << 2 included)
            ws[r][col] = o[r];
        }
    }
    if (wide) { atomicMax(&status[f], JD_ST_IRREGULAR); return; }       // (before pass 2: its inputs must be known to be 16 bit)
    const int pw = g.bw[c] * 8;
    size_t pbase = 0;                                                   // planes: Y, Cb, Cr, each padded to whole MCUs
    if (c >= 1) pbase += (size_t)g.bw[0] * 8 * g.mcuy * g.vs * 8;
    if (c == 2) pbase += (size_t)g.mcux * 8 * g.mcuy * 8;
    uint8_t* dst = planes + (size_t)fi * plane_stride + pbase + (size_t)by * 8 * pw + (size_t)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        wide |= jd_pass_wide(ws[r]);
        const uint32_t x[8] = {(uint32_t)ws[r][0], (uint32_t)ws[r][1], (uint32_t)ws[r][2], (uint32_t)ws[r][3],
                               (uint32_t)ws[r][4], (uint32_t)ws[r][5], (uint32_t)ws[r][6], (uint32_t)ws[r][7]};
        int o[8];
        jd_idct_1d<18>(x, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) wide |= (uint32_t)(o[j] + 512) > 1023u;    // the range the mask leaves alone
        uint2 w;
        w.x = jd_range_limit(o[0]) | jd_range_limit(o[1]) << 8 | jd_range_limit(o[2]) << 16 | jd_range_limit(o[3]) << 24;
        w.y = jd_range_limit(o[4]) | jd_range_limit(o[5]) << 8 | jd_range_limit(o[6]) << 16 | jd_range_limit(o[7]) << 24;
        *(uint2*)(dst + (size_t)r * pw) = w;                            // (a plane is workspace: k_jpegd_color skips a gated frame)
    }
    if (wide) atomicMax(&status[f], JD_ST_IRREGULAR);
}

// One chroma sample at output pixel (x, y): jdsample.c's fancy upsampling on the component's dw x dh samples (pw = row pitch).
__device__ __forceinline__ int jd_chroma(const uint8_t* __restrict__ P, int pw, int dw, int dh, int hs, int vs, int x, int y) {
    if (hs == 1) return P[(size_t)y * pw + x];
    const int cx = x >> 1;
    if (vs == 1) {                                                       // h2v1
        const uint8_t* row = P + (size_t)y * pw;
        const int t = row[cx];
        if (dw <= 2) return t;
        if (x & 1) return cx == dw - 1 ? t : (3 * t + row[cx + 1] + 2) >> 2;
        return cx == 0 ? t : (3 * t + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                               // h2v2
    const uint8_t* r0 = P + (size_t)cy * pw;
    if (dw <= 2) return r0[cx];
    const int oy = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);       // the nearer neighbour row, replicated at the edges
    const uint8_t* r1 = P + (size_t)oy * pw;
    const int t = 3 * r0[cx] + r1[cx];
    if (x & 1) return cx == dw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void k_jpegd_color(const uint8_t* __restrict__ planes, size_t plane_stride,
                                                     const JdFrame* __restrict__ frames, const int* __restrict__ status, int H, int W,
                                                     int f0, uint8_t* __restrict__ bgr, long long frame_stride) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, fi = blockIdx.z, f = f0 + fi;
    if (x >= W || status[f] != 0) return;
    const JdFrame fr = frames[f];
    const JdGeom g = jd_geom(H, W, fr.hs, fr.vs);
    const int pwy = g.bw[0] * 8, pwc = g.mcux * 8;
    const uint8_t* Yp = planes + (size_t)fi * plane_stride;
    const uint8_t* Cb = Yp + (size_t)pwy * g.mcuy * g.vs * 8;
    const uint8_t* Cr = Cb + (size_t)pwc * g.mcuy * 8;
    const int dw = (W + fr.hs - 1) / fr.hs, dh = (H + fr.vs - 1) / fr.vs;
    const int yy = Yp[(size_t)y * pwy + x];
    const int cb = jd_chroma(Cb, pwc, dw, dh, fr.hs, fr.vs, x, y) - 128;
    const int cr = jd_chroma(Cr, pwc, dw, dh, fr.hs, fr.vs, x, y) - 128;
    // jdcolor.c build_ycc_rgb_table: FIX(1.40200) 91881, FIX(1.77200) 116130, FIX(0.71414) 46802, FIX(0.34414) 22554
    const int r = yy + ((91881 * cr + 32768) >> 16);
    const int gg = yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    const int b = yy + ((116130 * cb + 32768) >> 16);
    uint8_t* o = bgr + (size_t)f * frame_stride + ((size_t)y * W + x) * 3;
    o[0] = (uint8_t)min(max(b, 0), 255);
    o[1] = (uint8_t)min(max(gg, 0), 255);
    o[2] = (uint8_t)min(max(r, 0), 255);
}

int jd_check_shape(int H, int W) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) { trl_set_error("trl_jpegd: frame %d x %d outside 1..65535", W, H); return TRL_ERR_INVALID; }
    return TRL_OK;
}

}  // namespace

struct trl_jpegd {
    int device = 0, H = 0, W = 0, max_frames = 0, chunk = 0;
    long long max_bytes = 0;
    size_t coef_stride = 0;      // int16 per frame slot
    size_t plane_stride = 0;     // bytes per frame slot
    size_t seg_cap = 0;
    void* mem = nullptr;         // one device allocation, carved below
    size_t mem_bytes = 0;
    int16_t* coef = nullptr;
    uint8_t* planes = nullptr;
    JdFrame* d_frames = nullptr;
    int* d_status = nullptr;
    JdTables* d_tabs = nullptr;
    JdSeg* d_segs = nullptr;
    void* hmem = nullptr;        // one pinned allocation
    JdFrame* h_frames = nullptr;
    int* h_status = nullptr;
    JdTables* h_tabs = nullptr;
    JdSeg* h_segs = nullptr;
    long long* rst = nullptr;    // restart marker offsets of the file being prepared (host)
    size_t* seg_first = nullptr; // [max_frames + 1]
};

extern "C" {

int trl_jpegd_parse(const uint8_t* file, size_t len, trl_jpegd_info* info) {
    if (!file || !info) { trl_set_error("trl_jpegd_parse: null argument"); return TRL_ERR_INVALID; }
    static thread_local JdParsed p;
    jpegd_parse(file, len, &p);
    info->width = p.W; info->height = p.H; info->h_samp = p.hs; info->v_samp = p.vs;
    info->restart_interval = p.ri; info->scan_offset = (int32_t)p.scan;
    info->supported = p.reason == JD_OK; info->reason = p.reason;
    return TRL_OK;
}

int trl_jpegd_create(int device, int H, int W, int max_frames, long long max_bytes, trl_jpegd** out) {
    if (!out) { trl_set_error("trl_jpegd_create: null argument"); return TRL_ERR_INVALID; }
    *out = nullptr;
    TRL_CHECK(jd_check_shape(H, W));
    if (max_frames < 1 || max_frames > 65535) { trl_set_error("trl_jpegd_create: max_frames %d outside 1..65535", max_frames); return TRL_ERR_INVALID; }
    if (max_bytes < 1) { trl_set_error("trl_jpegd_create: max_bytes %lld < 1", max_bytes); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(device));
    trl_jpegd* d = new trl_jpegd;
    d->device = device; d->H = H; d->W = W; d->max_frames = max_frames; d->max_bytes = max_bytes;
    size_t max_blocks = 0, max_plane = 0, max_mcus = 0;
    const int modes[3][2] = {{2, 2}, {2, 1}, {1, 1}};
    for (auto& m : modes) {
        const JdGeom g = jd_geom(H, W, m[0], m[1]);
        max_blocks = std::max(max_blocks, (size_t)g.nblocks);
        max_plane = std::max(max_plane, (size_t)g.nblocks * 64);
        max_mcus = std::max(max_mcus, (size_t)g.mcux * g.mcuy);
    }
    d->coef_stride = max_blocks * 64;
    d->plane_stride = (max_plane + 255) & ~(size_t)255;
    const size_t per_frame = d->coef_stride * 2 + d->plane_stride;
    d->chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)max_frames, kChunkBudget / per_frame));
    d->seg_cap = std::min(kSegCap, (size_t)max_frames * max_mcus);
    const size_t C = (size_t)d->chunk, F = (size_t)max_frames;
    const size_t sz[] = {C * d->coef_stride * 2, C * d->plane_stride, F * sizeof(JdFrame), F * sizeof(int),
                         kMaxTabSets * sizeof(JdTables), d->seg_cap * sizeof(JdSeg)};
    size_t offs[6], total = 0;
    for (int i = 0; i < 6; ++i) { offs[i] = total; total += (sz[i] + 255) & ~(size_t)255; }
    const size_t hoff0 = offs[2], htotal = total - hoff0;                // the host mirrors the four small tables
    hipError_t st = hipMalloc(&d->mem, total);
    if (st == hipSuccess) st = hipHostMalloc(&d->hmem, htotal, hipHostMallocDefault);
    if (st != hipSuccess) {
        trl_set_error("trl_jpegd_create: %zu device bytes for %d x %d frames: %s", total, W, H, hipGetErrorString(st));
        if (d->mem) (void)hipFree(d->mem);
        delete d;
        return TRL_ERR_HIP;
    }
    d->mem_bytes = total;
    uint8_t* m = (uint8_t*)d->mem;
    uint8_t* h = (uint8_t*)d->hmem;
    d->coef = (int16_t*)(m + offs[0]); d->planes = m + offs[1];
    d->d_frames = (JdFrame*)(m + offs[2]); d->d_status = (int*)(m + offs[3]); d->d_tabs = (JdTables*)(m + offs[4]); d->d_segs = (JdSeg*)(m + offs[5]);
    d->h_frames = (JdFrame*)(h + offs[2] - hoff0); d->h_status = (int*)(h + offs[3] - hoff0);
    d->h_tabs = (JdTables*)(h + offs[4] - hoff0); d->h_segs = (JdSeg*)(h + offs[5] - hoff0);
    d->rst = new long long[max_mcus];
    d->seg_first = new size_t[F + 1];
    *out = d;
    return TRL_OK;
}

int trl_jpegd_destroy(trl_jpegd* d) {
    if (!d) return TRL_OK;
    (void)hipSetDevice(d->device);
    (void)hipFree(d->mem);
    (void)hipHostFree(d->hmem);
    delete[] d->rst;
    delete[] d->seg_first;
    delete d;
    return TRL_OK;
}

int trl_jpegd_debug_poison(trl_jpegd* d, int byte) {
    if (!d) { trl_set_error("trl_jpegd_debug_poison: null decoder"); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(d->device));
    TRL_HIP(hipMemset(d->mem, byte, d->mem_bytes));
    TRL_HIP(hipDeviceSynchronize());
    return TRL_OK;
}

int trl_jpegd_decode(trl_jpegd* d, const uint8_t* h_files, const uint8_t* d_files, const long long* offsets, const long long* sizes,
                     int n, uint8_t* d_bgr, long long frame_stride, int32_t* h_status, void* stream) {
    if (!d) { trl_set_error("trl_jpegd_decode: null decoder"); return TRL_ERR_INVALID; }
    if (n < 0 || n > d->max_frames) { trl_set_error("trl_jpegd_decode: n = %d outside 0..%d", n, d->max_frames); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!h_files || !d_files || !offsets || !sizes || !d_bgr || !h_status) { trl_set_error("trl_jpegd_decode: null argument"); return TRL_ERR_INVALID; }
    if (n > 1 && frame_stride < (long long)d->H * d->W * 3) {
        trl_set_error("trl_jpegd_decode: frame stride %lld < %d x %d x 3", frame_stride, d->H, d->W);
        return TRL_ERR_INVALID;
    }
    for (int k = 0; k < n; ++k)
        if (offsets[k] < 0 || sizes[k] < 0 || sizes[k] > 0x7FFFFFFF || offsets[k] > d->max_bytes || sizes[k] > d->max_bytes - offsets[k]) {
            trl_set_error("trl_jpegd_decode: file %d (%lld bytes at %lld) outside the buffer of %lld bytes", k, sizes[k], offsets[k], d->max_bytes);
            return TRL_ERR_INVALID;
        }
    TRL_HIP(hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;

    // ---- host: headers, tables, segments ----
    static thread_local JdParsed ps;
    static thread_local JdTables tb;
    int ntab = 0, n_now = n;                                             // frames [0, n_now) are decoded by this pass
    size_t nseg = 0;
    for (int k = 0; k < n; ++k) {
        d->seg_first[k] = nseg;
        d->h_frames[k] = JdFrame{0, 1, 1, 0};
        d->h_status[k] = JD_ST_UNSUPPORTED;
        const uint8_t* file = h_files + offsets[k];
        const size_t len = (size_t)sizes[k];
        if (jpegd_parse(file, len, &ps) != JD_OK || ps.H != d->H || ps.W != d->W) continue;
        memset(&tb, 0, sizeof(tb));
        jd_build_tables(ps, &tb);
        int t = 0;
        while (t < ntab && memcmp(&d->h_tabs[t], &tb, sizeof(tb)) != 0) ++t;
        if (t == ntab) {
            if (ntab == kMaxTabSets) { n_now = k; break; }               // the table cache is full: the rest is a call of its own
            memcpy(&d->h_tabs[ntab++], &tb, sizeof(tb));
        }
        const JdGeom g = jd_geom(d->H, d->W, ps.hs, ps.vs);
        const long long made = jd_build_segments(file, len, ps, g, offsets[k], k, d->rst, d->h_segs + nseg, d->seg_cap - nseg);
        if (made < 0) continue;
        nseg += (size_t)made;
        d->h_frames[k] = JdFrame{t, ps.hs, ps.vs, 0};
        d->h_status[k] = JD_ST_OK;
    }
    d->seg_first[n_now] = nseg;

    // ---- device ----
    TRL_HIP(hipMemcpyAsync(d->d_frames, d->h_frames, (size_t)n_now * sizeof(JdFrame), hipMemcpyHostToDevice, s));
    TRL_HIP(hipMemcpyAsync(d->d_status, d->h_status, (size_t)n_now * sizeof(int), hipMemcpyHostToDevice, s));
    if (ntab) TRL_HIP(hipMemcpyAsync(d->d_tabs, d->h_tabs, (size_t)ntab * sizeof(JdTables), hipMemcpyHostToDevice, s));
    if (nseg) TRL_HIP(hipMemcpyAsync(d->d_segs, d->h_segs, nseg * sizeof(JdSeg), hipMemcpyHostToDevice, s));
    const int max_blocks = (int)(d->coef_stride / 64);
    for (int f0 = 0; f0 < n_now && nseg; f0 += d->chunk) {
        const int cn = std::min(d->chunk, n_now - f0);
        const size_t s0 = d->seg_first[f0], s1 = d->seg_first[f0 + cn];
        if (s1 == s0) continue;
        TRL_HIP(hipMemsetAsync(d->coef, 0, (size_t)cn * d->coef_stride * 2, s));
        hipLaunchKernelGGL(k_jpegd_huff, dim3((unsigned)(s1 - s0)), dim3(64), 0, s, d_files, d->d_segs + s0, d->d_frames, d->d_tabs, d->H,
                           d->W, f0, d->coef, d->coef_stride, d->d_status);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpegd_idct, dim3((unsigned)((max_blocks + 63) / 64), cn), dim3(64), 0, s, d->coef, d->coef_stride, d->d_frames,
                           d->d_tabs, d->H, d->W, f0, d->planes, d->plane_stride, d->d_status);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpegd_color, dim3((unsigned)((d->W + 255) / 256), d->H, cn), dim3(256), 0, s, d->planes, d->plane_stride,
                           d->d_frames, d->d_status, d->H, d->W, f0, d_bgr, frame_stride);
        TRL_LAUNCH_CHECK();
    }
    TRL_HIP(hipMemcpyAsync(d->h_status, d->d_status, (size_t)n_now * sizeof(int), hipMemcpyDeviceToHost, s));
    TRL_HIP(hipStreamSynchronize(s));
    memcpy(h_status, d->h_status, (size_t)n_now * sizeof(int));
    if (n_now < n)                                                       // (the stream is idle: the pinned tables may be rewritten)
        return trl_jpegd_decode(d, h_files, d_files, offsets + n_now, sizes + n_now, n - n_now, d_bgr + (size_t)n_now * frame_stride,
                                frame_stride, h_status + n_now, stream);
    return TRL_OK;
}

}  // extern "C"

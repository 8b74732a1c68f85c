// trl_jpeg.hip -- baseline Motion-JPEG encoder for run()'s annotated output, byte-identical to Pillow's
// Image.save(format="JPEG", quality=q, subsampling=s, restart_marker_rows=r | restart_marker_blocks=b, optimize=o) (libjpeg-turbo's
// baseline path).  trl_jpeg_create writes the default kind of file: 4:2:0, standard tables, no restart markers; trl_jpeg_create_ex
// takes the options.  Integer arithmetic only, so the bytes do not depend on the launch shape.  The rules (DESIGN.md "Motion-JPEG
// on the device"; restated in numpy and pinned to Pillow by tests/test_jpeg_cpu.py and tests/jpeg_options_ref.py):
//   colour      jccolor's 16-bit fixed point, BGR input
//   edges       every component: source columns and rows replicated (the last pixel repeats), which is what libjpeg's padding of
//               each component to whole blocks amounts to, with these downsampling rules
//               4:2:0 (MCU 16 x 16: Y00 Y01 Y10 Y11 Cb Cr)  chroma: full-resolution columns replicated to whole chroma blocks x 2,
//                     rows to an even count, h2v2 average with bias 1,2,1,2..., last chroma row replicated to whole blocks
//               4:2:2 (MCU 16 x 8: Y0 Y1 Cb Cr)             chroma: columns as for 4:2:0, h2v1 average with bias 0,1,0,1...
//               4:4:4 (MCU 8 x 8: Y Cb Cr)                  no downsampling
//   FDCT        jfdctint islow (CONST_BITS 13, PASS1_BITS 2) on sample - 128; quantisation (|c| + 4q) / 8q, sign restored
//   dummies     Y blocks past the image in the last MCU column / row: zero AC and
//               4:2:0  the DC of the left neighbour (right edge) or of the MCU's Y01 (bottom edge)
//               4:2:2  the DC of Y0 (right edge); an MCU is one block high, so there is no bottom dummy
//               4:4:4  none: an MCU is one block
//   entropy     DC predictor per component, ZRL / EOB, last byte padded with 1-bits, 0xFF stuffed as FF 00; Annex K tables
//   restart     an interval of R MCUs (restart_rows x MCUs per row, at most 65535, else restart_blocks): DRI after the DHTs; at
//               each interval start all three DC predictors are 0; each interval is padded with 1-bits to a byte (stuffed like
//               any other byte when it comes out as 0xFF), FF D0 .. FF D7 follow, cycling, never stuffed; none after the last
//   optimize    libjpeg's two passes: the symbols the scan will emit are counted per table (luma; Cb and Cr together), each of
//               the four tables is jpeg_gen_optimal_table's (trl_jpeg_hufftab.h), and the frame's header carries its own DHTs
// Pipeline per chunk of frames (all on the caller's stream; one host synchronisation per batch, to read the sizes):
//   k_jpeg_blocks<S>  a workgroup = a strip of one MCU row, 64 pixels wide (4 MCUs; 8 at 4:4:4): BGR -> YCbCr into LDS, the
//                     sampling's chroma average, FDCT, quantisation, zigzag, dummy blocks -> int16 coefficients
//                     [frame][mcu][blocks per MCU][64]
//   k_jpeg_hist       optimize only: the symbols the scan will emit, per-workgroup LDS histograms added to the frame's by
//   k_jpeg_tables     device-scope integer atomics that only later kernels read; then one wave per frame and table builds the
//                     table, and the workgroup the frame's header.  Tables never visit the host.
//   k_jpeg_bits       one wave per block, lane k = zigzag coefficient k: ballot -> run lengths -> the block's bit count
//   k_jpeg_scan       one workgroup per frame: exclusive scan of the block bit counts; with restart intervals the offsets restart
//                     per interval and the intervals' byte lengths (+ 2 marker bytes) are scanned again
//   k_jpeg_emit       one wave per block: each lane ORs its codes into the wave's LDS words at (block offset + lane prefix); an
//                     interval's last block adds the padding and, unless the interval is the frame's last, the marker, so that
//                     every word has one writer; the words inside the block's range are stored, its first and last set aside
//   k_jpeg_edges      one thread per block: the words blocks share, merged by the one block that owns each (no atomics)
//   k_jpeg_ffcount    FF bytes per 4 KiB segment of each frame's scan (the markers' are found by the interval starts, and skipped)
//   k_jpeg_sizes      one workgroup per chunk: scan of the segment counts, frame sizes and output offsets
//   k_jpeg_scatter    header + stuffed scan + EOI into the caller's buffer; a frame that would end past the capacity is not written
// Every stage is written once.  The entropy stages (bits .. scatter) are templates over a layout policy: FixedLayout is the
// default kind of file with everything a constant (6 blocks per MCU, one interval, one table and one header), RunLayout carries
// blocks per MCU, the interval, the interval count and the table stride as kernel arguments; an encoder launches one or the other
// throughout (trl_jpeg::ex).
#include "trl_common.h"
#include "trl_jpeg_hufftab.h"
#include "trl_zigzag.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

namespace {

constexpr int kZigzag[64] = TRL_ZIGZAG_LIST;
__constant__ int c_zigzag[64] = TRL_ZIGZAG_LIST;
// ITU-T T.81 Annex K: quantisation tables (natural order) and Huffman tables (code counts per length, symbols)
constexpr int kStdQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

constexpr int kMaxBlockBits = 1792;           // >= 22 (DC) + 63 x 27 (AC) + 3 ZRL x 11 + EOB: 224 scratch bytes per block
constexpr int kSeg = 4096;                    // bytes per stuffing segment (256 threads x 16 bytes)
constexpr size_t kChunkBudget = 256u << 20;   // device workspace per chunk of frames
constexpr int kHist = 4 * 256;                // optimize: symbol counts per frame [DC luma, AC luma, DC chroma, AC chroma][256]
constexpr int kHdrCap = 1024;                 // bytes set aside for a header (the common one; with optimize one per frame)

// What k_jpeg_blocks<S> needs to know of sampling S = 0 / 1 / 2 (4:4:4 / 4:2:2 / 4:2:0, Pillow's numbering): a workgroup's strip
// is one MCU high and 64 pixels wide.
template <int S>
struct Sampling {
    static constexpr int kRows = S == 2 ? 16 : 8;            // MCU height = strip rows
    static constexpr int kMcuW = S == 0 ? 8 : 16;            // MCU width
    static constexpr int kLuma = S == 0 ? 1 : S == 1 ? 2 : 4;// Y blocks per MCU (Y00 Y01 Y10 Y11; Cb and Cr follow)
    static constexpr int kBpm = kLuma + 2;                   // blocks per MCU
    static constexpr int kMcus = 64 / kMcuW;                 // MCUs per workgroup
    static constexpr int kBlocks = kMcus * kBpm;             // blocks per workgroup: 24 / 16 / 24
};

struct JTab {
    uint16_t qdiv[2][64];   // 8 * quantiser, natural order (luma, chroma)
    uint32_t dc[2][12];     // (code << 8) | length, by magnitude category
    uint32_t ac[2][256];    // (code << 8) | length, by (run << 4) | category
};

void quant_table(int quality, int t, uint8_t* q) {
    const int qq = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = qq < 50 ? 5000 / qq : 200 - 2 * qq;
    for (int i = 0; i < 64; ++i) {
        long v = ((long)kStdQ[t][i] * s + 50) / 100;
        q[i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = ((uint32_t)code++ << 8) | (uint32_t)len;
        code <<= 1;
    }
}

// sampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0 (Pillow's numbering); dri > 0 adds a DRI segment where libjpeg puts it (after the
// DHTs); dht_at / tail_at receive the offsets of the first DHT and of what follows the last (k_jpeg_tables splices there)
size_t header_bytes(int H, int W, int quality, int sampling, int dri, uint8_t* o, int* dht_at = nullptr, int* tail_at = nullptr) {   // o == nullptr: length only
    size_t p = 0;
    auto put = [&](int v) { if (o) o[p] = (uint8_t)v; ++p; };
    auto seg = [&](int marker, int len) { put(0xFF); put(marker); put(len >> 8); put(len & 0xFF); };
    put(0xFF); put(0xD8);
    seg(0xE0, 16);
    for (int v : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        seg(0xDB, 67);
        put(t);
        for (int i = 0; i < 64; ++i) put(q[kZigzag[i]]);
    }
    seg(0xC0, 17);
    for (int v : {8, H >> 8, H & 0xFF, W >> 8, W & 0xFF, 3, 1, sampling == 0 ? 0x11 : sampling == 1 ? 0x21 : 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
    if (dht_at) *dht_at = (int)p;
    for (int t = 0; t < 2; ++t) {
        seg(0xC4, 2 + 1 + 16 + 12);
        put(t);
        for (int i = 0; i < 16; ++i) put(kDcBits[t][i]);
        for (int i = 0; i < 12; ++i) put(i);
        int nv = 0;
        for (int i = 0; i < 16; ++i) nv += kAcBits[t][i];
        seg(0xC4, 2 + 1 + 16 + nv);
        put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(kAcBits[t][i]);
        for (int i = 0; i < nv; ++i) put(kAcVals[t][i]);
    }
    if (tail_at) *tail_at = (int)p;
    if (dri > 0) { seg(0xDD, 4); put(dri >> 8); put(dri & 0xFF); }
    seg(0xDA, 12);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
    return p;
}

int check_shape(int H, int W) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535) {
        trl_set_error("trl_jpeg: frame %d x %d outside 1..65535 px per side", W, H);
        return TRL_ERR_INVALID;
    }
    return TRL_OK;
}

struct JOpt {               // trl_jpeg_options, checked and resolved for a frame size
    int quality, sampling, bpm, mcuw, mcuh, mcux, mcuy, dri, optimize;
    bool ex() const { return sampling != 2 || dri > 0 || optimize; }   // anything but the kind of file trl_jpeg_create writes
};

int resolve_options(const char* who, int H, int W, const trl_jpeg_options* o, JOpt* r) {
    TRL_CHECK(check_shape(H, W));
    if (!o) { trl_set_error("%s: null options", who); return TRL_ERR_INVALID; }
    if (o->subsampling < 0 || o->subsampling > 2) { trl_set_error("%s: subsampling %d outside 0..2 (4:4:4, 4:2:2, 4:2:0)", who, o->subsampling); return TRL_ERR_INVALID; }
    if (o->restart_rows < 0 || o->restart_blocks < 0 || o->restart_blocks > 65535) {
        trl_set_error("%s: restart_rows %d / restart_blocks %d: rows >= 0, blocks 0..65535", who, o->restart_rows, o->restart_blocks);
        return TRL_ERR_INVALID;
    }
    r->quality = o->quality; r->sampling = o->subsampling; r->optimize = o->optimize != 0;
    r->bpm = o->subsampling == 0 ? 3 : o->subsampling == 1 ? 4 : 6;
    r->mcuw = o->subsampling == 0 ? 8 : 16; r->mcuh = o->subsampling == 2 ? 16 : 8;
    r->mcux = (W + r->mcuw - 1) / r->mcuw; r->mcuy = (H + r->mcuh - 1) / r->mcuh;
    r->dri = o->restart_rows > 0 ? (int)std::min<long long>((long long)o->restart_rows * r->mcux, 65535) : o->restart_blocks;
    // libjpeg fails on a histogram whose optimal code is deeper than 32 bits; fewer than 9,227,465 symbols cannot make one
    if (r->optimize && (long long)r->mcux * r->mcuy * (r->bpm - 2) * 64 >= 9227465) {
        trl_set_error("%s: optimize needs fewer than 9227465 luma coefficients per frame (%d x %d has more)", who, W, H);
        return TRL_ERR_INVALID;
    }
    return TRL_OK;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint islow, one 8-point pass over d[0], d[s], ..., d[7s] in place
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int s) {
    constexpr int CB = 13, P1 = 2, SH = FIRST ? CB - P1 : CB + P1;
    const int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
    const int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << P1 : descale(t10 + t11, P1);
    d[4 * s] = FIRST ? (t10 - t11) << P1 : descale(t10 - t11, P1);
    const int e1 = (t12 + t13) * 4433;                                   // FIX_0_541196100
    d[2 * s] = descale(e1 + t13 * 6270, SH);                             // FIX_0_765366865
    d[6 * s] = descale(e1 - t12 * 15137, SH);                            // FIX_1_847759065
    const int z5 = (t4 + t6 + t5 + t7) * 9633;                           // FIX_1_175875602
    const int z1 = -(t4 + t7) * 7373, z2 = -(t5 + t6) * 20995;           // FIX_0_899976223, FIX_2_562915447
    const int z3 = -(t4 + t6) * 16069 + z5, z4 = -(t5 + t7) * 3196 + z5; // FIX_1_961570560, FIX_0_390180644
    d[7 * s] = descale(t4 * 2446 + z1 + z3, SH);                         // FIX_0_298631336
    d[5 * s] = descale(t5 * 16819 + z2 + z4, SH);                        // FIX_2_053119869
    d[3 * s] = descale(t6 * 25172 + z2 + z3, SH);                        // FIX_3_072711026
    d[1 * s] = descale(t7 * 12299 + z1 + z4, SH);                        // FIX_1_501321110
}

// grid (ceil(mcux / Sampling<S>::kMcus), mcuy, frames of the chunk), 256 threads: one strip
template <int S>
__global__ __launch_bounds__(256) void k_jpeg_blocks(const uint8_t* __restrict__ src, long long frame_stride, int H, int W,
                                                     int mcux, int mcuy, const JTab* __restrict__ tab, int16_t* __restrict__ coef) {
    using T = Sampling<S>;
    constexpr int ROWS = T::kRows, MW = T::kMcuW, NY = T::kLuma, BPM = T::kBpm, NB = T::kBlocks;
    __shared__ int pix[3][ROWS][64];          // Y, Cb, Cr of the strip at full resolution (edge-replicated source pixels)
    __shared__ int blk[NB][64];               // centred samples -> FDCT output, natural order
    __shared__ int16_t qz[NB][64];            // quantised, zigzag order
    const int tid = threadIdx.x, mx0 = blockIdx.x * T::kMcus, my = blockIdx.y, f = blockIdx.z;
    const uint8_t* fr = src + (size_t)f * frame_stride;
    for (int i = tid; i < ROWS * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int gy = min(ROWS * my + r, H - 1), gx = min(MW * mx0 + c, W - 1);
        const uint8_t* p = fr + ((size_t)gy * W + gx) * 3;
        const int B = p[0], G = p[1], R = p[2];
        pix[0][r][c] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        pix[1][r][c] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        pix[2][r][c] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    }
    __syncthreads();
    [[maybe_unused]] const int crow_last = ((H + 1) >> 1) - 1 - 8 * my;   // 4:2:0: last real chroma row of the strip (>= 0)
    for (int i = tid; i < NB * 64; i += 256) {
        const int b = i >> 6, r = (i >> 3) & 7, c = i & 7, m = b / BPM, kind = b % BPM;
        int v;
        if constexpr (S == 0) {                                          // an MCU is Y Cb Cr: every component is copied
            v = pix[kind][r][m * 8 + c];
        } else if (kind < NY) {
            v = pix[0][(kind >> 1) * 8 + r][m * MW + (kind & 1) * 8 + c];
        } else {
            const int (*pl)[64] = pix[kind - NY + 1];
            if constexpr (S == 1) {                                      // h2v1, bias 0,1,0,1...
                const int cc = 2 * (m * 8 + c);
                v = (pl[r][cc] + pl[r][cc + 1] + (c & 1)) >> 1;
            } else {                                                     // h2v2, bias 1,2,1,2...; the last real row repeats
                const int rr = 2 * min(r, crow_last), cc = 2 * (m * 8 + c);
                v = (pl[rr][cc] + pl[rr][cc + 1] + pl[rr + 1][cc] + pl[rr + 1][cc + 1] + 1 + (c & 1)) >> 2;
            }
        }
        blk[b][(r << 3) | c] = v - 128;
    }
    __syncthreads();
    if (tid < NB * 8) fdct8<true>(&blk[tid >> 3][(tid & 7) * 8], 1);
    __syncthreads();
    if (tid < NB * 8) fdct8<false>(&blk[tid >> 3][tid & 7], 8);
    __syncthreads();
    for (int i = tid; i < NB * 64; i += 256) {
        const int b = i >> 6, z = i & 63;
        const int c = blk[b][c_zigzag[z]], d = tab->qdiv[(b % BPM) < NY ? 0 : 1][c_zigzag[z]];
        const int a = ((c < 0 ? -c : c) + (d >> 1)) / d;
        qz[b][z] = (int16_t)(c < 0 ? -a : a);
    }
    __syncthreads();
    [[maybe_unused]] const int bw = (W + 7) >> 3, bh = (H + 7) >> 3;   // Y blocks holding image samples
    for (int i = tid; i < NB * 64; i += 256) {
        const int b = i >> 6, z = i & 63, m = b / BPM, kind = b % BPM, mx = mx0 + m;
        if (mx >= mcux) continue;
        int v = qz[b][z];
        if constexpr (S != 0) {                                  // dummies: 4:4:4 none, 4:2:2 right only, 4:2:0 right and bottom
            if (kind < NY) {
                const bool right = 2 * mx + (kind & 1) >= bw, bottom = S == 2 && 2 * my + (kind >> 1) >= bh;
                if (bottom) {                                    // the MCU's Y01 (itself a right dummy: Y00's DC)
                    v = z ? 0 : (2 * mx + 1 >= bw ? qz[m * BPM][0] : qz[m * BPM + 1][0]);
                } else if (right) {                              // the left neighbour in the MCU
                    v = z ? 0 : qz[b - 1][0];
                }
            }
        }
        // One index, spelled per sampling so that each instantiation compiles to the store of the kernel it replaces: on the
        // 4:2:0 spelling k_jpeg_blocks<0> measured 1.6 - 2.2 % slower (profiles/jpeg_refactor_kernel_stats.csv, s1_ rows).
        const size_t mcu = ((size_t)f * mcuy + my) * mcux + mx;
        coef[S == 2 ? mcu * (BPM * 64) + kind * 64 + z : (mcu * BPM + kind) * 64 + z] = (int16_t)v;
    }
}

__device__ __forceinline__ int nbits_of(int a) { return a ? 32 - __clz(a) : 0; }

// How a frame's blocks are laid out for the entropy stages: blocks per MCU (component order in an MCU: the Y blocks, Cb, Cr),
// the restart intervals, and whether each frame has a code table of its own.  FixedLayout is the default kind of file, all of it
// constants, and is never a kernel argument; RunLayout is one.
struct FixedLayout {
    static constexpr bool kIntervals = false;                // one interval: the frame
    __device__ static constexpr int bpm() { return 6; }
    __device__ static constexpr int nint() { return 1; }
    __device__ static constexpr int tab_stride() { return 0; }
    __device__ static bool starts_interval(int mcu) { return mcu == 0; }
    __device__ static bool ends_interval(int j, int blocks) { return j == blocks - 1; }
    __device__ static constexpr int interval_of(int) { return 0; }
};
struct RunLayout {
    static constexpr bool kIntervals = true;
    int bpm_, R, nint_, tab_stride_;                         // R: MCUs per interval (no DRI: the frame's MCU count, one interval)
    __device__ int bpm() const { return bpm_; }
    __device__ int nint() const { return nint_; }
    __device__ int tab_stride() const { return tab_stride_; }   // 1: a table per frame (optimize)
    __device__ bool starts_interval(int mcu) const { return mcu % R == 0; }
    __device__ int per() const { return R * bpm_; }          // blocks per interval
    __device__ bool ends_interval(int j, int blocks) const { return j == blocks - 1 || (j + 1) % per() == 0; }
    __device__ int interval_of(int j) const { return j / per(); }
};
// A kernel <L, LA...> ends its parameters with LA... la and begins with `const L lay{la...}`: LA is empty for FixedLayout and
// the RunLayout itself otherwise (JPEG_STAGE launches either).

template <class L>
__device__ __forceinline__ int table_of(const L& lay, int j) { return j % lay.bpm() < lay.bpm() - 2 ? 0 : 1; }   // luma / chroma

// the DC predictor of block j of a frame: the component's previous block, 0 at the start of each restart interval
template <class L>
__device__ __forceinline__ int dc_pred(const L& lay, const int16_t* __restrict__ fcoef, int j) {
    const int bpm = lay.bpm(), mcu = j / bpm, kind = j % bpm, ny = bpm - 2;
    if (kind >= 1 && kind < ny) return fcoef[(size_t)(j - 1) * 64];
    if (lay.starts_interval(mcu)) return 0;
    return fcoef[(size_t)(j - bpm + (kind == 0 ? ny - 1 : 0)) * 64];
}

// the zero run in front of the non-zero coefficient of lane `lane` (>= 1), given the ballot of the block's non-zero lanes
__device__ __forceinline__ int run_before(unsigned long long mask, int lane) {
    const unsigned long long below = mask & ((1ull << lane) - 1ull) & ~1ull;
    const int prev = below ? 63 - __clzll(below) : 0;
    return lane - prev - 1;
}

// The codes of lane k of a block (lane = zigzag index).  Up to three ZRL codes and one (code, magnitude) piece, or the EOB on
// lane 63 when coefficient 63 is zero (its lane has no other bits, so the EOB lands at the block's end).  k_jpeg_hist counts
// the same symbols on the same three branches: a classification shared through callbacks cost k_jpeg_bits 1 %.
struct LaneCodes {
    uint32_t piece;   // (code << nb) | magnitude bits
    int plen;         // its length (0: none)
    int nzrl;         // ZRL codes before it
    uint32_t zrl;     // ZRL code << 8 | length
    __device__ int bits() const { return plen + nzrl * (int)(zrl & 0xFF); }
};

__device__ __forceinline__ LaneCodes lane_codes(const JTab* __restrict__ tab, const int16_t* __restrict__ blkc, int lane, int t,
                                                int pred) {
    const int v = blkc[lane];
    const unsigned long long mask = __ballot(v != 0);
    LaneCodes o{0u, 0, 0, tab->ac[t][0xF0]};
    if (lane == 0) {
        const int diff = v - pred, a = diff < 0 ? -diff : diff, nb = nbits_of(a);
        const uint32_t e = tab->dc[t][nb];
        o.piece = ((e >> 8) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u));
        o.plen = (int)(e & 0xFF) + nb;
    } else if (v != 0) {
        const int run = run_before(mask, lane), a = v < 0 ? -v : v, nb = nbits_of(a);
        o.nzrl = run >> 4;
        const uint32_t e = tab->ac[t][((run & 15) << 4) | nb];
        o.piece = ((e >> 8) << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u));
        o.plen = (int)(e & 0xFF) + nb;
    } else if (lane == 63) {
        const uint32_t e = tab->ac[t][0x00];
        o.piece = e >> 8;
        o.plen = (int)(e & 0xFF);
    }
    return o;
}

__device__ __forceinline__ int wave_sum(int x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// grid ceil(frames * blocks / 4), 256 threads: one wave per block
template <class L, class... LA>
__global__ __launch_bounds__(256) void k_jpeg_bits(const int16_t* __restrict__ coef, int blocks, long long total,
                                                   const JTab* __restrict__ tab, uint32_t* __restrict__ bits, LA... la) {
    const L lay{la...};
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= total) return;                                 // wave-uniform
    const long long f = g / blocks;
    const int j = (int)(g - f * blocks);
    const int16_t* fcoef = coef + (size_t)f * blocks * 64;
    const int pred = lane == 0 ? dc_pred(lay, fcoef, j) : 0;
    const LaneCodes lc = lane_codes(tab + (size_t)f * lay.tab_stride(), fcoef + (size_t)j * 64, lane, table_of(lay, j), pred);
    const int s = wave_sum(lc.bits());
    if (lane == 0) bits[g] = (uint32_t)s;
}

// exclusive scan of n values in LDS-sized steps by one 1024-thread workgroup; returns the total
template <typename T, typename In, typename Out>
__device__ T block_exclusive_scan(In in, Out out, long long n, T* sh) {
    T carry = 0;
    const int tid = threadIdx.x;
    for (long long base = 0; base < n; base += 1024) {
        const long long i = base + tid;
        const T v = i < n ? in(i) : (T)0;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const T add = tid >= o ? sh[tid - o] : (T)0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        if (i < n) out(i, carry + sh[tid] - v);
        carry += sh[1023];
        __syncthreads();
    }
    return carry;
}

// grid = frames of the chunk, 1024 threads: block bit offsets and the frame's scan length in bits.  With restart intervals the
// frame's scan is the intervals' bits back to back, each padded to a byte and (but for the last) followed by the two marker
// bytes, which are part of the stream k_jpeg_emit writes:
//   off[j]   block j's bit offset in that stream (its offset within the interval + the interval's byte start)
//   bits[j]  the interval's last block: its bits + the padding + 16 marker bits, so that every word has one owner
//   ist[i]   interval i's byte start (k_jpeg_ffcount / k_jpeg_scatter find the marker bytes, which are not stuffed, by it)
//   fbits    the stream's length in bits (whole bytes)
// FixedLayout has none of that pass: bits[] stays as k_jpeg_bits wrote it, fbits is the sum, and the frame's one padding is
// added where it is used (k_jpeg_emit, word_range).
template <class L, class... LA>
__global__ __launch_bounds__(1024) void k_jpeg_scan(uint32_t* __restrict__ bits, int blocks, unsigned long long* __restrict__ off,
                                                    unsigned long long* __restrict__ fbits, unsigned long long* __restrict__ ist,
                                                    unsigned long long* __restrict__ ibase, LA... la) {
    __shared__ unsigned long long sh[1024];
    const size_t f = blockIdx.x;
    uint32_t* b = bits + f * blocks;
    unsigned long long* o = off + f * blocks;
    unsigned long long t = block_exclusive_scan<unsigned long long>(
        [&](long long i) { return (unsigned long long)b[i]; }, [&](long long i, unsigned long long v) { o[i] = v; }, blocks, sh);
    if constexpr (L::kIntervals) {
        const L lay{la...};
        const int nint = lay.nint();
        unsigned long long* is = ist + f * nint;
        unsigned long long* ib = ibase + f * nint;           // interval bit starts before padding
        __syncthreads();
        for (int i = threadIdx.x; i < nint; i += 1024) {
            const long long sb = (long long)i * lay.per(), eb = sb + lay.per();
            const unsigned long long len = (eb < blocks ? o[eb] : t) - o[sb];
            ib[i] = o[sb];
            is[i] = ((len + 7) >> 3) + (i < nint - 1 ? 2 : 0);
        }
        __syncthreads();
        const unsigned long long nbytes = block_exclusive_scan<unsigned long long>(
            [&](long long i) { return is[i]; }, [&](long long i, unsigned long long v) { is[i] = v; }, nint, sh);
        __syncthreads();
        for (int j = threadIdx.x; j < blocks; j += 1024) {
            const int i = lay.interval_of(j);
            const unsigned long long p = is[i] * 8 + (o[j] - ib[i]);
            o[j] = p;
            if (lay.ends_interval(j, blocks)) {
                const unsigned long long end = p + b[j];
                b[j] += (uint32_t)((0 - end) & 7) + (i < nint - 1 ? 16u : 0u);
            }
        }
        t = nbytes * 8;
    }
    if (threadIdx.x == 0) fbits[f] = t;
}

__device__ __forceinline__ void put_bits(uint32_t* w, int p, uint32_t val, int len) {   // big-endian bit order
    if (len <= 0) return;
    const unsigned long long x = (unsigned long long)val << (64 - (p & 31) - len);
    atomicOr(&w[p >> 5], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&w[(p >> 5) + 1], (uint32_t)x);
}

// grid ceil(frames * blocks / 4), 256 threads: one wave per block, LDS words per wave.  The last block of an interval adds the
// 1-bit padding to a byte and, unless the interval is the frame's last, the RSTn marker.  A block's words strictly inside its bit
// range are stored; its first and last words, which it may share with its neighbours, go to first[] / last[] for k_jpeg_edges.
// No word is written twice and there are no global atomics: per-XCD L2s are not coherent with each other within a kernel.
template <class L, class... LA>
__global__ __launch_bounds__(256) void k_jpeg_emit(const int16_t* __restrict__ coef, int blocks, long long total,
                                                   const JTab* __restrict__ tab, const unsigned long long* __restrict__ off,
                                                   const uint32_t* __restrict__ bits, size_t scratch_per_frame,
                                                   uint32_t* __restrict__ scratch, uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                   LA... la) {
    const L lay{la...};
    __shared__ uint32_t buf[4][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + wv;
    buf[wv][lane] = 0;
    __syncthreads();
    if (g < total) {                                         // wave-uniform
        const long long f = g / blocks;
        const int j = (int)(g - f * blocks);
        const int16_t* fcoef = coef + (size_t)f * blocks * 64;
        const int pred = lane == 0 ? dc_pred(lay, fcoef, j) : 0;
        const LaneCodes lc = lane_codes(tab + (size_t)f * lay.tab_stride(), fcoef + (size_t)j * 64, lane, table_of(lay, j), pred);
        int pre = lc.bits();                                 // inclusive -> exclusive wave prefix
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(pre, o, 64);
            if (lane >= o) pre += y;
        }
        const int sum = __shfl(pre, 63, 64);                 // the block's bits
        pre -= lc.bits();
        const unsigned long long b0 = off[g];
        const int s0 = (int)(b0 & 31);
        int p = s0 + pre;
        for (int z = 0; z < lc.nzrl; ++z, p += (int)(lc.zrl & 0xFF)) put_bits(buf[wv], p, lc.zrl >> 8, (int)(lc.zrl & 0xFF));
        put_bits(buf[wv], p, lc.piece, lc.plen);
        // With intervals k_jpeg_scan has added the padding and the marker to bits[g]; without, bits[g] is the block's own bits and
        // spares the shuffle.  `pend` below is read from bits[g] in the first case and derived from the rule in the second:
        // both MUST equal end + padding + marker bits, which is what the scan added.  (Deriving it in both forms measured 4 %
        // slower with intervals: profiles/jpeg_refactor_kernel_stats.csv, alt_ rows.)
        const int end = s0 + (L::kIntervals ? sum : (int)bits[g]);
        // end of interval: pad with 1-bits to a byte, then the marker unless the interval is the frame's last
        const bool ends = lay.ends_interval(j, blocks);
        const int iv = lay.interval_of(j);
        const bool marker = ends && iv < lay.nint() - 1;
        if (lane == 0 && ends) {
            if (end & 7) put_bits(buf[wv], end, 0xFFu >> (end & 7), 8 - (end & 7));
            if (marker) put_bits(buf[wv], (end + 7) & ~7, 0xFFD0u | (uint32_t)(iv & 7), 16);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int pend = L::kIntervals ? s0 + (int)bits[g] : ends ? (end + 7) & ~7 : end;   // the block's words include both
        const int nwords = (pend + 31) >> 5;
        if (lane < nwords) {
            const uint32_t v = __builtin_bswap32(buf[wv][lane]);
            if (lane == 0) first[g] = v;
            else if (lane == nwords - 1) last[g] = v;
            else scratch[(size_t)f * (scratch_per_frame >> 2) + (b0 >> 5) + lane] = v;
        }
    }
}

__device__ __forceinline__ void word_range(const unsigned long long* off, const uint32_t* bits, long long g, bool last_block,
                                           unsigned long long& wf, unsigned long long& wl) {
    unsigned long long end = off[g] + bits[g];
    if (last_block) end = (end + 7) & ~7ull;
    wf = off[g] >> 5;
    wl = (end - 1) >> 5;
}

// grid ceil(frames * blocks / 256), 256 threads: the words blocks share.  Block g writes its first word unless the previous block
// ends in it, and its last word: each is the OR of its own part and the first words of the following blocks that start there.
// With intervals bits[] already holds every padding (k_jpeg_scan); without, the frame's last block is padded here.
template <class L, class... LA>
__global__ __launch_bounds__(256) void k_jpeg_edges(int blocks, long long total, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ last, size_t scratch_per_frame,
                                                    uint32_t* __restrict__ scratch, LA...) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const long long f = g / blocks;
    const int j = (int)(g - f * blocks);
    uint32_t* fs = scratch + (size_t)f * (scratch_per_frame >> 2);
    unsigned long long wf, wl, pf, pl;
    word_range(off, bits, g, !L::kIntervals && j == blocks - 1, wf, wl);
    auto merged = [&](unsigned long long w, uint32_t v) {   // OR in the first words of the blocks after g that start in word w
        for (int h = j + 1; h < blocks; ++h) {
            unsigned long long hf, hl;
            word_range(off, bits, g + (h - j), !L::kIntervals && h == blocks - 1, hf, hl);
            if (hf != w) break;
            v |= first[g + (h - j)];
        }
        return v;
    };
    bool own_first = true;
    if (j > 0) {
        word_range(off, bits, g - 1, false, pf, pl);
        own_first = pl < wf;
    }
    if (own_first) fs[wf] = merged(wf, first[g]);
    if (wl > wf) fs[wl] = merged(wl, last[g]);
}

// whether the 0xFF at byte p of a frame's stream is the first byte of a restart marker (interval k's marker ends at ist[k + 1])
__device__ __forceinline__ bool marker_at(const unsigned long long* __restrict__ is, int nint, unsigned long long p) {
    int lo = 1, hi = nint;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (is[mid] < p + 2) lo = mid + 1; else hi = mid;
    }
    return lo < nint && is[lo] == p + 2;
}

// The stuffing rule: byte b at position p of a frame's stream (is: the frame's interval starts) gets a 0 after it when it is
// 0xFF and not the first byte of a restart marker.  k_jpeg_ffcount counts by it what k_jpeg_scatter writes by it.
template <class L>
__device__ __forceinline__ bool stuffed(const L& lay, const unsigned long long* __restrict__ is, uint32_t b, unsigned long long p) {
    return b == 0xFF && !(L::kIntervals && lay.nint() > 1 && marker_at(is, lay.nint(), p));
}

__device__ __forceinline__ uint8_t byte_of(const uint32_t (&w)[4], int k) { return (uint8_t)(w[k >> 2] >> (8 * (k & 3))); }

// grid (segments per frame, frames of the chunk), 256 threads: bytes to stuff per 4 KiB segment of the scan
template <class L, class... LA>
__global__ __launch_bounds__(256) void k_jpeg_ffcount(const uint8_t* __restrict__ scratch, size_t scratch_per_frame,
                                                      const unsigned long long* __restrict__ fbits, int segs_per_frame,
                                                      uint32_t* __restrict__ segcnt, const unsigned long long* __restrict__ ist, LA... la) {
    const L lay{la...};
    __shared__ int sh[4];
    const int f = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
    const unsigned long long nbytes = (fbits[f] + 7) >> 3;
    const unsigned long long i0 = (unsigned long long)seg * kSeg + tid * 16;
    if ((unsigned long long)seg * kSeg >= nbytes) {          // workgroup-uniform
        if (tid == 0) segcnt[(size_t)f * segs_per_frame + seg] = 0;
        return;
    }
    int cnt = 0;
    if (i0 < nbytes) {
        const uint4 q = *reinterpret_cast<const uint4*>(scratch + (size_t)f * scratch_per_frame + i0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        for (int k = 0; k < 16; ++k) cnt += (i0 + k < nbytes) && stuffed(lay, ist + (size_t)f * lay.nint(), byte_of(w, k), i0 + k);
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) sh[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) segcnt[(size_t)f * segs_per_frame + seg] = (uint32_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// one 1024-thread workgroup per chunk: segment counts -> offsets, frame sizes, output offsets (frame f0 + k starts at foff[f0 + k])
__global__ __launch_bounds__(1024) void k_jpeg_sizes(uint32_t* __restrict__ segcnt, int segs_per_frame,
                                                     const unsigned long long* __restrict__ fbits, int frames, int f0, int hdr_len,
                                                     const int* __restrict__ hlen, long long* __restrict__ fsize,
                                                     long long* __restrict__ foff) {   // hlen: a header length per frame (optimize)
    __shared__ unsigned long long sh[1024];
    for (int f = 0; f < frames; ++f) {
        const unsigned long long nbytes = (fbits[f] + 7) >> 3;
        const long long nseg = (long long)((nbytes + kSeg - 1) / kSeg);
        uint32_t* c = segcnt + (size_t)f * segs_per_frame;
        const unsigned long long ff = block_exclusive_scan<unsigned long long>(
            [&](long long i) { return (unsigned long long)c[i]; }, [&](long long i, unsigned long long v) { c[i] = (uint32_t)v; }, nseg, sh);
        if (threadIdx.x == 0) {
            const long long size = (long long)((hlen ? hlen[f] : hdr_len) + nbytes + ff + 2);
            fsize[f0 + f] = size;
            foff[f0 + f + 1] = foff[f0 + f] + size;
        }
        __syncthreads();
    }
}

// grid (segments per frame, frames of the chunk), 256 threads: header, stuffed scan bytes and EOI of each frame that fits.
// Restart markers are copied unstuffed; hlen != nullptr: frame f's header is hlen[f] bytes at hdr + f * hdr_stride (optimize)
template <class L, class... LA>
__global__ __launch_bounds__(256) void k_jpeg_scatter(const uint8_t* __restrict__ scratch, size_t scratch_per_frame,
                                                      const unsigned long long* __restrict__ fbits, const uint32_t* __restrict__ segoff,
                                                      int segs_per_frame, const uint8_t* __restrict__ hdr, int hdr_len, int f0,
                                                      const long long* __restrict__ fsize, const long long* __restrict__ foff,
                                                      uint8_t* __restrict__ out, long long capacity,
                                                      const unsigned long long* __restrict__ ist, int hdr_stride,
                                                      const int* __restrict__ hlen, LA... la) {
    const L lay{la...};
    __shared__ int sh[256];
    const int f = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
    if (L::kIntervals && hlen) { hdr += (size_t)f * hdr_stride; hdr_len = hlen[f]; }
    const unsigned long long nbytes = (fbits[f] + 7) >> 3;
    const long long o = foff[f0 + f], size = fsize[f0 + f];
    if (o + size > capacity) return;                         // the caller grows its buffer and re-runs
    if ((unsigned long long)seg * kSeg >= nbytes && seg != 0) return;
    uint8_t* dst = out + o;
    if (seg == 0) {
        for (int i = tid; i < hdr_len; i += 256) dst[i] = hdr[i];
        if (tid == 0) { dst[size - 2] = 0xFF; dst[size - 1] = 0xD9; }
    }
    const unsigned long long i0 = (unsigned long long)seg * kSeg + tid * 16;
    uint32_t w[4] = {0, 0, 0, 0};
    int cnt = 0;
    if (i0 < nbytes) {
        const uint4 q = *reinterpret_cast<const uint4*>(scratch + (size_t)f * scratch_per_frame + i0);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        for (int k = 0; k < 16; ++k) cnt += (i0 + k < nbytes) && stuffed(lay, ist + (size_t)f * lay.nint(), byte_of(w, k), i0 + k);
    }
    sh[tid] = cnt;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        const int add = tid >= s ? sh[tid - s] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    if (i0 >= nbytes) return;
    unsigned long long q = hdr_len + i0 + segoff[(size_t)f * segs_per_frame + seg] + (unsigned long long)(sh[tid] - cnt);
    for (int k = 0; k < 16 && i0 + k < nbytes; ++k) {
        const uint8_t b = byte_of(w, k);
        dst[q++] = b;
        if (stuffed(lay, ist + (size_t)f * lay.nint(), b, i0 + k)) dst[q++] = 0;
    }
}

// optimize, pass 1.  grid (ceil(blocks / 64), frames of the chunk), 256 threads: a wave per block, 16 blocks per wave; the symbols
// the entropy coder will emit, counted in LDS and added to the frame's four histograms [DC luma, AC luma, DC chroma, AC chroma]
// (exact integer counts: the order of the additions is free).  hist is zeroed before the launch.
__global__ __launch_bounds__(256) void k_jpeg_hist(const int16_t* __restrict__ coef, int blocks, uint32_t* __restrict__ hist, RunLayout lay) {
    __shared__ uint32_t h[kHist];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, f = blockIdx.y;
    for (int i = tid; i < kHist; i += 256) h[i] = 0;
    __syncthreads();
    const int16_t* fcoef = coef + (size_t)f * blocks * 64;
    for (int it = 0; it < 16; ++it) {
        const int j = blockIdx.x * 64 + it * 4 + wv;
        if (j >= blocks) break;                              // wave-uniform
        const int pred = lane == 0 ? dc_pred(lay, fcoef, j) : 0;
        const int t = table_of(lay, j);
        const int v = fcoef[(size_t)j * 64 + lane];
        const unsigned long long mask = __ballot(v != 0);
        if (lane == 0) {
            const int diff = v - pred;
            atomicAdd(&h[(2 * t) * 256 + nbits_of(diff < 0 ? -diff : diff)], 1u);
        } else if (v != 0) {
            const int run = run_before(mask, lane);
            if (run >> 4) atomicAdd(&h[(2 * t + 1) * 256 + 0xF0], (uint32_t)(run >> 4));
            atomicAdd(&h[(2 * t + 1) * 256 + (((run & 15) << 4) | nbits_of(v < 0 ? -v : v))], 1u);
        } else if (lane == 63) {
            atomicAdd(&h[(2 * t + 1) * 256], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < kHist; i += 256)
        if (h[i]) atomicAdd(&hist[(size_t)f * kHist + i], h[i]);
}

// optimize, between the passes.  grid = frames of the chunk, 256 threads: wave t builds table t of the frame on its lane 0
// (trl_jpeg_hufftab: a sequential procedure), then the workgroup writes the frame's code table and its header: the common header
// up to the first DHT, the four DHTs in the order DC luma, AC luma, DC chroma, AC chroma, and the common header's DRI / SOS tail.
__global__ __launch_bounds__(256) void k_jpeg_tables(const uint32_t* __restrict__ hist, const JTab* __restrict__ tab,
                                                     const uint8_t* __restrict__ hdr, int hdr_len, int dht_at, int tail_at,
                                                     JTab* __restrict__ ftab, uint8_t* __restrict__ fhdr, int fhdr_stride,
                                                     int* __restrict__ hlen) {
    __shared__ trl_hufftab_work work[4];
    __shared__ uint8_t hb[4][16], hv[4][256];
    __shared__ int nv[4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, f = blockIdx.x;
    JTab* ft = ftab + f;
    if (lane == 0) {
        nv[wv] = trl_jpeg_hufftab(hist + (size_t)f * kHist + wv * 256, hb[wv], hv[wv], &work[wv], nullptr);
        uint32_t* codes = (wv & 1) ? ft->ac[wv >> 1] : ft->dc[wv >> 1];
        int code = 0, k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < hb[wv][len - 1]; ++i) codes[hv[wv][k++]] = ((uint32_t)code++ << 8) | (uint32_t)len;
            code <<= 1;
        }
    }
    for (int i = tid; i < 128; i += 256) ft->qdiv[i >> 6][i & 63] = tab->qdiv[i >> 6][i & 63];
    __syncthreads();
    uint8_t* o = fhdr + (size_t)f * fhdr_stride;
    for (int i = tid; i < dht_at; i += 256) o[i] = hdr[i];
    int at = dht_at;
    for (int t = 0; t < 4; ++t) {
        const int n = nv[t], len = 2 + 1 + 16 + n;
        for (int i = tid; i < 5 + 16 + n; i += 256) {
            uint8_t v;
            if (i == 0) v = 0xFF;
            else if (i == 1) v = 0xC4;
            else if (i == 2) v = (uint8_t)(len >> 8);
            else if (i == 3) v = (uint8_t)len;
            else if (i == 4) v = (uint8_t)(((t & 1) << 4) | (t >> 1));
            else if (i < 21) v = hb[t][i - 5];
            else v = hv[t][i - 21];
            o[at + i] = v;
        }
        at += 2 + len;
    }
    for (int i = tid; i < hdr_len - tail_at; i += 256) o[at + i] = hdr[tail_at + i];
    if (tid == 0) hlen[f] = at + hdr_len - tail_at;
}

}  // namespace

struct trl_jpeg {
    int device = 0, H = 0, W = 0, quality = 0, max_frames = 0;
    int mcux = 0, mcuy = 0, blocks = 0, chunk = 0, segs_per_frame = 0, hdr_len = 0;
    size_t scratch_per_frame = 0;
    void* mem = nullptr;                 // one allocation, carved below
    JTab* tab = nullptr;
    uint8_t* hdr = nullptr;
    int16_t* coef = nullptr;
    uint32_t* bits = nullptr;
    unsigned long long* off = nullptr;
    unsigned long long* fbits = nullptr;
    uint32_t* segcnt = nullptr;
    uint32_t* first = nullptr;           // per block: its first / last scan word (k_jpeg_emit -> k_jpeg_edges)
    uint32_t* last = nullptr;
    uint8_t* scratch = nullptr;
    long long* fsize = nullptr;          // [max_frames]
    long long* foff = nullptr;           // [max_frames + 1]
    long long* h_sizes = nullptr;        // pinned [max_frames]
    // the optioned path (JOpt::ex()): blocks per MCU, the interval in MCUs (no DRI: the MCU count), intervals per frame
    bool ex = false, optimize = false;
    int sampling = 2, bpm = 6, R = 0, nint = 1, dht_at = 0, tail_at = 0;
    unsigned long long* ist = nullptr;   // [chunk][nint] interval byte starts
    unsigned long long* ibase = nullptr; // [chunk][nint] interval bit starts before padding (k_jpeg_scan's own)
    uint32_t* hist = nullptr;            // optimize: [chunk][4][256] symbol counts
    JTab* ftab = nullptr;                //           [chunk] code tables
    uint8_t* fhdr = nullptr;             //           [chunk][kHdrCap] headers
    int* hlen = nullptr;                 //           [chunk] their lengths
};

// The device workspace of an encoder that runs C frames at a time, carved from `a` into e's pointers; over a counting arena, its
// size.  The only place that knows what a block or a frame costs: e->chunk and the allocation come from dry runs of it.
static void carve(Arena& a, size_t C, trl_jpeg* e) {
    auto take = [&](auto*& p, size_t n) { p = static_cast<std::remove_reference_t<decltype(p)>>(a.alloc(n * sizeof(*p))); };
    const size_t B = C * (size_t)e->blocks, NI = e->ex ? C * (size_t)e->nint : 0;
    take(e->tab, 1); take(e->hdr, kHdrCap);
    take(e->coef, B * 64); take(e->bits, B); take(e->off, B); take(e->first, B); take(e->last, B);
    take(e->fbits, C); take(e->segcnt, C * e->segs_per_frame); take(e->scratch, C * e->scratch_per_frame);
    take(e->fsize, (size_t)e->max_frames); take(e->foff, (size_t)e->max_frames + 1);
    take(e->ist, NI); take(e->ibase, NI);
    if (e->optimize) { take(e->hist, C * kHist); take(e->ftab, C); take(e->fhdr, C * kHdrCap); take(e->hlen, C); }
}

// One stage of the pipeline: kernel k<FixedLayout>(args) or, for an encoder with options, k<RunLayout>(args, lay).
#define JPEG_STAGE(k, grid, block, ...)                                                                          \
    do {                                                                                                         \
        if (e->ex) hipLaunchKernelGGL((k<RunLayout, RunLayout>), grid, block, 0, s, __VA_ARGS__, lay);           \
        else hipLaunchKernelGGL((k<FixedLayout>), grid, block, 0, s, __VA_ARGS__);                               \
        TRL_LAUNCH_CHECK();                                                                                      \
    } while (0)

template <int S>
static void launch_blocks(const trl_jpeg* e, const uint8_t* src, long long frame_stride, int cn, hipStream_t s) {
    hipLaunchKernelGGL(k_jpeg_blocks<S>, dim3((e->mcux + Sampling<S>::kMcus - 1) / Sampling<S>::kMcus, e->mcuy, cn), dim3(256), 0, s, src,
                       frame_stride, e->H, e->W, e->mcux, e->mcuy, e->tab, e->coef);
}

// frames f0 .. f0 + cn of a batch, cn <= e->chunk: every kernel of the pipeline, on stream s
static int encode_chunk(trl_jpeg* e, const uint8_t* src, long long frame_stride, int cn, int f0, uint8_t* d_out, long long capacity,
                        hipStream_t s) {
    const long long total = (long long)cn * e->blocks;
    const RunLayout lay{e->bpm, e->R, e->nint, e->optimize ? 1 : 0};
    if (e->sampling == 2) launch_blocks<2>(e, src, frame_stride, cn, s);
    else if (e->sampling == 1) launch_blocks<1>(e, src, frame_stride, cn, s);
    else launch_blocks<0>(e, src, frame_stride, cn, s);
    TRL_LAUNCH_CHECK();
    const JTab* tab = e->tab;
    if (e->optimize) {                                       // a table and a header per frame, made on the device
        TRL_HIP(hipMemsetAsync(e->hist, 0, (size_t)cn * kHist * sizeof(*e->hist), s));
        hipLaunchKernelGGL(k_jpeg_hist, dim3((e->blocks + 63) / 64, cn), dim3(256), 0, s, e->coef, e->blocks, e->hist, lay);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_tables, dim3(cn), dim3(256), 0, s, e->hist, e->tab, e->hdr, e->hdr_len, e->dht_at, e->tail_at, e->ftab,
                           e->fhdr, kHdrCap, e->hlen);
        TRL_LAUNCH_CHECK();
        tab = e->ftab;
    }
    const dim3 waves((unsigned)((total + 3) / 4)), threads((unsigned)((total + 255) / 256)), segs(e->segs_per_frame, cn);
    JPEG_STAGE(k_jpeg_bits, waves, dim3(256), e->coef, e->blocks, total, tab, e->bits);
    JPEG_STAGE(k_jpeg_scan, dim3(cn), dim3(1024), e->bits, e->blocks, e->off, e->fbits, e->ist, e->ibase);
    JPEG_STAGE(k_jpeg_emit, waves, dim3(256), e->coef, e->blocks, total, tab, e->off, e->bits, e->scratch_per_frame,
               (uint32_t*)e->scratch, e->first, e->last);
    JPEG_STAGE(k_jpeg_edges, threads, dim3(256), e->blocks, total, e->off, e->bits, e->first, e->last, e->scratch_per_frame,
               (uint32_t*)e->scratch);
    JPEG_STAGE(k_jpeg_ffcount, segs, dim3(256), e->scratch, e->scratch_per_frame, e->fbits, e->segs_per_frame, e->segcnt, e->ist);
    hipLaunchKernelGGL(k_jpeg_sizes, dim3(1), dim3(1024), 0, s, e->segcnt, e->segs_per_frame, e->fbits, cn, f0, e->hdr_len, e->hlen,
                       e->fsize, e->foff);
    TRL_LAUNCH_CHECK();
    JPEG_STAGE(k_jpeg_scatter, segs, dim3(256), e->scratch, e->scratch_per_frame, e->fbits, e->segcnt, e->segs_per_frame,
               e->optimize ? e->fhdr : e->hdr, e->hdr_len, f0, e->fsize, e->foff, d_out, capacity, e->ist, e->optimize ? kHdrCap : 0,
               e->hlen);
    return TRL_OK;
}
#undef JPEG_STAGE

static int jpeg_header(const char* who, int H, int W, const trl_jpeg_options* opt, uint8_t* buf, size_t cap, int* len) {
    JOpt o;
    TRL_CHECK(resolve_options(who, H, W, opt, &o));
    if (!len || (!buf && cap)) { trl_set_error("%s: null argument", who); return TRL_ERR_INVALID; }
    const size_t n = header_bytes(H, W, o.quality, o.sampling, o.dri, nullptr);
    *len = (int)n;
    if (cap < n) { trl_set_error("%s: %zu bytes needed, capacity %zu", who, n, cap); return TRL_ERR_CAPACITY; }
    header_bytes(H, W, o.quality, o.sampling, o.dri, buf);
    return TRL_OK;
}

static int jpeg_create(const char* who, int device, int H, int W, const trl_jpeg_options* opt, int max_frames, trl_jpeg** out);

extern "C" {

int trl_jpeg_header(int H, int W, int quality, uint8_t* buf, size_t cap, int* len) {
    const trl_jpeg_options opt = {quality, 2, 0, 0, 0};
    return jpeg_header("trl_jpeg_header", H, W, &opt, buf, cap, len);
}

int trl_jpeg_header_ex(int H, int W, const trl_jpeg_options* opt, uint8_t* buf, size_t cap, int* len) {
    return jpeg_header("trl_jpeg_header_ex", H, W, opt, buf, cap, len);
}

int trl_jpeg_optimal_table(const uint32_t* hist, uint8_t* bits, uint8_t* vals, int* nvals, int* maxlen) {
    if (!hist || !bits || !vals || !nvals) { trl_set_error("trl_jpeg_optimal_table: null argument"); return TRL_ERR_INVALID; }
    trl_hufftab_work w;
    *nvals = trl_jpeg_hufftab(hist, bits, vals, &w, maxlen);
    return TRL_OK;
}

int trl_jpeg_create(int device, int H, int W, int quality, int max_frames, trl_jpeg** out) {
    const trl_jpeg_options opt = {quality, 2, 0, 0, 0};
    return jpeg_create("trl_jpeg_create", device, H, W, &opt, max_frames, out);
}

int trl_jpeg_create_ex(int device, int H, int W, const trl_jpeg_options* opt, int max_frames, trl_jpeg** out) {
    return jpeg_create("trl_jpeg_create_ex", device, H, W, opt, max_frames, out);
}

int trl_jpeg_destroy(trl_jpeg* e) {
    if (!e) return TRL_OK;
    (void)hipSetDevice(e->device);
    (void)hipFree(e->mem);
    (void)hipHostFree(e->h_sizes);
    delete e;
    return TRL_OK;
}

int trl_jpeg_encode(trl_jpeg* e, const uint8_t* d_bgr, int n, long long frame_stride, uint8_t* d_out, long long capacity,
                    long long* h_sizes, void* stream) {
    if (!e) { trl_set_error("trl_jpeg_encode: null encoder"); return TRL_ERR_INVALID; }
    if (n < 0 || n > e->max_frames) { trl_set_error("trl_jpeg_encode: n = %d outside 0..%d", n, e->max_frames); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_bgr || !h_sizes || capacity < 0 || (capacity > 0 && !d_out)) { trl_set_error("trl_jpeg_encode: null argument"); return TRL_ERR_INVALID; }
    if (n > 1 && frame_stride < (long long)e->H * e->W * 3) {
        trl_set_error("trl_jpeg_encode: frame stride %lld < %d x %d x 3", frame_stride, e->H, e->W);
        return TRL_ERR_INVALID;
    }
    TRL_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    TRL_HIP(hipMemsetAsync(e->foff, 0, sizeof(long long), s));
    for (int f0 = 0; f0 < n; f0 += e->chunk)
        TRL_CHECK(encode_chunk(e, d_bgr + (size_t)f0 * frame_stride, frame_stride, std::min(e->chunk, n - f0), f0, d_out, capacity, s));
    TRL_HIP(hipMemcpyAsync(e->h_sizes, e->fsize, (size_t)n * sizeof(*e->fsize), hipMemcpyDeviceToHost, s));
    TRL_HIP(hipStreamSynchronize(s));
    memcpy(h_sizes, e->h_sizes, (size_t)n * sizeof(*e->fsize));
    return TRL_OK;
}

}  // extern "C"

static int jpeg_create(const char* who, int device, int H, int W, const trl_jpeg_options* opt, int max_frames, trl_jpeg** out) {
    if (!out) { trl_set_error("%s: null argument", who); return TRL_ERR_INVALID; }
    *out = nullptr;
    JOpt o;
    TRL_CHECK(resolve_options(who, H, W, opt, &o));
    if (max_frames < 1 || max_frames > 65535) { trl_set_error("%s: max_frames %d outside 1..65535", who, max_frames); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(device));
    trl_jpeg* e = new trl_jpeg;
    e->device = device; e->H = H; e->W = W; e->quality = o.quality; e->max_frames = max_frames;
    e->mcux = o.mcux; e->mcuy = o.mcuy; e->blocks = e->mcux * e->mcuy * o.bpm;
    e->ex = o.ex(); e->optimize = o.optimize; e->sampling = o.sampling; e->bpm = o.bpm;
    const int nmcu = e->mcux * e->mcuy;
    e->R = o.dri > 0 ? o.dri : nmcu;
    e->nint = (nmcu + e->R - 1) / e->R;
    e->scratch_per_frame = (size_t)e->blocks * (kMaxBlockBits / 8);
    e->segs_per_frame = (int)((e->scratch_per_frame + kSeg - 1) / kSeg);
    auto bytes = [&](size_t C) { Arena count = Arena::counter(0); carve(count, C, e); return count.off; };
    e->chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)max_frames, kChunkBudget / (bytes(1) - bytes(0))));
    const size_t total = bytes((size_t)e->chunk);
    uint8_t hdr[kHdrCap];
    e->hdr_len = (int)header_bytes(H, W, o.quality, o.sampling, o.dri, hdr, &e->dht_at, &e->tail_at);
    JTab tab;
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(o.quality, t, q);
        for (int i = 0; i < 64; ++i) tab.qdiv[t][i] = (uint16_t)(8 * q[i]);
        uint8_t dcv[12];
        for (int i = 0; i < 12; ++i) dcv[i] = (uint8_t)i;
        uint32_t dc[256] = {0}, ac[256] = {0};
        huff_codes(kDcBits[t], dcv, dc);
        huff_codes(kAcBits[t], kAcVals[t], ac);
        memcpy(tab.dc[t], dc, sizeof(tab.dc[t]));
        memcpy(tab.ac[t], ac, sizeof(tab.ac[t]));
    }
    hipError_t st = hipMalloc(&e->mem, total);
    if (st == hipSuccess) st = hipHostMalloc((void**)&e->h_sizes, (size_t)max_frames * sizeof(*e->h_sizes), hipHostMallocDefault);
    if (st != hipSuccess) {
        trl_set_error("%s: %zu device bytes for %d x %d frames: %s", who, total, W, H, hipGetErrorString(st));
        if (e->mem) (void)hipFree(e->mem);
        delete e;
        return TRL_ERR_HIP;
    }
    Arena a = Arena::over(e->mem, total);
    carve(a, (size_t)e->chunk, e);
    st = hipMemcpy(e->tab, &tab, sizeof(JTab), hipMemcpyHostToDevice);
    if (st == hipSuccess) st = hipMemcpy(e->hdr, hdr, e->hdr_len, hipMemcpyHostToDevice);
    if (st != hipSuccess) {
        trl_set_error("%s: %s", who, hipGetErrorString(st));
        (void)hipFree(e->mem); (void)hipHostFree(e->h_sizes);
        delete e;
        return TRL_ERR_HIP;
    }
    *out = e;
    return TRL_OK;
}

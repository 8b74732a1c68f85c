// trl_jpeg.hip -- baseline Motion-JPEG encoder for run()'s annotated output, byte-identical to Pillow's
// Image.save(format="JPEG", quality=q, subsampling=2) (libjpeg-turbo's baseline path: 4:2:0, standard tables, no restart markers,
// no optimisation).  Integer arithmetic only, so the bytes do not depend on the launch shape.  The rules (DESIGN.md "Motion-JPEG
// on the device"; restated in numpy and pinned to Pillow by tests/test_jpeg_cpu.py):
//   colour      jccolor's 16-bit fixed point, BGR input
//   edges       Y: last column / row replicated to whole blocks; chroma: full-resolution columns replicated to whole chroma
//               blocks x 2, rows to an even count, h2v2 average with bias 1,2,1,2..., last chroma row replicated to whole blocks
//   FDCT        jfdctint islow (CONST_BITS 13, PASS1_BITS 2) on sample - 128; quantisation (|c| + 4q) / 8q, sign restored
//   dummies     Y blocks past the image in the last MCU column / row: zero AC, DC of the left neighbour (right edge) or of the
//               MCU's Y01 (bottom edge)
//   entropy     Annex K tables, DC predictor per component, ZRL / EOB, last byte padded with 1-bits, 0xFF stuffed as FF 00
// Pipeline per chunk of frames (all on the caller's stream; one host synchronisation per batch, to read the sizes):
//   k_jpeg_blocks   a workgroup = 4 MCUs of one MCU row: BGR -> YCbCr + downsampling into LDS, FDCT, quantisation, zigzag,
//                   dummy blocks -> int16 coefficients [frame][mcu][6][64]
//   k_jpeg_bits     one wave per block, lane k = zigzag coefficient k: ballot -> run lengths -> the block's bit count
//   k_jpeg_scan     one workgroup per frame: exclusive scan of the block bit counts
//   k_jpeg_emit     one wave per block: each lane ORs its codes into the wave's LDS words at (block offset + lane prefix); the
//                   words inside the block's range are stored, its first and last words set aside
//   k_jpeg_edges    one thread per block: the words blocks share, merged by the one block that owns each (no atomics)
//   k_jpeg_ffcount  FF bytes per 4 KiB segment of each frame's scan
//   k_jpeg_sizes    one workgroup per chunk: scan of the segment counts, frame sizes and output offsets
//   k_jpeg_scatter  header + stuffed scan + EOI into the caller's buffer; a frame that would end past the capacity is not written
#include "trl_common.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace {

constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
__constant__ int c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
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

constexpr int kMcuPerWg = 4;                  // k_jpeg_blocks: 4 MCUs = a 16 x 64 pixel strip, 24 blocks, 256 threads
constexpr int kMaxBlockBits = 1792;           // >= 22 (DC) + 63 x 27 (AC) + 3 ZRL x 11 + EOB: 224 scratch bytes per block
constexpr int kSeg = 4096;                    // bytes per stuffing segment (256 threads x 16 bytes)
constexpr size_t kChunkBudget = 256u << 20;   // device workspace per chunk of frames

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

size_t header_bytes(int H, int W, int quality, uint8_t* o) {   // o == nullptr: length only
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
    for (int v : {8, H >> 8, H & 0xFF, W >> 8, W & 0xFF, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) put(v);
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

// grid (ceil(mcux / 4), mcuy, frames of the chunk), 256 threads
__global__ __launch_bounds__(256) void k_jpeg_blocks(const uint8_t* __restrict__ src, long long frame_stride, int H, int W,
                                                     int mcux, int mcuy, const JTab* __restrict__ tab, int16_t* __restrict__ coef) {
    __shared__ int pix[3][16][64];            // Y, Cb, Cr of the strip at full resolution (edge-replicated source pixels)
    __shared__ int blk[24][64];               // centred samples -> FDCT output, natural order
    __shared__ int16_t qz[24][64];            // quantised, zigzag order
    const int tid = threadIdx.x, mx0 = blockIdx.x * kMcuPerWg, my = blockIdx.y, f = blockIdx.z;
    const uint8_t* fr = src + (size_t)f * frame_stride;
    for (int i = tid; i < 16 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        const int gy = min(16 * my + r, H - 1), gx = min(16 * mx0 + c, W - 1);
        const uint8_t* p = fr + ((size_t)gy * W + gx) * 3;
        const int B = p[0], G = p[1], R = p[2];
        pix[0][r][c] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        pix[1][r][c] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
        pix[2][r][c] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    }
    __syncthreads();
    const int crow_last = ((H + 1) >> 1) - 1 - 8 * my;           // last real chroma row of the strip (>= 0)
    for (int i = tid; i < 24 * 64; i += 256) {
        const int b = i >> 6, r = (i >> 3) & 7, c = i & 7, m = b / 6, kind = b % 6;
        int v;
        if (kind < 4) {
            v = pix[0][(kind >> 1) * 8 + r][m * 16 + (kind & 1) * 8 + c];
        } else {
            const int (*pl)[64] = pix[kind - 3];
            const int rr = 2 * min(r, crow_last), cc = 2 * (m * 8 + c);
            v = (pl[rr][cc] + pl[rr][cc + 1] + pl[rr + 1][cc] + pl[rr + 1][cc + 1] + 1 + (c & 1)) >> 2;
        }
        blk[b][(r << 3) | c] = v - 128;
    }
    __syncthreads();
    if (tid < 192) fdct8<true>(&blk[tid >> 3][(tid & 7) * 8], 1);
    __syncthreads();
    if (tid < 192) fdct8<false>(&blk[tid >> 3][tid & 7], 8);
    __syncthreads();
    for (int i = tid; i < 24 * 64; i += 256) {
        const int b = i >> 6, z = i & 63;
        const int c = blk[b][c_zigzag[z]], d = tab->qdiv[(b % 6) < 4 ? 0 : 1][c_zigzag[z]];
        const int a = ((c < 0 ? -c : c) + (d >> 1)) / d;
        qz[b][z] = (int16_t)(c < 0 ? -a : a);
    }
    __syncthreads();
    const int bw = (W + 7) >> 3, bh = (H + 7) >> 3;              // Y blocks holding image samples
    for (int i = tid; i < 24 * 64; i += 256) {
        const int b = i >> 6, z = i & 63, m = b / 6, kind = b % 6, mx = mx0 + m;
        if (mx >= mcux) continue;
        int v = qz[b][z];
        if (kind < 4) {
            const bool right = 2 * mx + (kind & 1) >= bw, bottom = 2 * my + (kind >> 1) >= bh;
            if (bottom) {                                        // the MCU's Y01 (itself a right dummy: Y00's DC)
                v = z ? 0 : (2 * mx + 1 >= bw ? qz[m * 6][0] : qz[m * 6 + 1][0]);
            } else if (right) {                                  // the left neighbour in the MCU
                v = z ? 0 : qz[b - 1][0];
            }
        }
        coef[(((size_t)f * mcuy + my) * mcux + mx) * 384 + kind * 64 + z] = (int16_t)v;
    }
}

__device__ __forceinline__ int nbits_of(int a) { return a ? 32 - __clz(a) : 0; }

// The codes of lane k of a block (lane = zigzag index).  Up to three ZRL codes and one (code, magnitude) piece, or the EOB on
// lane 63 when coefficient 63 is zero (its lane has no other bits, so the EOB lands at the block's end).
struct LaneCodes {
    uint32_t piece;   // (code << nb) | magnitude bits
    int plen;         // its length (0: none)
    int nzrl;         // ZRL codes before it
    uint32_t zrl;     // ZRL code << 8 | length
    __device__ int bits() const { return plen + nzrl * (int)(zrl & 0xFF); }
};

__device__ __forceinline__ LaneCodes lane_codes(const JTab* __restrict__ tab, const int16_t* __restrict__ blkc, int lane, int kind,
                                                int pred) {
    const int t = kind < 4 ? 0 : 1;
    const int v = blkc[lane];
    const unsigned long long mask = __ballot(v != 0);
    LaneCodes o{0u, 0, 0, tab->ac[t][0xF0]};
    if (lane == 0) {
        const int diff = v - pred, a = diff < 0 ? -diff : diff, nb = nbits_of(a);
        const uint32_t e = tab->dc[t][nb];
        o.piece = ((e >> 8) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u));
        o.plen = (int)(e & 0xFF) + nb;
    } else if (v != 0) {
        const unsigned long long below = mask & ((1ull << lane) - 1ull) & ~1ull;
        const int prev = below ? 63 - __clzll(below) : 0;
        const int run = lane - prev - 1, a = v < 0 ? -v : v, nb = nbits_of(a);
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

// the DC predictor of block j of a frame (component order in an MCU: Y00 Y01 Y10 Y11 Cb Cr)
__device__ __forceinline__ int dc_pred(const int16_t* __restrict__ fcoef, int j) {
    const int mcu = j / 6, kind = j % 6;
    if (kind >= 1 && kind <= 3) return fcoef[(size_t)(j - 1) * 64];
    if (mcu == 0) return 0;
    return fcoef[(size_t)(j - 6 + (kind == 0 ? 3 : 0)) * 64];
}

__device__ __forceinline__ int wave_sum(int x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// grid ceil(frames * blocks / 4), 256 threads: one wave per block
__global__ __launch_bounds__(256) void k_jpeg_bits(const int16_t* __restrict__ coef, int blocks, long long total,
                                                   const JTab* __restrict__ tab, uint32_t* __restrict__ bits) {
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= total) return;                                  // wave-uniform
    const long long f = g / blocks;
    const int j = (int)(g - f * blocks);
    const int16_t* fcoef = coef + (size_t)f * blocks * 64;
    const int pred = lane == 0 ? dc_pred(fcoef, j) : 0;
    const LaneCodes lc = lane_codes(tab, fcoef + (size_t)j * 64, lane, j % 6, pred);
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

// grid = frames of the chunk, 1024 threads: block bit offsets and the frame's scan length in bits
__global__ __launch_bounds__(1024) void k_jpeg_scan(const uint32_t* __restrict__ bits, int blocks, unsigned long long* __restrict__ off,
                                                    unsigned long long* __restrict__ fbits) {
    __shared__ unsigned long long sh[1024];
    const size_t f = blockIdx.x;
    const uint32_t* b = bits + f * blocks;
    unsigned long long* o = off + f * blocks;
    const unsigned long long t = block_exclusive_scan<unsigned long long>(
        [&](long long i) { return (unsigned long long)b[i]; }, [&](long long i, unsigned long long v) { o[i] = v; }, blocks, sh);
    if (threadIdx.x == 0) fbits[f] = t;
}

__device__ __forceinline__ void put_bits(uint32_t* w, int p, uint32_t val, int len) {   // big-endian bit order
    if (len <= 0) return;
    const unsigned long long x = (unsigned long long)val << (64 - (p & 31) - len);
    atomicOr(&w[p >> 5], (uint32_t)(x >> 32));
    if ((uint32_t)x) atomicOr(&w[(p >> 5) + 1], (uint32_t)x);
}

// grid ceil(frames * blocks / 4), 256 threads: one wave per block, LDS words per wave.  A block's words strictly inside its bit
// range are stored; its first and last words, which it may share with its neighbours, go to first[] / last[] for k_jpeg_edges.
// No word is written twice and there are no global atomics: per-XCD L2s are not coherent with each other within a kernel.
__global__ __launch_bounds__(256) void k_jpeg_emit(const int16_t* __restrict__ coef, int blocks, long long total,
                                                   const JTab* __restrict__ tab, const unsigned long long* __restrict__ off,
                                                   const uint32_t* __restrict__ bits, size_t scratch_per_frame,
                                                   uint32_t* __restrict__ scratch, uint32_t* __restrict__ first, uint32_t* __restrict__ last) {
    __shared__ uint32_t buf[4][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * 4 + wv;
    buf[wv][lane] = 0;
    __syncthreads();
    if (g < total) {                                         // wave-uniform
        const long long f = g / blocks;
        const int j = (int)(g - f * blocks);
        const int16_t* fcoef = coef + (size_t)f * blocks * 64;
        const int pred = lane == 0 ? dc_pred(fcoef, j) : 0;
        const LaneCodes lc = lane_codes(tab, fcoef + (size_t)j * 64, lane, j % 6, pred);
        int pre = lc.bits();                                 // inclusive -> exclusive wave prefix
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(pre, o, 64);
            if (lane >= o) pre += y;
        }
        pre -= lc.bits();
        const unsigned long long b0 = off[g];
        const int s0 = (int)(b0 & 31);
        int p = s0 + pre;
        for (int z = 0; z < lc.nzrl; ++z, p += (int)(lc.zrl & 0xFF)) put_bits(buf[wv], p, lc.zrl >> 8, (int)(lc.zrl & 0xFF));
        put_bits(buf[wv], p, lc.piece, lc.plen);
        const int end = s0 + (int)bits[g];
        if (j == blocks - 1 && lane == 0 && (end & 7)) put_bits(buf[wv], end, 0xFFu >> (end & 7), 8 - (end & 7));   // 1-bit padding
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int pend = j == blocks - 1 ? (end + 7) & ~7 : end;           // the last block's words include its padding
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
__global__ __launch_bounds__(256) void k_jpeg_edges(int blocks, long long total, const unsigned long long* __restrict__ off,
                                                    const uint32_t* __restrict__ bits, const uint32_t* __restrict__ first,
                                                    const uint32_t* __restrict__ last, size_t scratch_per_frame,
                                                    uint32_t* __restrict__ scratch) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const long long f = g / blocks;
    const int j = (int)(g - f * blocks);
    uint32_t* fs = scratch + (size_t)f * (scratch_per_frame >> 2);
    unsigned long long wf, wl, pf, pl;
    word_range(off, bits, g, j == blocks - 1, wf, wl);
    auto merged = [&](unsigned long long w, uint32_t v) {   // OR in the first words of the blocks after g that start in word w
        for (int h = j + 1; h < blocks; ++h) {
            unsigned long long hf, hl;
            word_range(off, bits, g + (h - j), h == blocks - 1, hf, hl);
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

// grid (segments per frame, frames of the chunk), 256 threads: FF bytes per 4 KiB segment of the scan
__global__ __launch_bounds__(256) void k_jpeg_ffcount(const uint8_t* __restrict__ scratch, size_t scratch_per_frame,
                                                      const unsigned long long* __restrict__ fbits, int segs_per_frame,
                                                      uint32_t* __restrict__ segcnt) {
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
        for (int k = 0; k < 16; ++k)
            cnt += (i0 + k < nbytes) && ((w[k >> 2] >> (8 * (k & 3))) & 0xFF) == 0xFF;
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) sh[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) segcnt[(size_t)f * segs_per_frame + seg] = (uint32_t)(sh[0] + sh[1] + sh[2] + sh[3]);
}

// one 1024-thread workgroup per chunk: segment counts -> offsets, frame sizes, output offsets (frame f0 + k starts at foff[f0 + k])
__global__ __launch_bounds__(1024) void k_jpeg_sizes(uint32_t* __restrict__ segcnt, int segs_per_frame,
                                                     const unsigned long long* __restrict__ fbits, int frames, int f0, int hdr_len,
                                                     long long* __restrict__ fsize, long long* __restrict__ foff) {
    __shared__ unsigned long long sh[1024];
    for (int f = 0; f < frames; ++f) {
        const unsigned long long nbytes = (fbits[f] + 7) >> 3;
        const long long nseg = (long long)((nbytes + kSeg - 1) / kSeg);
        uint32_t* c = segcnt + (size_t)f * segs_per_frame;
        const unsigned long long ff = block_exclusive_scan<unsigned long long>(
            [&](long long i) { return (unsigned long long)c[i]; }, [&](long long i, unsigned long long v) { c[i] = (uint32_t)v; }, nseg, sh);
        if (threadIdx.x == 0) {
            const long long size = (long long)(hdr_len + nbytes + ff + 2);
            fsize[f0 + f] = size;
            foff[f0 + f + 1] = foff[f0 + f] + size;
        }
        __syncthreads();
    }
}

// grid (segments per frame, frames of the chunk), 256 threads: header, stuffed scan bytes and EOI of each frame that fits
__global__ __launch_bounds__(256) void k_jpeg_scatter(const uint8_t* __restrict__ scratch, size_t scratch_per_frame,
                                                      const unsigned long long* __restrict__ fbits, const uint32_t* __restrict__ segoff,
                                                      int segs_per_frame, const uint8_t* __restrict__ hdr, int hdr_len, int f0,
                                                      const long long* __restrict__ fsize, const long long* __restrict__ foff,
                                                      uint8_t* __restrict__ out, long long capacity) {
    __shared__ int sh[256];
    const int f = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
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
        for (int k = 0; k < 16; ++k) cnt += (i0 + k < nbytes) && ((w[k >> 2] >> (8 * (k & 3))) & 0xFF) == 0xFF;
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
        const uint8_t b = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        dst[q++] = b;
        if (b == 0xFF) dst[q++] = 0;
    }
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
};

extern "C" {

int trl_jpeg_header(int H, int W, int quality, uint8_t* buf, size_t cap, int* len) {
    TRL_CHECK(check_shape(H, W));
    if (!len || (!buf && cap)) { trl_set_error("trl_jpeg_header: null argument"); return TRL_ERR_INVALID; }
    const size_t n = header_bytes(H, W, quality, nullptr);
    *len = (int)n;
    if (cap < n) { trl_set_error("trl_jpeg_header: %zu bytes needed, capacity %zu", n, cap); return TRL_ERR_CAPACITY; }
    header_bytes(H, W, quality, buf);
    return TRL_OK;
}

int trl_jpeg_create(int device, int H, int W, int quality, int max_frames, trl_jpeg** out) {
    if (!out) { trl_set_error("trl_jpeg_create: null argument"); return TRL_ERR_INVALID; }
    *out = nullptr;
    TRL_CHECK(check_shape(H, W));
    if (max_frames < 1 || max_frames > 65535) { trl_set_error("trl_jpeg_create: max_frames %d outside 1..65535", max_frames); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(device));
    trl_jpeg* e = new trl_jpeg;
    e->device = device; e->H = H; e->W = W; e->quality = quality; e->max_frames = max_frames;
    e->mcux = (W + 15) / 16; e->mcuy = (H + 15) / 16; e->blocks = e->mcux * e->mcuy * 6;
    e->scratch_per_frame = (size_t)e->blocks * (kMaxBlockBits / 8);
    e->segs_per_frame = (int)((e->scratch_per_frame + kSeg - 1) / kSeg);
    const size_t per_frame = (size_t)e->blocks * (128 + 4 + 8 + 8) + e->scratch_per_frame + (size_t)e->segs_per_frame * 4 + 8;
    e->chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)max_frames, kChunkBudget / per_frame));
    uint8_t hdr[1024];
    e->hdr_len = (int)header_bytes(H, W, quality, hdr);
    JTab tab;
    for (int t = 0; t < 2; ++t) {
        uint8_t q[64];
        quant_table(quality, t, q);
        for (int i = 0; i < 64; ++i) tab.qdiv[t][i] = (uint16_t)(8 * q[i]);
        uint8_t dcv[12];
        for (int i = 0; i < 12; ++i) dcv[i] = (uint8_t)i;
        uint32_t dc[256] = {0}, ac[256] = {0};
        huff_codes(kDcBits[t], dcv, dc);
        huff_codes(kAcBits[t], kAcVals[t], ac);
        memcpy(tab.dc[t], dc, sizeof(tab.dc[t]));
        memcpy(tab.ac[t], ac, sizeof(tab.ac[t]));
    }
    const size_t C = (size_t)e->chunk, B = (size_t)e->blocks;
    size_t sz[] = {sizeof(JTab), 1024, C * B * 128, C * B * 4, C * B * 8, C * 8, C * e->segs_per_frame * 4, C * e->scratch_per_frame,
                   (size_t)max_frames * 8, ((size_t)max_frames + 1) * 8, C * B * 4, C * B * 4};
    size_t total = 0, offs[12];
    for (int i = 0; i < 12; ++i) { offs[i] = total; total += (sz[i] + 255) & ~(size_t)255; }
    hipError_t st = hipMalloc(&e->mem, total);
    if (st == hipSuccess) st = hipHostMalloc((void**)&e->h_sizes, (size_t)max_frames * 8, hipHostMallocDefault);
    if (st != hipSuccess) {
        trl_set_error("trl_jpeg_create: %zu device bytes for %d x %d frames: %s", total, W, H, hipGetErrorString(st));
        if (e->mem) (void)hipFree(e->mem);
        delete e;
        return TRL_ERR_HIP;
    }
    uint8_t* m = (uint8_t*)e->mem;
    e->tab = (JTab*)(m + offs[0]); e->hdr = m + offs[1]; e->coef = (int16_t*)(m + offs[2]); e->bits = (uint32_t*)(m + offs[3]);
    e->off = (unsigned long long*)(m + offs[4]); e->fbits = (unsigned long long*)(m + offs[5]); e->segcnt = (uint32_t*)(m + offs[6]);
    e->scratch = m + offs[7]; e->fsize = (long long*)(m + offs[8]); e->foff = (long long*)(m + offs[9]);
    e->first = (uint32_t*)(m + offs[10]); e->last = (uint32_t*)(m + offs[11]);
    st = hipMemcpy(e->tab, &tab, sizeof(JTab), hipMemcpyHostToDevice);
    if (st == hipSuccess) st = hipMemcpy(e->hdr, hdr, e->hdr_len, hipMemcpyHostToDevice);
    if (st != hipSuccess) {
        trl_set_error("trl_jpeg_create: %s", hipGetErrorString(st));
        (void)hipFree(e->mem); (void)hipHostFree(e->h_sizes);
        delete e;
        return TRL_ERR_HIP;
    }
    *out = e;
    return TRL_OK;
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
    for (int f0 = 0; f0 < n; f0 += e->chunk) {
        const int cn = std::min(e->chunk, n - f0);
        const long long total = (long long)cn * e->blocks;
        hipLaunchKernelGGL(k_jpeg_blocks, dim3((e->mcux + kMcuPerWg - 1) / kMcuPerWg, e->mcuy, cn), dim3(256), 0, s,
                           d_bgr + (size_t)f0 * frame_stride, frame_stride, e->H, e->W, e->mcux, e->mcuy, e->tab, e->coef);
        TRL_LAUNCH_CHECK();
        const unsigned wgs = (unsigned)((total + 3) / 4);
        hipLaunchKernelGGL(k_jpeg_bits, dim3(wgs), dim3(256), 0, s, e->coef, e->blocks, total, e->tab, e->bits);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_scan, dim3(cn), dim3(1024), 0, s, e->bits, e->blocks, e->off, e->fbits);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_emit, dim3(wgs), dim3(256), 0, s, e->coef, e->blocks, total, e->tab, e->off, e->bits,
                           e->scratch_per_frame, (uint32_t*)e->scratch, e->first, e->last);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_edges, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, e->blocks, total, e->off, e->bits,
                           e->first, e->last, e->scratch_per_frame, (uint32_t*)e->scratch);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_ffcount, dim3(e->segs_per_frame, cn), dim3(256), 0, s, e->scratch, e->scratch_per_frame, e->fbits,
                           e->segs_per_frame, e->segcnt);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_sizes, dim3(1), dim3(1024), 0, s, e->segcnt, e->segs_per_frame, e->fbits, cn, f0, e->hdr_len,
                           e->fsize, e->foff);
        TRL_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_jpeg_scatter, dim3(e->segs_per_frame, cn), dim3(256), 0, s, e->scratch, e->scratch_per_frame, e->fbits,
                           e->segcnt, e->segs_per_frame, e->hdr, e->hdr_len, f0, e->fsize, e->foff, d_out, capacity);
        TRL_LAUNCH_CHECK();
    }
    TRL_HIP(hipMemcpyAsync(e->h_sizes, e->fsize, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    TRL_HIP(hipStreamSynchronize(s));
    memcpy(h_sizes, e->h_sizes, (size_t)n * 8);
    return TRL_OK;
}

}  // extern "C"

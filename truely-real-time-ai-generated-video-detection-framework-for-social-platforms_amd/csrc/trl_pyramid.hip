// trl_pyramid.hip -- the image pyramid of MTCNN stage 1 for gfx950: u8 BGR frames -> every pyramid level, imresample
// (F.interpolate mode="area") + (x-127.5)*0.0078125, stored as three floats {b,g,r} per pixel (12 B, streamed past the caches) for
// the fused PNet kernel (trl_pnet.hip), its only reader.
//
// Byte sums are integer (v_dot4 / packed 16-bit adds: exact in any order), bin edges come from host tables or exact multiply-high
// division, the bin mean from the exhaustively verified reciprocal division (pyr_div): every kernel below writes the same bits.
// Per batch of frames trl_pyramid_build launches, in this order,
//
//  k_pyramid_stream<4|8, OwnBlock>  the coarse levels (bins wider than 5 px) in ONE pass over the source, a workgroup per band of
//  k_pyramid_stream<4|8, OwnWave>   rows, or a WAVE per (band, column segment) for frames wider than 1,365 px: one kernel text;
//  k_pyramid_fine           the three finest levels (85 % of the pixels) in one pass, a wave per level and source tile;
//  k_pyramid0<3|4|5>        whatever the passes above cannot take (see the preconditions in launch_coarse / launch_fine), one launch
//  k_pyramid<1|2>           per (level, Infinity-Cache-sized frame chunk): one lane (mode 0) or lane group (modes 1, 2) per pixel.
#include "trl_pyramid.h"
#include <type_traits>

typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 bytes at dword alignment
struct __attribute__((packed, aligned(4))) u32x3_a4 { unsigned x, y, z; };
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));            // two 16-bit sums of a dword: packed adds, no carry between them

namespace {

// ---- one launch per level ----------------------------------------------------------------------------
// One LANE GROUP of G lanes per output pixel (G = 1, 4, 16 or 64 by level: coarse levels average
// thousands of source bytes per pixel, so their bins are split across lanes and summed with xor
// shuffles -- integer sums, exact in any order).  Bytes are fetched as aligned dwords; the three
// channel sums of a dword are three v_dot4_u32_u8 against 0/1 byte masks selected by the dword's
// phase (byte offset mod 3) inside the BGR span.
__device__ __forceinline__ void dword_sums(unsigned v, int rel, int nbytes, unsigned& s0, unsigned& s1, unsigned& s2) {
    // rel = byte offset of this dword relative to the first byte of the span (-3 .. nbytes-1)
    const int lo = rel < 0 ? -rel : 0;
    const int hi = (nbytes - rel) < 4 ? (nbytes - rel) : 4;
    const unsigned vm = (hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u)) & ~((1u << (8 * lo)) - 1u);
    v &= vm;
    const int phase = (rel + 3) % 3;   // channel of byte 0 of the dword
    const unsigned m0 = phase == 0 ? 0x01000001u : (phase == 1 ? 0x00010000u : 0x00000100u);
    const unsigned m1 = phase == 0 ? 0x00000100u : (phase == 1 ? 0x01000001u : 0x00010000u);
    const unsigned m2 = phase == 0 ? 0x00010000u : (phase == 1 ? 0x00000100u : 0x01000001u);
    s0 = __builtin_amdgcn_udot4(v, m0, s0, false);
    s1 = __builtin_amdgcn_udot4(v, m1, s1, false);
    s2 = __builtin_amdgcn_udot4(v, m2, s2, false);
}

// Bin edges are precomputed on the host (one packed (start | end<<16) word per output row / column of
// every level): the kernel does no 64-bit or repeated integer division.  grid = (blocks, frames).
// Three per-level modes (wave-uniform):
//   0  small bins (<= 5 px wide): one lane per pixel; each source row is 4-5 aligned dwords re-aligned to
//      the bin's first byte with v_alignbyte, so the BGR byte->channel masks are compile-time constants;
//   1  big bins, row pitch a multiple of 4 bytes: a lane owns one 12-byte group (4 whole pixels, constant
//      channel phase) of the bin for every (rl-th) source row: 3 coalesced loads + 9 v_dot4 per 12 bytes;
//   2  generic fallback (odd row pitch): flattened (row, dword) walk with per-dword masks.
__device__ __forceinline__ unsigned chan_mask(int p, int c) {   // dword whose byte 0 has channel p: bytes of channel c
    const int d = (c - p + 3) % 3;                               // byte index of the first byte of channel c
    return d == 0 ? 0x01000001u : (d == 1 ? 0x00000100u : 0x00010000u);
}
__device__ __forceinline__ unsigned valid_bytes(int rel, int nbytes) {   // 0xFF for bytes b of the dword with 0 <= rel+b < nbytes
    const int lo = rel < 0 ? -rel : 0;
    int hi = nbytes - rel; hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
    if (lo >= hi) return 0u;
    return (hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u)) & ~((1u << (8 * lo)) - 1u);
}

// The pyramid is written once and read once, much later, by the PNet kernel: stream it past the caches so the source
// frame (re-read by every level) keeps its L2 / Infinity Cache lines.
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pyr_store(PyrPx* dst, const float4& v) {
    static_assert(sizeof(PyrPx) == 12, "layout");
    f32x3_nt t = {v.x, v.y, v.z};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x3_nt*>(dst));
}

// Correctly rounded a / b from r = RN(1/b) (Markstein): q0 = RN(a r), e = a - b q0 (exact in one fma), q = RN(q0 + e r).
// For a = integer sums up to 255 kh kw and the bin sizes used here (kh, kw <= 96) the result equals the IEEE
// quotient for EVERY input -- checked exhaustively by the oracle's self test (oracle/trl_oracle.c:orc_selftest_recip_div);
// larger bins take the true division.  3 VALU ops instead of the ~11 of v_div_scale/v_rcp/v_div_fmas/v_div_fixup.
__device__ __forceinline__ float pyr_div(float a, float b, float r) {
    const float q0 = a * r;
    const float e = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(e, r, q0);
}
// s / kh / kw, normalised; r1 = RN(1/kh), r2 = RN(1/kw) when `fast`
__device__ __forceinline__ float pyr_norm(unsigned s, float fkh, float fkw, float r1, float r2, bool fast) {
    const float a = (float)s;
    const float q = fast ? pyr_div(pyr_div(a, fkh, r1), fkw, r2) : a / fkh / fkw;
    return (q - 127.5f) * 0.0078125f;
}
__device__ __forceinline__ float pyr_norm(unsigned s, int kh, int kw, const PyrBins& g) {
    const float a = (float)s, fkh = (float)kh, fkw = (float)kw;
    float q;
    if (g.fastdiv) {
        const float r1 = kh == g.khA ? g.rkh[0] : g.rkh[1], r2 = kw == g.kwA ? g.rkw[0] : g.rkw[1];
        q = pyr_div(pyr_div(a, fkh, r1), fkw, r2);
    } else {
        q = a / fkh / fkw;
    }
    return (q - 127.5f) * 0.0078125f;
}

struct PyrArgs { int H, W, n_frames, f0; long long pyr_stride; PyrLevel g; };

// threads q = q0, q0 + qstep, ... of level g of frame f
template <int MODE>
__device__ __forceinline__ void pyr_level(const uint8_t* __restrict__ frames, const PyrArgs& a, const PyrLevel& g, const uint32_t* __restrict__ tab,
                                          PyrPx* __restrict__ pyr, int f, int q0, int qstep) {
    const int per_frame = g.pix_pad << g.gshift;            // threads of this level per frame
    constexpr int mode = MODE;
    const uint32_t* base32 = reinterpret_cast<const uint32_t*>(frames);
    const long long fbase = (long long)f * a.H * a.W * 3;
    const long long last_dw = ((long long)a.n_frames * a.H * a.W * 3 - 1) >> 2;
    const int row_bytes = a.W * 3;
    for (int q = q0; q < per_frame; q += qstep) {
        const int w = g.w, gsh = g.gshift, G = 1 << gsh;
        const int pixel = q >> gsh, sub = q & (G - 1);
        const bool valid = pixel < g.h * w;
        unsigned s0 = 0, s1 = 0, s2 = 0;
        int kh = 1, kw = 1;
        if (valid) {
            int oy = (int)__umulhi((unsigned)pixel, g.wmagic);       // floor(pixel / w) or one above it (large levels): fix up
            oy -= (oy * w > pixel) ? 1 : 0;
            const int ox = pixel - oy * w;
            const uint32_t ty = tab[g.ytab0 + oy], tx = tab[g.xtab0 + ox];
            const int ys = ty & 0xFFFF, ye = ty >> 16, xs = tx & 0xFFFF, xe = tx >> 16;
            kh = ye - ys; kw = xe - xs;
            const int nbytes = kw * 3;
            const long long o0 = fbase + (long long)ys * row_bytes + xs * 3;   // first byte of the bin
            if (mode == 1) {
                const int grsh = g.grshift, grp = sub & ((1 << grsh) - 1), rlane = sub >> grsh, rl = G >> grsh;
                const int sh = (int)(o0 & 3);
                const int rel = -sh + 12 * grp;                      // offset of this lane's group relative to the bin's first byte
                if (rel < nbytes) {
                    const int ph = (3 - sh % 3) % 3;                 // channel of the byte at the aligned start (12*grp keeps it)
                    unsigned mk[3][3];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const unsigned vb = valid_bytes(rel + 4 * j, nbytes) & 0x01010101u;
#pragma unroll
                        for (int c = 0; c < 3; c++) mk[j][c] = chan_mask((ph + j) % 3, c) & vb;
                    }
                    long long dw = ((o0 - sh) >> 2) + 3 * grp + (long long)rlane * (row_bytes >> 2);
                    const long long dstep = (long long)rl * (row_bytes >> 2);
                    for (int y = rlane; y < kh; y += 4 * rl, dw += 4 * dstep) {
                        unsigned w3[4][3];
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const bool act = y + r * rl < kh;
                            const long long d = act ? dw + r * dstep : dw;
                            if (d + 2 <= last_dw) {
                                const u32x3_a4 v3 = *reinterpret_cast<const u32x3_a4*>(base32 + d);
                                w3[r][0] = v3.x; w3[r][1] = v3.y; w3[r][2] = v3.z;
                            } else {
                                w3[r][0] = base32[d]; w3[r][1] = base32[d + 1 <= last_dw ? d + 1 : last_dw]; w3[r][2] = base32[last_dw];
                            }
                            if (!act) { w3[r][0] = 0u; w3[r][1] = 0u; w3[r][2] = 0u; }
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            s0 = __builtin_amdgcn_udot4(w3[r][0], mk[0][0], s0, false); s1 = __builtin_amdgcn_udot4(w3[r][0], mk[0][1], s1, false);
                            s2 = __builtin_amdgcn_udot4(w3[r][0], mk[0][2], s2, false);
                            s0 = __builtin_amdgcn_udot4(w3[r][1], mk[1][0], s0, false); s1 = __builtin_amdgcn_udot4(w3[r][1], mk[1][1], s1, false);
                            s2 = __builtin_amdgcn_udot4(w3[r][1], mk[1][2], s2, false);
                            s0 = __builtin_amdgcn_udot4(w3[r][2], mk[2][0], s0, false); s1 = __builtin_amdgcn_udot4(w3[r][2], mk[2][1], s1, false);
                            s2 = __builtin_amdgcn_udot4(w3[r][2], mk[2][2], s2, false);
                        }
                    }
                }
            } else {
                const int ndw = (nbytes + 6) >> 2;            // dwords per row for the worst alignment
                int row = 0, d = sub;
                while (d >= ndw) { d -= ndw; row++; }
                while (row < kh) {
                    const long long o = o0 + (long long)row * row_bytes;
                    const long long al = (o & ~3ll) + 4 * d;
                    const int rel = (int)(al - o);
                    if (rel < nbytes) dword_sums(base32[al >> 2], rel, nbytes, s0, s1, s2);
                    d += G;
                    while (d >= ndw) { d -= ndw; row++; }
                }
            }
        }
        for (int off = G >> 1; off >= 1; off >>= 1) {
            s0 += __shfl_xor((int)s0, off, 64); s1 += __shfl_xor((int)s1, off, 64); s2 += __shfl_xor((int)s2, off, 64);
        }
        if (sub == 0 && pixel < g.pix_pad) {
            float4 o4;
            o4.x = valid ? pyr_norm(s0, kh, kw, g) : 0.f;
            o4.y = valid ? pyr_norm(s1, kh, kw, g) : 0.f;
            o4.z = valid ? pyr_norm(s2, kh, kw, g) : 0.f;
            o4.w = 0.f;
            pyr_store(pyr + ((long long)f * a.pyr_stride + g.pix0 + pixel), o4);
        }
    }
}

// Mode 0 (bins <= 5 px wide and <= 5 rows: the three finest levels = 85 % of the output pixels): one lane per pixel.
// VALU-bound, so everything per-row is pared down: the frame base is a scalar, the lane offset 32-bit; rows are
// unrolled to the level's khmax (scalar) and only the last one can be dead; the byte masks of the two possible bin
// widths are picked, not computed.
// ROWS = the level's khmax (3..5), FOUR = bins reach 5 px (a 5th dword per row).  Two pixels per thread per pass: the row
// loads of both are issued before either is consumed -- the kernel is bound by memory latency at 8 waves per SIMD, so
// loads in flight per wave are what counts (specialising on ROWS / FOUR keeps it under 64 VGPRs).
template <int ROWS, bool FOUR>
__device__ __forceinline__ void pyr_level0(const uint8_t* __restrict__ frames, const PyrArgs& a, const PyrLevel& g, const uint32_t* __restrict__ tab,
                                           PyrPx* __restrict__ pyr, int f, int q0, int qstep) {
    constexpr int ND = FOUR ? 5 : 4;                                                 // dwords fetched per row
    const long long fbase = (long long)f * a.H * a.W * 3;
    const long long total = (long long)a.n_frames * a.H * a.W * 3;
    const int fb3 = (int)(fbase & 3);
    const char* fptr = reinterpret_cast<const char*>(frames) + (fbase - fb3);     // dword aligned, scalar
    const int row_bytes = a.W * 3;
    const bool lastf = f == a.n_frames - 1;                                          // other frames may read into their successor
    const unsigned avail = ((unsigned)fb3 + (unsigned)a.H * row_bytes + 3u) & ~3u;  // bytes from fptr to the end of the last dword
    struct Px { unsigned ww[ROWS][ND]; unsigned shv[ROWS]; int kh, kw; bool valid; };
    auto prep = [&](int pixel, Px& p) __attribute__((always_inline)) {
        p.valid = pixel < g.h * g.w;
        p.kh = 1; p.kw = 1;
        if (!p.valid) return;
        int oy = (int)__umulhi((unsigned)pixel, g.wmagic);       // floor(pixel / w) or one above it (large levels): fix up
        oy -= (oy * g.w > pixel) ? 1 : 0;
        const int ox = pixel - oy * g.w;
        int ys, kh, xs, kw;
        if (g.arith) {   // adaptive_avg_pool2d edges [floor(i*in/out), ceil((i+1)*in/out)) without touching memory
            ys = (int)__umulhi((unsigned)(oy * a.H), g.hmagic);
            kh = (int)__umulhi((unsigned)((oy + 1) * a.H + g.h - 1), g.hmagic) - ys;
            xs = (int)__umulhi((unsigned)(ox * a.W), g.wmagic);
            kw = (int)__umulhi((unsigned)((ox + 1) * a.W + g.w - 1), g.wmagic) - xs;
        } else {
            const uint32_t ty = tab[g.ytab0 + oy], tx = tab[g.xtab0 + ox];
            ys = ty & 0xFFFF; kh = (int)(ty >> 16) - ys; xs = tx & 0xFFFF; kw = (int)(tx >> 16) - xs;
        }
        p.kh = kh; p.kw = kw;
        const unsigned lo0 = (unsigned)(ys * row_bytes + xs * 3 + fb3);        // byte offset from fptr of the bin's first byte
        // the aligned 16/20-byte fetch of the LAST row may run past the end of the frame buffer only for the very
        // last pixels of the last frame: those take per-dword clamped loads
        const bool safe = !lastf || (lo0 & ~3u) + (unsigned)((kh - 1) * row_bytes) + 4u * ND <= avail;
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const unsigned lo = lo0 + (unsigned)((r < kh ? r : kh - 1) * row_bytes);
            p.shv[r] = lo & 3u;
            const char* q = fptr + (lo & ~3u);
            if (safe) {
                const u32x4_a4 v4 = *reinterpret_cast<const u32x4_a4*>(q);
                p.ww[r][0] = v4[0]; p.ww[r][1] = v4[1]; p.ww[r][2] = v4[2]; p.ww[r][3] = v4[3];
                if (FOUR) p.ww[r][ND - 1] = *reinterpret_cast<const uint32_t*>(q + 16);
            } else {
                const long long lim = ((total - 1) >> 2) * 4 - (fbase - fb3);   // offset of the last dword holding frame bytes
#pragma unroll
                for (int j = 0; j < ND; j++) {
                    const long long o = (long long)(lo & ~3u) + 4 * j;
                    p.ww[r][j] = *reinterpret_cast<const uint32_t*>(fptr + (o < lim ? o : lim));
                }
            }
        }
    };
    auto finish = [&](int pixel, const Px& p) __attribute__((always_inline)) {
        if (pixel >= g.pix_pad) return;
        float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.valid) {
            const bool wA = p.kw == g.kwA;                                      // a level has two bin widths: pick, don't compute
            const unsigned vm0 = wA ? g.vmA[0] : g.vmB[0], vm1 = wA ? g.vmA[1] : g.vmB[1], vm2 = wA ? g.vmA[2] : g.vmB[2],
                           vm3 = wA ? g.vmA[3] : g.vmB[3];
            unsigned s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
            for (int r = 0; r < ROWS; r++) {
                const bool act = r < p.kh;                                       // only the last unrolled row can be dead
                const unsigned sh = p.shv[r];
                const unsigned d0 = __builtin_amdgcn_alignbyte(p.ww[r][1], p.ww[r][0], sh) & (act ? vm0 : 0u);
                const unsigned d1 = __builtin_amdgcn_alignbyte(p.ww[r][2], p.ww[r][1], sh) & (act ? vm1 : 0u);
                const unsigned d2 = __builtin_amdgcn_alignbyte(FOUR ? p.ww[r][3] : 0u, p.ww[r][2], sh) & (act ? vm2 : 0u);
                s0 = __builtin_amdgcn_udot4(d0, 0x01000001u, s0, false); s1 = __builtin_amdgcn_udot4(d0, 0x00000100u, s1, false);
                s2 = __builtin_amdgcn_udot4(d0, 0x00010000u, s2, false);
                s0 = __builtin_amdgcn_udot4(d1, 0x00010000u, s0, false); s1 = __builtin_amdgcn_udot4(d1, 0x01000001u, s1, false);
                s2 = __builtin_amdgcn_udot4(d1, 0x00000100u, s2, false);
                s0 = __builtin_amdgcn_udot4(d2, 0x00000100u, s0, false); s1 = __builtin_amdgcn_udot4(d2, 0x00010000u, s1, false);
                s2 = __builtin_amdgcn_udot4(d2, 0x01000001u, s2, false);
                if (FOUR) {
                    const unsigned d3 = __builtin_amdgcn_alignbyte(p.ww[r][4], p.ww[r][3], sh) & (act ? vm3 : 0u);
                    s0 = __builtin_amdgcn_udot4(d3, 0x01000001u, s0, false); s1 = __builtin_amdgcn_udot4(d3, 0x00000100u, s1, false);
                    s2 = __builtin_amdgcn_udot4(d3, 0x00010000u, s2, false);
                }
            }
            o4.x = pyr_norm(s0, p.kh, p.kw, g); o4.y = pyr_norm(s1, p.kh, p.kw, g); o4.z = pyr_norm(s2, p.kh, p.kw, g);
        }
        pyr_store(pyr + ((long long)f * a.pyr_stride + g.pix0 + pixel), o4);
    };
    for (int pixel = q0; pixel < g.pix_pad; pixel += 2 * qstep) {
        Px pa, pb;
        prep(pixel, pa);
        prep(pixel + qstep, pb);          // beyond pix_pad: invalid, nothing loaded, nothing stored
        finish(pixel, pa);
        finish(pixel + qstep, pb);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_pyramid(const uint8_t* __restrict__ frames, PyrArgs a, const uint32_t* __restrict__ tab,
                                                 PyrPx* __restrict__ pyr) {
    pyr_level<MODE>(frames, a, a.g, tab, pyr, a.f0 + blockIdx.y, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// mode 0, specialised on the level's row count / dword count (register budget = occupancy = loads in flight)
template <int ROWS, bool FOUR>
__global__ __launch_bounds__(256) void k_pyramid0(const uint8_t* __restrict__ frames, PyrArgs a, const uint32_t* __restrict__ tab,
                                                  PyrPx* __restrict__ pyr) {
    pyr_level0<ROWS, FOUR>(frames, a, a.g, tab, pyr, a.f0 + blockIdx.y, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// The three finest levels in ONE pass over the source.  A workgroup owns a source tile (a band of `band_cols` source
// columns x a strip of `strip_rows` source rows); wave L walks the tile's source rows for level L: its 64 lanes are the output
// columns of that level whose bins START in the band, its output rows those whose bins start in the strip (a bin may run past the
// tile: the wave simply reads on).  The three waves read the same source rows at about the same time, so the frame bytes come from
// HBM once and from the CU's L1 / the L2 for the other two levels -- the per-level kernels above re-read the whole frame chunk
// from the Infinity Cache for every level.  Inside a wave: a source row's three channel sums are formed once and added to the (at
// most two: H >= h) bins that contain it, column quantities are per-lane constants, row quantities wave-uniform (SALU); integer
// sums, the same division and normalisation (pyr_norm): bit-identical pixels.  D source rows in flight per lane.
struct PyrFineArgs {
    int H, W, n_frames; long long pyr_stride;
    int nlev, band_cols, strip_rows, n_bands, n_strips;
    int own0;                      // offset in `tab` of the ownership table: [level][band] (ox_lo, ox_hi), then [level][strip] (oy_lo, oy_hi)
    PyrLevel g[3];
};
template <bool FOUR>
__device__ __forceinline__ void pyr_fine_wave(const uint8_t* __restrict__ frames, const PyrFineArgs& a, const PyrLevel& g, const uint32_t* __restrict__ tab,
                                              PyrPx* __restrict__ pyr, int f, int ox_lo, int ox_hi, int oy0, int oy1, int lane, bool pad_wave) {
    constexpr int ND = FOUR ? 5 : 4, D = 6;                                          // (4 and 8 rows in flight measured the same)
    PyrPx* const out = pyr + ((long long)f * a.pyr_stride + g.pix0);
    if (pad_wave && g.h * g.w + lane < g.pix_pad) pyr_store(out + (g.h * g.w + lane), make_float4(0.f, 0.f, 0.f, 0.f));   // the level's padding pixels: zeros, as ever
    if (oy0 >= oy1 || ox_lo >= ox_hi) return;                                        // wave-uniform
    const int ox = ox_lo + lane;
    const bool valid = ox < ox_hi;
    // ---- column quantities: constants of the lane for the whole strip ----
    const uint32_t tx = tab[g.xtab0 + (valid ? ox : ox_hi - 1)];
    const int xs = tx & 0xFFFF, kw = (int)(tx >> 16) - xs;
    const long long fbase = (long long)f * a.H * a.W * 3;
    const int fb3 = (int)(fbase & 3);
    const char* fptr = reinterpret_cast<const char*>(frames) + (fbase - fb3);      // dword aligned, scalar
    const unsigned row_bytes = (unsigned)a.W * 3u;
    const unsigned lx = (unsigned)(xs * 3 + fb3);                                   // the bin's first byte inside a source row, from fptr
    const bool wA = kw == g.kwA;
    const unsigned vm0 = wA ? g.vmA[0] : g.vmB[0], vm1 = wA ? g.vmA[1] : g.vmB[1], vm2 = wA ? g.vmA[2] : g.vmB[2], vm3 = wA ? g.vmA[3] : g.vmB[3];
    const bool lastf = f == a.n_frames - 1;
    const long long lim = ((((long long)a.n_frames * a.H * a.W * 3) - 1) >> 2) * 4 - (fbase - fb3);   // last dword holding frame bytes, from fptr
    // a source row: ND aligned dwords from the bin's first byte.  SLOW = a strip that reads the last row of the last frame, which
    // may not be read past the end of the buffer: clamped dwords (the pipelined loop stays single-path)
    auto fetch = [&](auto SLOW_T, int y, unsigned (&w)[ND]) __attribute__((always_inline)) {
        const unsigned lo = (unsigned)y * row_bytes + lx;
        const char* q = fptr + (lo & ~3u);
        if (!decltype(SLOW_T)::value) {
            const u32x4_a4 v4 = *reinterpret_cast<const u32x4_a4*>(q);
            w[0] = v4[0]; w[1] = v4[1]; w[2] = v4[2]; w[3] = v4[3];
            if (FOUR) w[ND - 1] = *reinterpret_cast<const uint32_t*>(q + 16);
        } else {
#pragma unroll
            for (int j = 0; j < ND; j++) {
                const long long o = (long long)(lo & ~3u) + 4 * j;
                w[j] = *reinterpret_cast<const uint32_t*>(fptr + (o < lim ? o : lim));
            }
        }
    };
    auto rowsum = [&](int y, const unsigned (&w)[ND], unsigned& r0, unsigned& r1, unsigned& r2) __attribute__((always_inline)) {
        const unsigned sh = ((unsigned)y * row_bytes + lx) & 3u;
        const unsigned d0 = __builtin_amdgcn_alignbyte(w[1], w[0], sh) & vm0;
        const unsigned d1 = __builtin_amdgcn_alignbyte(w[2], w[1], sh) & vm1;
        const unsigned d2 = __builtin_amdgcn_alignbyte(w[3], w[2], sh) & vm2;
        r0 = __builtin_amdgcn_udot4(d0, 0x01000001u, 0u, false); r1 = __builtin_amdgcn_udot4(d0, 0x00000100u, 0u, false);
        r2 = __builtin_amdgcn_udot4(d0, 0x00010000u, 0u, false);
        r0 = __builtin_amdgcn_udot4(d1, 0x00010000u, r0, false); r1 = __builtin_amdgcn_udot4(d1, 0x01000001u, r1, false);
        r2 = __builtin_amdgcn_udot4(d1, 0x00000100u, r2, false);
        r0 = __builtin_amdgcn_udot4(d2, 0x00000100u, r0, false); r1 = __builtin_amdgcn_udot4(d2, 0x00010000u, r1, false);
        r2 = __builtin_amdgcn_udot4(d2, 0x01000001u, r2, false);
        if (FOUR) {
            const unsigned d3 = __builtin_amdgcn_alignbyte(w[4], w[3], sh) & vm3;
            r0 = __builtin_amdgcn_udot4(d3, 0x01000001u, r0, false); r1 = __builtin_amdgcn_udot4(d3, 0x00000100u, r1, false);
            r2 = __builtin_amdgcn_udot4(d3, 0x00010000u, r2, false);
        }
    };
    // ---- row quantities: wave-uniform ----
    auto edges = [&](int oy, int& ys, int& ye) __attribute__((always_inline)) {     // bin [ys, ye) of output row oy; past the strip: never
        if (oy >= oy1) { ys = 0x7fffffff; ye = 0x7fffffff; return; }
        if (g.arith) {
            ys = (int)__umulhi((unsigned)(oy * a.H), g.hmagic);
            ye = (int)__umulhi((unsigned)((oy + 1) * a.H + g.h - 1), g.hmagic);
        } else {
            const uint32_t t = tab[g.ytab0 + oy];
            ys = (int)(t & 0xFFFF); ye = (int)(t >> 16);
        }
        ys = __builtin_amdgcn_readfirstlane(ys); ye = __builtin_amdgcn_readfirstlane(ye);
    };
    int ys_first, ye_first, ys_last, yend;
    edges(oy0, ys_first, ye_first);
    edges(oy1 - 1, ys_last, yend);                                                   // the wave's source rows: [ys_first, yend)
    auto run = [&](auto SLOW_T) __attribute__((always_inline)) {
        int oy = oy0, ys_c = ys_first, ye_c = ye_first, ys_n, ye_n;
        edges(oy + 1, ys_n, ye_n);
        unsigned c0 = 0, c1 = 0, c2 = 0, n0 = 0, n1 = 0, n2 = 0;                    // channel sums of the current bin and of the next one
        unsigned ring[D][ND];
        const int ycl = yend - 1;                                                    // rows past the wave's last bin are never touched
#pragma unroll
        for (int k = 0; k < D; k++) fetch(SLOW_T, ys_first + k < ycl ? ys_first + k : ycl, ring[k]);
        for (int yb = ys_first; yb < yend; yb += D) {
#pragma unroll
            for (int k = 0; k < D; k++) {
                const int y = yb + k;                                                // wave-uniform
                unsigned r0, r1, r2;
                rowsum(y, ring[k], r0, r1, r2);                                      // (rows at and past yend: a re-read row, sums unused)
                fetch(SLOW_T, y + D < ycl ? y + D : ycl, ring[k]);
                if (y < yend) {
                    c0 += r0; c1 += r1; c2 += r2;
                    if (y >= ys_n) { n0 += r0; n1 += r1; n2 += r2; }
                    if (y + 1 == ye_c) {                                           // the current bin is complete
                        if (valid) {
                            const int kh = ye_c - ys_c;
                            float4 o4;
                            o4.x = pyr_norm(c0, kh, kw, g); o4.y = pyr_norm(c1, kh, kw, g); o4.z = pyr_norm(c2, kh, kw, g); o4.w = 0.f;
                            pyr_store(out + (oy * g.w + ox), o4);
                        }
                        c0 = n0; c1 = n1; c2 = n2; n0 = 0; n1 = 0; n2 = 0;
                        oy++;
                        ys_c = ys_n; ye_c = ye_n;
                        edges(oy + 1, ys_n, ye_n);
                    }
                }
            }
        }
    };
    if (lastf && yend >= a.H) run(std::true_type{}); else run(std::false_type{});
}

__global__ __launch_bounds__(192) void k_pyramid_fine(const uint8_t* __restrict__ frames, PyrFineArgs a, const uint32_t* __restrict__ tab,
                                                      PyrPx* __restrict__ pyr) {
    const int lane = threadIdx.x & 63, lvl = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (lvl >= a.nlev) return;
    const int band = blockIdx.x, strip = blockIdx.z, f = blockIdx.y;
    const uint32_t* own = tab + a.own0;
    const uint32_t cb = own[lvl * a.n_bands + band], rb = own[3 * a.n_bands + lvl * a.n_strips + strip];
    const int ox_lo = __builtin_amdgcn_readfirstlane((int)(cb & 0xFFFF)), ox_hi = __builtin_amdgcn_readfirstlane((int)(cb >> 16));
    const int oy_lo = __builtin_amdgcn_readfirstlane((int)(rb & 0xFFFF)), oy_hi = __builtin_amdgcn_readfirstlane((int)(rb >> 16));
    const bool pad_wave = band == 0 && strip == 0;
    if (lvl == 0) { if (a.g[0].kwmax * 3 + 3 > 16) pyr_fine_wave<true>(frames, a, a.g[0], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); else pyr_fine_wave<false>(frames, a, a.g[0], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); }
    else if (lvl == 1) { if (a.g[1].kwmax * 3 + 3 > 16) pyr_fine_wave<true>(frames, a, a.g[1], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); else pyr_fine_wave<false>(frames, a, a.g[1], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); }
    else { if (a.g[2].kwmax * 3 + 3 > 16) pyr_fine_wave<true>(frames, a, a.g[2], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); else pyr_fine_wave<false>(frames, a, a.g[2], tab, pyr, f, ox_lo, ox_hi, oy_lo, oy_hi, lane, pad_wave); }
}

// ---- coarse levels in ONE streaming pass ------------------------------------------------------------------
// The per-level kernels above make every level re-read its whole source chunk; for the coarse levels (bins wider than
// 5 px: 8 of the 11 levels at 720p, 15 % of the pixels) that re-read IS the cost (~55 us per level and 64 frames,
// whatever the level's size).  The streaming pass reads each source row ONCE for all of them:
//   * an owner -- a workgroup or a wave, see OwnBlock / OwnWave -- takes a unit of the frame (rows [R0,R1) x a segment of columns) and
//     walks its rows top down; a lane holds 16 or 20 consecutive bytes of the row (one dword-aligned 16-byte load + 1 or 2 dwords,
//     re-aligned by a scalar shift);
//   * it keeps ONE running sum P of the rows walked so far (packed 16-bit, one field per byte column, updated once per row whatever
//     the number of levels) and, per level, the snapshot S_l = P before the current bin's first row (without that row when the bin
//     starts on the row that ends its predecessor).  At the bin's last row its column sums are P - S_l per field.  The fields wrap
//     (a band of 290 rows of 255s overflows 16 bits) and the difference is still exact, because a streamed bin's column sum is below
//     2^16: launch_coarse refuses khmax > 256 -- the limit that test_packed_column_sums_at_the_256_row_limit pins now bounds the
//     wrapped running sum as well;
//   * the column sums go to an LDS strip of 16-bit words; 2^gs lanes share an output pixel, each issues the reads of four of the
//     bin's columns before its first add, and the group is summed with DPP adds; normalised (pyr_norm) and stored.  The block-wide
//     pass alternates two strips, so one barrier per flush suffices;
//   * the per-level state lives in lanes (lane L = level L), not in scalar registers: a row costs two vector compares whatever
//     the number of levels, and the flush is written once per row slot (3 k instructions instead of 25 k);
//   * a unit computes the bins that START inside it and reads on past its end until they are complete (no atomics).
// Integer sums in any order are exact, so the result is bit-identical to the per-level kernels (tests: every level, 180p..4K).
constexpr int SMAXL = 12;               // coarse levels per launch
constexpr int SBYTES = 4096;            // bytes of a source row a workgroup covers (256 threads x 16)
constexpr int SW_BYTES = 1280;          // bytes of a source row a wave covers (64 lanes x 20)
constexpr int STAB = 6144;              // most bin-edge words of a launch's levels (rows + columns) kept in LDS; a launch allocates its own
struct PyrStreamArgs {
    int H, W, n_frames, nlev, rows_per_band, cols_per_band, row_bands, col_bands;
    int tab0, tab_words;                // the span of the device table that holds the launch's levels
    long long pyr_stride;
    PyrBins lv[SMAXL];
};

// Who owns a unit of the pass (a band of rows x a segment of BYTES source bytes per row) and the STRIPS LDS strips its bin rows are
// flushed through.  A lane holds DW dwords of the row (+ 1 for the re-alignment); a workgroup holds UNITS units.
//   OwnBlock  the workgroup: one unit covers the whole row of a frame up to 1,365 px wide; a block barrier between a flush's strip
//             writes and its reads, and two strips in turn instead of a second one.
//   OwnWave   one wave, which never talks to another (frames wider than one 4096-byte band: 1080p, 4K).  The segment is 64 x 20 =
//             1280 bytes = 426 pixels of which the last kwmax overlap the next segment, so that every bin that STARTS in the segment
//             is covered by the wave's own loads; LDS operations of one wave execute in order: no barrier, one strip.  (At 720p,
//             where both apply, the block-wide pass was the faster one when both were last compared -- 0.63 vs 1.11 ms: every wave
//             pays all ~165 flush round trips alone -- so it keeps the narrow frames.)
struct OwnBlock {
    static constexpr int LANES = 256, DW = 4, UNITS = 1, BYTES = SBYTES, STRIPS = 2;
    static __device__ __forceinline__ int lane() { return threadIdx.x; }
    static __device__ __forceinline__ int slot() { return 0; }                   // unit of the workgroup
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};
struct OwnWave {
    static constexpr int LANES = 64, DW = 5, UNITS = 4, BYTES = SW_BYTES, STRIPS = 1;
    static __device__ __forceinline__ int lane() { return threadIdx.x & 63; }
    static __device__ __forceinline__ int slot() { return __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); }
    static __device__ __forceinline__ void sync() { __builtin_amdgcn_wave_barrier(); }
};

extern __shared__ uint4 stream_lds[];
template <class Own> constexpr int stream_strip_words() { return Own::UNITS * Own::STRIPS * Own::BYTES; }   // 16-bit words
// sums of 2, 4, 8 and 16 neighbouring lanes: s + the value of the lane a DPP pattern names
template <int CTRL> __device__ __forceinline__ unsigned dpp_add(unsigned s) {
    return s + (unsigned)__builtin_amdgcn_update_dpp(0, (int)s, CTRL, 0xF, 0xF, false);
}

template <int NL, class Own>
__global__ __launch_bounds__(256) void k_pyramid_stream(const uint8_t* __restrict__ frames, PyrStreamArgs a, const uint32_t* __restrict__ gtab,
                                                        PyrPx* __restrict__ pyr) {
    constexpr int DW = Own::DW, LANES = Own::LANES;
    static_assert(Own::BYTES == 4 * DW * LANES && Own::UNITS * LANES == 256, "a lane's dwords tile the segment, the units the workgroup");
    // dynamic LDS: per unit STRIPS strips of one 16-bit word per byte column of its segment, then the levels' edge tables, re-based
    // (a level's rows at its ty0, its columns at its tx0): as many words as the launch's levels have rows and columns
    unsigned short* const strips = reinterpret_cast<unsigned short*>(stream_lds);
    uint32_t* const tab = reinterpret_cast<uint32_t*>(strips + stream_strip_words<Own>());
    const int tid = threadIdx.x, lane = Own::lane(), slot = Own::slot();
    const int f = blockIdx.y;
    const int row_bytes = a.W * 3;
    const long long fbase = (long long)f * a.H * row_bytes;
    const long long last_dw = ((long long)a.n_frames * a.H * row_bytes - 1) >> 2;
    const uint32_t* base32 = reinterpret_cast<const uint32_t*>(frames);
    // edge tables of the handled levels -> LDS (a flush would otherwise end in a dependent global load): one flat copy of the span
    // that holds them, every load in flight at once
    for (int i = tid; i < a.tab_words; i += 256) tab[i] = gtab[a.tab0 + i];
    __syncthreads();                                     // (OwnWave: the only block barrier, from here on the waves are on their own)
    const int unit = blockIdx.x * Own::UNITS + slot;     // (row band, column segment)
    if (Own::UNITS > 1 && unit >= a.row_bands * a.col_bands) return;
    const int rb = unit / a.col_bands, cb = unit - rb * a.col_bands;
    const int R0 = rb * a.rows_per_band, R1 = (R0 + a.rows_per_band < a.H) ? R0 + a.rows_per_band : a.H;
    const int C0 = cb * a.cols_per_band, C1 = (C0 + a.cols_per_band < a.W) ? C0 + a.cols_per_band : a.W;
    unsigned short* const colbuf = strips + slot * Own::STRIPS * Own::BYTES;
    int flip = 0;                                        // OwnBlock: the strip the next flush goes through

    // Level state lives in LANES: lane L of every wave holds the quantities of level L (all waves of a workgroup the same values), so
    // that a row costs two vector compares, not two scalar tests per level, and the flush below exists once per row slot, for a level
    // index read from the compare's mask.  Per level: owned output rows [j, jend), owned output columns [ox0, ox1), current bin rows
    // [ys, ye), gs = log2 of the lanes that share one output pixel of a flush, table offsets, and what normalising needs (as VALUES: a
    // per-lane choice between two members of the argument block compiles to a choice of address and a global load per channel).
    const int L = threadIdx.x & 63;
    const bool has = L < a.nlev;
    const PyrBins& gl = a.lv[has ? L : 0];
    const int v_ty0 = gl.ytab0 - a.tab0, v_tx0 = gl.xtab0 - a.tab0, v_w = gl.w, v_pix0 = gl.pix0, v_khA = gl.khA, v_kwA = gl.kwA,
              v_fast = gl.fastdiv;
    const float v_rkh0 = gl.rkh[0], v_rkh1 = gl.rkh[1], v_rkw0 = gl.rkw[0], v_rkw1 = gl.rkw[1];
    int v_j = 0, v_jend = 0, v_ys = 0x7fffffff, v_ye = 0x7fffffff, v_ox0 = 0, v_ox1 = 0, v_gs = 0, v_e1 = R0;
    if (has) {
        auto first_at_or_after = [&](int tab0, int n_out, int n_in, int pos) {   // first bin whose start >= pos
            if (pos >= n_in) return n_out;
            int q = (int)(((long long)pos * n_out + n_in - 1) / n_in);
            if (q > n_out) q = n_out;
            while (q > 0 && (int)(tab[tab0 + q - 1] & 0xFFFF) >= pos) q--;
            while (q < n_out && (int)(tab[tab0 + q] & 0xFFFF) < pos) q++;
            return q;
        };
        v_j = first_at_or_after(v_ty0, gl.h, a.H, R0);
        v_jend = first_at_or_after(v_ty0, gl.h, a.H, R1);
        v_ox0 = first_at_or_after(v_tx0, gl.w, a.W, C0);
        v_ox1 = first_at_or_after(v_tx0, gl.w, a.W, C1);
        while (v_gs < 4 && ((v_ox1 - v_ox0) << (v_gs + 1)) <= LANES && (2 << v_gs) <= gl.kwA) v_gs++;   // within a DPP row
        if (v_j < v_jend && v_ox0 < v_ox1) {
            const uint32_t t0 = tab[v_ty0 + v_j], t1 = tab[v_ty0 + v_jend - 1];
            v_ys = (int)(t0 & 0xFFFF); v_ye = (int)(t0 >> 16);
            v_e1 = (int)(t1 >> 16);
        } else {
            v_j = v_jend;
        }
    }
    auto rl = [](int v, int l) { return __builtin_amdgcn_readlane(v, l); };
    auto rlf = [](float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
    int yend = R0;
    for (int l = 0; l < a.nlev; l++) { const int e1 = rl(v_e1, l); yend = e1 > yend ? e1 : yend; }
    if (unit == 0) {                                     // zero the 64-pixel padding behind each level once per frame
        for (int l = 0; l < a.nlev; l++) {
            const PyrBins& g = a.lv[l];
            for (int p = g.h * g.w + lane; p < g.pix_pad; p += LANES)
                pyr_store(pyr + ((long long)f * a.pyr_stride + g.pix0 + p), make_float4(0.f, 0.f, 0.f, 0.f));
        }
    }
    if (yend <= R0) return;

    // packed 16-bit column sums, bytes 0,2 / 1,3 of each of the lane's DW dwords: the running sum of every row walked so far and, per
    // level, its value before the current bin's first row (fields wrap on their own: v_pk_add_u16 / v_pk_sub_u16)
    u16x2 pe[DW], po[DW], se[NL][DW], so[NL][DW];
#pragma unroll
    for (int d = 0; d < DW; d++) { pe[d] = 0; po[d] = 0; }
#pragma unroll
    for (int l = 0; l < NL; l++)
#pragma unroll
        for (int d = 0; d < DW; d++) { se[l][d] = 0; so[l][d] = 0; }

    // one source row: this lane's 4*DW bytes at byte offset C0*3 + 4*DW*lane of row y (+ the dword behind them for the re-alignment)
    // The SAME memory instructions for every lane and row, issued unconditionally: the compiler counts the loads in flight behind
    // the row it waits for only when every path issues the same number (a conditional or two-shaped load made it wait for all but
    // the newest row).  A lane whose window would end past the frame buffer moves it back to end there and shifts the dwords up
    // again when the row is consumed (rows at the very end of the last frame: `tail`).
    const long long lim_dw = last_dw - DW > 0 ? last_dw - DW : 0;
    auto load_row = [&](int y, unsigned (&w)[DW + 1], unsigned& sh) {
        const int yy = y < a.H ? y : a.H - 1;                                    // rows past the frame are never accumulated
        const long long o = fbase + (long long)yy * row_bytes + (long long)C0 * 3;   // scalar
        sh = (unsigned)(o & 3);
        long long dw = (o >> 2) + DW * lane;
        dw = dw < lim_dw ? dw : lim_dw;
        const u32x4_a4 v4 = *reinterpret_cast<const u32x4_a4*>(base32 + dw);
        w[0] = v4[0]; w[1] = v4[1]; w[2] = v4[2]; w[3] = v4[3];
#pragma unroll
        for (int k = 4; k <= DW; k++) w[k] = base32[dw + k];
    };
    auto fix_tail = [&](int y, unsigned (&w)[DW + 1]) {
        const int yy = y < a.H ? y : a.H - 1;
        const long long dw0 = (fbase + (long long)yy * row_bytes + (long long)C0 * 3) >> 2;   // scalar
        if (dw0 + DW * (LANES - 1) <= lim_dw) return;                                        // uniform: no lane moved its window
        const long long over = dw0 + DW * lane - lim_dw;                        // dwords the window was moved back by
#pragma unroll
        for (int m = 1; m <= DW; m++)
            if (over == m) {
#pragma unroll
                for (int k = 0; k + m <= DW; k++) w[k] = w[k + m];              // (what lies past the buffer is past the frame: unused)
            }
    };
    // the row's bytes 0,2 / 1,3 of each dword, re-aligned to the segment's first byte
    auto unpack = [&](int y, unsigned (&w)[DW + 1], unsigned sh, u16x2 (&re)[DW], u16x2 (&ro)[DW]) {
        fix_tail(y, w);
#pragma unroll
        for (int d = 0; d < DW; d++) {
            const unsigned v = __builtin_amdgcn_alignbyte(w[d + 1], w[d], sh);
            re[d] = __builtin_bit_cast(u16x2, v & 0x00FF00FFu); ro[d] = __builtin_bit_cast(u16x2, (v >> 8) & 0x00FF00FFu);
        }
    };
    auto consume = [&](int y, const u16x2 (&re)[DW], const u16x2 (&ro)[DW]) {
        const unsigned starts = (unsigned)__builtin_amdgcn_ballot_w64(v_ys == y);     // levels with a bin that starts on this row
        const unsigned ends = (unsigned)__builtin_amdgcn_ballot_w64(v_ye == y + 1);   // ... that ends on it
        if (starts) {
#pragma unroll
            for (int l = 0; l < NL; l++)
                if (starts >> l & 1) {
#pragma unroll
                    for (int d = 0; d < DW; d++) { se[l][d] = pe[d]; so[l][d] = po[d]; }
                }
        }
#pragma unroll
        for (int d = 0; d < DW; d++) { pe[d] += re[d]; po[d] += ro[d]; }
        for (unsigned m = ends; m; m &= m - 1) {
            // ---- a bin row of level l is complete: column sums -> the unit's LDS strip -> horizontal bins -> normalise -> store ----
            const int l = __builtin_ctz(m);
            u16x2 ce[DW], co[DW];
#pragma unroll
            for (int k = 0; k < NL; k++)
                if (l == k) {
#pragma unroll
                    for (int d = 0; d < DW; d++) { ce[d] = pe[d] - se[k][d]; co[d] = po[d] - so[k][d]; }
                }
            const int jl = rl(v_j, l), kh = rl(v_ye, l) - rl(v_ys, l), ox0 = rl(v_ox0, l), ox1 = rl(v_ox1, l), gsh = rl(v_gs, l);
            const int ty0 = rl(v_ty0, l), tx0 = rl(v_tx0, l), kwA = rl(v_kwA, l);
            const float fkh = (float)kh, rh = kh == rl(v_khA, l) ? rlf(v_rkh0, l) : rlf(v_rkh1, l), rw0 = rlf(v_rkw0, l), rw1 = rlf(v_rkw1, l);
            const bool fast = rl(v_fast, l) != 0;
            PyrPx* const orow = pyr + ((long long)f * a.pyr_stride + rl(v_pix0, l) + (long long)jl * rl(v_w, l));
            unsigned short* const strip = colbuf + flip * Own::BYTES;
            uint2* const dst = reinterpret_cast<uint2*>(strip + 4 * DW * lane);
#pragma unroll
            for (int d = 0; d < DW; d++) dst[d] = make_uint2(ce[d].x | ((unsigned)co[d].x << 16), ce[d].y | ((unsigned)co[d].y << 16));
            Own::sync();
            // 2^gs lanes per output pixel, each takes every 2^gs-th column of the bin: the reads of four columns are issued
            // before the first add, the group is summed across lanes (DPP)
            const int nth = (ox1 - ox0) << gsh;
            for (int t = lane; t < nth; t += LANES) {
                const int ox = ox0 + (t >> gsh), sub = t & ((1 << gsh) - 1);
                const uint32_t tx = tab[tx0 + ox];
                const int xs = tx & 0xFFFF, xe = tx >> 16;
                unsigned s0 = 0, s1 = 0, s2 = 0;
                for (int x0 = xs + sub; x0 < xe; x0 += 4 << gsh) {
                    unsigned q[4][3];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int xx = x0 + (k << gsh);
                        const unsigned short* p = strip + ((xx < xe ? xx : x0) - C0) * 3;
                        q[k][0] = p[0]; q[k][1] = p[1]; q[k][2] = p[2];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const bool in = x0 + (k << gsh) < xe;
                        s0 += in ? q[k][0] : 0u; s1 += in ? q[k][1] : 0u; s2 += in ? q[k][2] : 0u;
                    }
                }
                if (gsh > 0) { s0 = dpp_add<0xB1>(s0); s1 = dpp_add<0xB1>(s1); s2 = dpp_add<0xB1>(s2); }      // lane ^ 1
                if (gsh > 1) { s0 = dpp_add<0x4E>(s0); s1 = dpp_add<0x4E>(s1); s2 = dpp_add<0x4E>(s2); }      // lane ^ 2
                if (gsh > 2) { s0 = dpp_add<0x141>(s0); s1 = dpp_add<0x141>(s1); s2 = dpp_add<0x141>(s2); }   // the other quad
                if (gsh > 3) { s0 = dpp_add<0x140>(s0); s1 = dpp_add<0x140>(s1); s2 = dpp_add<0x140>(s2); }   // the other eight
                if (sub == 0) {
                    const float fkw = (float)(xe - xs), rw = xe - xs == kwA ? rw0 : rw1;
                    float4 o4;
                    o4.x = pyr_norm(s0, fkh, fkw, rh, rw, fast); o4.y = pyr_norm(s1, fkh, fkw, rh, rw, fast);
                    o4.z = pyr_norm(s2, fkh, fkw, rh, rw, fast); o4.w = 0.f;
                    pyr_store(orow + ox, o4);
                }
            }
            // OwnBlock: the next flush writes the other strip, and the one after it comes behind that flush's barrier, which
            // every wave reaches with these reads done: one barrier per flush
            if (Own::STRIPS > 1) flip ^= 1; else Own::sync();
            // next owned bin of this level; consecutive bins may share this source row
            int nys = 0x7fffffff, nye = 0x7fffffff;
            if (jl + 1 < rl(v_jend, l)) {
                const uint32_t t0 = tab[ty0 + jl + 1];
                nys = __builtin_amdgcn_readfirstlane((int)(t0 & 0xFFFF)); nye = __builtin_amdgcn_readfirstlane((int)(t0 >> 16));
            }
            if (L == l) { v_j = jl + 1; v_ys = nys; v_ye = nye; }
            if (nys <= y) {                                                      // it starts on this row: the sum without it
#pragma unroll
                for (int k = 0; k < NL; k++)
                    if (l == k) {
#pragma unroll
                        for (int d = 0; d < DW; d++) { se[k][d] = pe[d] - re[d]; so[k][d] = po[d] - ro[d]; }
                    }
            }
        }
    };

    // rows in groups of PF: the loads of the next group are issued, all of them, before this group is consumed, and move into this
    // group's registers behind it -- the only place that waits for them.  (Reloading a row's registers as soon as the row was consumed
    // looked tighter, but the compiler rotated the registers with moves at the loop's end that waited for every load in flight.)
    // Groups of 2 measured like 3 and 4 with the same waves per SIMD and cost 10 VGPRs less per row; 1 is slower (0.46 vs 0.42 ms).
    constexpr int PF = 2;
    unsigned wb[PF][DW + 1], shb[PF], wn[PF][DW + 1], shn[PF];
#pragma unroll
    for (int u = 0; u < PF; u++) load_row(R0 + u, wb[u], shb[u]);
    for (int y = R0; y < yend; y += PF) {
#pragma unroll
        for (int u = 0; u < PF; u++) load_row(y + PF + u, wn[u], shn[u]);   // (past the unit's end: a row of the frame, unused)
#pragma unroll
        for (int u = 0; u < PF; u++) {
            u16x2 re[DW], ro[DW];
            unpack(y + u, wb[u], shb[u], re, ro);
            if (y + u < yend) consume(y + u, re, ro);
        }
#pragma unroll
        for (int u = 0; u < PF; u++) {
#pragma unroll
            for (int k = 0; k <= DW; k++) wb[u][k] = wn[u][k];
            shb[u] = shn[u];
        }
    }
}

}  // namespace

// Levels of an H x W frame: where each lies in a frame's pyramid, its bin geometry and the per-level kernel it would take.
int trl_pyramid_layout(trl_ctx* c, int H, int W, PyrLayout& lay) {
    const int L = trl_compute_levels(c, H, W);
    if (L > 16) { trl_set_error("more than 16 pyramid levels"); return TRL_ERR_INVALID; }
    if (L < 1) { trl_set_error("frame %dx%d has no pyramid level at min_face_size %d", W, H, c->cfg.min_face_size); return TRL_ERR_INVALID; }
    lay.L = L;
    int ntab = 0; long long pix = 0;
    for (int l = 0; l < L; l++) {
        const LevelGeom& g = c->lv[l];
        PyrLevel& p = lay.lv[l];
        p.h = g.h; p.w = g.w;
        p.pix0 = (int)pix;
        p.pix_pad = (int)(((long long)g.h * g.w + 63) & ~63ll);
        pix += p.pix_pad;
        // pyramid kernel path and lanes per output pixel
        const int khmax = (H + g.h - 1) / g.h + 1, kwmax = (W + g.w - 1) / g.w + 1;   // upper bounds of the bin sizes
        p.khA = (H + g.h - 1) / g.h; p.kwA = (W + g.w - 1) / g.w;
        p.khmax = (H % g.h) ? p.khA + 1 : p.khA; p.kwmax = (W % g.w) ? p.kwA + 1 : p.kwA;
        p.rkh[0] = 1.0f / (float)p.khA; p.rkh[1] = 1.0f / (float)(p.khA + 1);
        p.rkw[0] = 1.0f / (float)p.kwA; p.rkw[1] = 1.0f / (float)(p.kwA + 1);
        p.fastdiv = (p.khA + 1 <= 96 && p.kwA + 1 <= 96) ? 1 : 0;
        for (int d = 0; d < 4; d++) {
            auto vb = [](int rel, int nbytes) { int hi = nbytes - rel; hi = hi < 0 ? 0 : (hi > 4 ? 4 : hi); return hi >= 4 ? 0xFFFFFFFFu : ((1u << (8 * hi)) - 1u); };
            p.vmA[d] = vb(4 * d, 3 * p.kwA); p.vmB[d] = vb(4 * d, 3 * (p.kwA + 1));
        }
        p.wmagic = (unsigned)((0x100000000ull + g.w - 1) / g.w);
        p.hmagic = (unsigned)((0x100000000ull + g.h - 1) / g.h);
        // floor(n / d) == umulhi(n, ceil(2^32 / d)) for every n with n * d < 2^32 (n <= (in + 1) * out here)
        p.arith = ((unsigned long long)(H + 1) * g.h * g.h < 0x100000000ull && (unsigned long long)(W + 1) * g.w * g.w < 0x100000000ull &&
                   g.h > 1 && g.w > 1) ? 1 : 0;
        p.nd = 3; p.grshift = 0;
        if (kwmax * 3 <= 15 && khmax <= 5) {
            p.mode = 0; p.gshift = 0; p.nd = kwmax * 3 <= 9 ? 3 : 4;
        } else if ((W * 3) % 4 == 0) {
            p.mode = 1;
            const int ngr = (kwmax * 3 + 3 + 11) / 12;
            while ((1 << p.grshift) < ngr) p.grshift++;
            int rlsh = 0;
            while ((khmax >> rlsh) > 8 && p.grshift + rlsh < 6) rlsh++;
            p.gshift = p.grshift + rlsh;
            if (p.gshift > 6) { p.mode = 2; p.gshift = 6; }
        } else {
            p.mode = 2;
            const int dwords = khmax * ((kwmax * 3 + 6) / 4);
            p.gshift = dwords <= 40 ? 0 : (dwords <= 160 ? 2 : (dwords <= 640 ? 4 : 6));
        }
        p.ytab0 = ntab; ntab += g.h;
        p.xtab0 = ntab; ntab += g.w;
    }
    lay.pyr_stride = pix;
    return TRL_OK;
}

// k_pyramid_fine: which output columns / rows of the (up to three) finest levels belong to which source tile -- those whose bins
// START in it.  A band must not own more than 64 columns of any level (one wave = one level's columns of the band): the widest band
// that keeps to it is searched, its tables appended to `tab`, the choice left in c->pyr_fine (nlev == 0: no fine pass for this shape).
static void pyr_fine_ownership(trl_ctx* c, int H, int W, const PyrLayout& lay, std::vector<uint32_t>& tab) {
    c->pyr_fine.nlev = 0;
    int nfine = 0;
    while (nfine < 3 && nfine < lay.L && lay.lv[nfine].mode == 0 && lay.lv[nfine].h <= H && lay.lv[nfine].w <= W) nfine++;
    if (nfine < 2) return;
    const int strip_rows = 24;                                            // source rows per tile
    std::vector<uint32_t> own;
    for (int band_cols = (int)(62.0 * W / lay.lv[0].w); band_cols >= 16; band_cols--) {
        const int nb = (W + band_cols - 1) / band_cols, ns = (H + strip_rows - 1) / strip_rows;
        own.assign((size_t)3 * nb + (size_t)3 * ns, 0u);
        bool ok = true;
        for (int l = 0; l < nfine && ok; l++) {
            const PyrLevel& g = lay.lv[l];
            int o = 0;
            for (int b = 0; b < nb; b++) {                   // columns: bin starts are non-decreasing in ox
                const int lo = o;
                while (o < g.w && (int)(tab[g.xtab0 + o] & 0xFFFF) < (b + 1) * band_cols) o++;
                if (o - lo > 64) { ok = false; break; }
                own[(size_t)l * nb + b] = (uint32_t)lo | ((uint32_t)o << 16);
            }
            o = 0;
            for (int t = 0; t < ns; t++) {
                const int lo = o;
                while (o < g.h && (int)(tab[g.ytab0 + o] & 0xFFFF) < (t + 1) * strip_rows) o++;
                own[(size_t)3 * nb + (size_t)l * ns + t] = (uint32_t)lo | ((uint32_t)o << 16);
            }
        }
        if (!ok) continue;
        c->pyr_fine.nlev = nfine; c->pyr_fine.own0 = (int)tab.size(); c->pyr_fine.band_cols = band_cols; c->pyr_fine.strip_rows = strip_rows;
        c->pyr_fine.n_bands = nb; c->pyr_fine.n_strips = ns;
        tab.insert(tab.end(), own.begin(), own.end());
        return;
    }
}

// The device tables of a frame shape: the bin edges of every level, one packed (start | end << 16) word per output row / column
// (adaptive_avg_pool2d: [floor(i*in/out), ceil((i+1)*in/out))), and the fine pass's ownership tables behind them.  They depend on
// (H, W) only and are kept until another shape arrives.
static int pyr_tables(trl_ctx* c, int H, int W, const PyrLayout& lay, hipStream_t s) {
    if (c->pyr_tab != nullptr && c->pyr_tab_H == H && c->pyr_tab_W == W) return TRL_OK;
    std::vector<uint32_t> tab;
    for (int l = 0; l < lay.L; l++) {
        const PyrLevel& g = lay.lv[l];
        for (int i = 0; i < g.h; i++) tab.push_back((uint32_t)(((long long)i * H) / g.h) | ((uint32_t)((((long long)i + 1) * H + g.h - 1) / g.h) << 16));
        for (int i = 0; i < g.w; i++) tab.push_back((uint32_t)(((long long)i * W) / g.w) | ((uint32_t)((((long long)i + 1) * W + g.w - 1) / g.w) << 16));
    }
    pyr_fine_ownership(c, H, W, lay, tab);
    TRL_HIP(hipStreamSynchronize(s));                    // kernels in flight may still read the table this one replaces
    if (c->pyr_tab) TRL_HIP(hipFree(c->pyr_tab));
    c->pyr_tab = nullptr;
    TRL_HIP(hipMalloc((void**)&c->pyr_tab, tab.size() * 4 + 64));
    TRL_HIP(hipMemcpy(c->pyr_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    c->pyr_tab_H = H; c->pyr_tab_W = W;
    return TRL_OK;
}

// One build: the three launch steps below run in this order on j.s; each marks the levels it took in `taken` and records the kernel
// of each in the plan (trl_debug_pyramid_plan).
struct PyrJob { trl_ctx* c; const uint8_t* frames; int n, H, W; const PyrLayout& lay; PyrPx* pyr; hipStream_t s; };
static void plan_row(const PyrJob& j, int l, int kind, int rb, int cb, int cpb, int frames) {
    int32_t* r = j.c->hook.pyr_plan.row[l];
    r[0] = kind; r[1] = rb; r[2] = cb; r[3] = cpb; r[4] = frames; r[5] = j.lay.lv[l].khmax;
}

// Coarse levels (mode != 0): streaming passes in three row bands whatever the batch (at 256 x 720p that is one workgroup per resident
// slot at the kernel's 3 waves per SIMD; 4 and 6 bands measured slower on this kernel, 0.50 and 0.43 against 0.42 ms, and 5 and 8
// on its first stage, profiles/pyramid_stream_bands.txt: the rows a band reads past its end are read again; smaller batches were
// not swept), at most 8 levels per launch (register budget of the per-level
// snapshots), each launch reading the source once -- every source row once, so no Infinity-Cache chunking.  A group that does not
// meet the kernel's preconditions is left to the per-level kernels.  (Streaming the fine levels as well was measured: 1.75 vs
// 1.83 ms, not worth it.)
static int launch_coarse(const PyrJob& j, bool (&taken)[16]) {
    const int n = j.n, H = j.H, W = j.W;
    int lv_idx[16], nsel = 0;
    for (int l = 0; l < j.lay.L; l++) if (j.lay.lv[l].mode != 0) lv_idx[nsel++] = l;
    const bool wide = W * 3 > SBYTES;                                       // one workgroup cannot cover the row: wave-local pass
    for (int g0 = 0; g0 < nsel; g0 += 8) {
        const int gn = nsel - g0 < 8 ? nsel - g0 : 8;
        PyrStreamArgs sa;
        sa.nlev = 0;
        int tab_lo = 0x7fffffff, tab_hi = 0, kwm = 0;
        bool ok = true;
        for (int q = 0; q < gn; q++) {
            const PyrLevel& g = j.lay.lv[lv_idx[g0 + q]];
            if (g.khmax > 256) ok = false;                                   // a bin's column sum must fit 16 bits (it may wrap, see the kernel)
            tab_lo = g.ytab0 < tab_lo ? g.ytab0 : tab_lo;
            tab_hi = g.xtab0 + g.w > tab_hi ? g.xtab0 + g.w : tab_hi;
            kwm = g.kwmax > kwm ? g.kwmax : kwm;
            sa.lv[sa.nlev++] = g;
        }
        const int stab_words = tab_hi - tab_lo;                               // rows + columns of the group's levels (they are neighbours)
        sa.tab0 = tab_lo; sa.tab_words = stab_words;
        sa.H = H; sa.W = W; sa.n_frames = n; sa.pyr_stride = j.lay.pyr_stride;
        const int forced = j.c->opt.pyr_row_bands;                                // test hook: 0 = the policy below
        sa.row_bands = forced > 0 ? (forced < H ? forced : H) : (H >= 256 ? 3 : 1);
        sa.rows_per_band = (H + sa.row_bands - 1) / sa.row_bands;
        sa.row_bands = (H + sa.rows_per_band - 1) / sa.rows_per_band;         // every band has a row
        if (!ok || stab_words > STAB || n > 65535) continue;
        if (!wide) {
            if ((kwm + 2) * 3 > SBYTES / 2) continue;
            sa.col_bands = 1; sa.cols_per_band = W;
            const dim3 sgrid(sa.row_bands * sa.col_bands, n);
            const size_t lds = stream_strip_words<OwnBlock>() * 2 + (size_t)stab_words * 4;
            if (sa.nlev <= 4) k_pyramid_stream<4, OwnBlock><<<sgrid, 256, lds, j.s>>>(j.frames, sa, j.c->pyr_tab, j.pyr);
            else k_pyramid_stream<8, OwnBlock><<<sgrid, 256, lds, j.s>>>(j.frames, sa, j.c->pyr_tab, j.pyr);
        } else {
            // a wave covers 1280 bytes = 426 whole pixels of a row; the bins that start in its segment may reach kwmax further
            sa.cols_per_band = SW_BYTES / 3 - kwm;
            if (sa.cols_per_band < 64) continue;
            sa.col_bands = (W + sa.cols_per_band - 1) / sa.cols_per_band;
            sa.cols_per_band = (W + sa.col_bands - 1) / sa.col_bands;           // even segments
            // enough waves to fill the chip (~4 k) when the batch is small: more, shorter row bands (each reads on past its end
            // until its last bins are complete, so not shorter than 256 rows)
            int rbn = (4096 + n * sa.col_bands - 1) / (n * sa.col_bands);
            if (rbn > H / 256) rbn = H / 256;
            if (rbn > sa.row_bands && forced <= 0) { sa.row_bands = rbn; sa.rows_per_band = (H + rbn - 1) / rbn; }
            const dim3 sgrid((sa.row_bands * sa.col_bands + 3) / 4, n);
            const size_t lds = stream_strip_words<OwnWave>() * 2 + (size_t)stab_words * 4;
            if (sa.nlev <= 4) k_pyramid_stream<4, OwnWave><<<sgrid, 256, lds, j.s>>>(j.frames, sa, j.c->pyr_tab, j.pyr);
            else k_pyramid_stream<8, OwnWave><<<sgrid, 256, lds, j.s>>>(j.frames, sa, j.c->pyr_tab, j.pyr);
        }
        TRL_LAUNCH_CHECK();
        const int kind = wide ? (sa.nlev <= 4 ? TRL_PYR_SW4 : TRL_PYR_SW8) : (sa.nlev <= 4 ? TRL_PYR_S4 : TRL_PYR_S8);
        for (int q = 0; q < gn; q++) {
            taken[lv_idx[g0 + q]] = true;
            plan_row(j, lv_idx[g0 + q], kind, sa.row_bands, sa.col_bands, sa.cols_per_band, n);
        }
    }
    return TRL_OK;
}

// The finest levels in one pass over the source, when the shape has an ownership table (pyr_fine_ownership).
static int launch_fine(const PyrJob& j, bool (&taken)[16]) {
    const auto& pf = j.c->pyr_fine;
    if (!(pf.nlev >= 2 && j.n <= 65535 && pf.n_strips <= 65535)) return TRL_OK;
    PyrFineArgs fa;
    fa.H = j.H; fa.W = j.W; fa.n_frames = j.n; fa.pyr_stride = j.lay.pyr_stride;
    fa.nlev = pf.nlev; fa.band_cols = pf.band_cols; fa.strip_rows = pf.strip_rows;
    fa.n_bands = pf.n_bands; fa.n_strips = pf.n_strips; fa.own0 = pf.own0;
    for (int l = 0; l < 3; l++) fa.g[l] = j.lay.lv[l < fa.nlev ? l : 0];
    k_pyramid_fine<<<dim3(fa.n_bands, j.n, fa.n_strips), 192, 0, j.s>>>(j.frames, fa, j.c->pyr_tab, j.pyr);
    TRL_LAUNCH_CHECK();
    for (int l = 0; l < fa.nlev; l++) { taken[l] = true; plan_row(j, l, TRL_PYR_FINE, 0, 0, 0, j.n); }
    return TRL_OK;
}

// Every level no pass above took: one launch per (level, frame chunk).  Each level re-reads the whole source image, so frames are
// resampled in chunks whose source bytes fit the 256 MiB Infinity Cache: the 2nd..11th level launches of a chunk are served on-die
// instead of from HBM.
static int launch_per_level(const PyrJob& j, bool (&taken)[16]) {
    const int n = j.n;
    int chunk = (int)((176ll << 20) / ((long long)j.H * j.W * 3));
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    for (int f0 = 0; f0 < n; f0 += chunk) {
        const int nf = (n - f0 < chunk) ? n - f0 : chunk;
        for (int l = 0; l < j.lay.L; l++) {
            if (taken[l]) continue;
            PyrArgs pa;
            pa.H = j.H; pa.W = j.W; pa.n_frames = n; pa.f0 = f0; pa.pyr_stride = j.lay.pyr_stride; pa.g = j.lay.lv[l];
            const int threads = pa.g.pix_pad << pa.g.gshift;
            dim3 grid(pa.g.mode == 0 ? (threads + 511) / 512 : (threads + 255) / 256, nf);   // mode 0: two pixels per thread
            int kind;
            if (pa.g.mode == 0) {
                if (pa.g.khmax <= 3 && pa.g.nd <= 3) { kind = TRL_PYR_L0_3; k_pyramid0<3, false><<<grid, 256, 0, j.s>>>(j.frames, pa, j.c->pyr_tab, j.pyr); }
                else if (pa.g.khmax <= 4) { kind = TRL_PYR_L0_4; k_pyramid0<4, true><<<grid, 256, 0, j.s>>>(j.frames, pa, j.c->pyr_tab, j.pyr); }
                else { kind = TRL_PYR_L0_5; k_pyramid0<5, true><<<grid, 256, 0, j.s>>>(j.frames, pa, j.c->pyr_tab, j.pyr); }
            }
            else if (pa.g.mode == 1) { kind = TRL_PYR_L1; k_pyramid<1><<<grid, 256, 0, j.s>>>(j.frames, pa, j.c->pyr_tab, j.pyr); }
            else { kind = TRL_PYR_L2; k_pyramid<2><<<grid, 256, 0, j.s>>>(j.frames, pa, j.c->pyr_tab, j.pyr); }
            TRL_LAUNCH_CHECK();
            if (f0 == 0) plan_row(j, l, kind, 0, 0, 0, chunk);
        }
    }
    return TRL_OK;
}

int trl_pyramid_build(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, PyrLayout& lay, PyrPx** pyr_out, hipEvent_t* ev, hipStream_t s) {
    if (((uintptr_t)d_frames & 3) != 0) { trl_set_error("frame buffer must be 4-byte aligned"); return TRL_ERR_INVALID; }
    if (H > 16383 || W > 16383) { trl_set_error("frame larger than 16383 px"); return TRL_ERR_INVALID; }
    c->hook.pyr_plan.L = 0;
    TRL_CHECK(trl_pyramid_layout(c, H, W, lay));
    TRL_CHECK(pyr_tables(c, H, W, lay, s));
    PyrPx* pyr = (PyrPx*)c->scratch.alloc(trl_pyramid_bytes(lay, n));
    if (!pyr) { trl_set_error("pyramid workspace"); return TRL_ERR_STATE; }
    if (ev) TRL_HIP(hipEventRecord(ev[0], s));
    const PyrJob j{c, d_frames, n, H, W, lay, pyr, s};
    bool taken[16] = {};
    TRL_CHECK(launch_coarse(j, taken));
    TRL_CHECK(launch_fine(j, taken));
    TRL_CHECK(launch_per_level(j, taken));
    if (ev) TRL_HIP(hipEventRecord(ev[1], s));
    c->hook.pyr_plan.L = lay.L;
    *pyr_out = pyr;
    return TRL_OK;
}

// debug / test hook: level `level` of ONE frame's pyramid exactly as the fused PNet kernel reads it -> d_out [h][w][3]
__global__ void k_export_level(const PyrPx* __restrict__ pyr, int npix, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const PyrPx v = pyr[i];
    out[3 * i + 0] = v.b; out[3 * i + 1] = v.g; out[3 * i + 2] = v.r;
}
int trl_pyramid_export(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_out, int* h, int* w, hipStream_t s) {
    PyrLayout lay;
    PyrPx* pyr = nullptr;
    TRL_CHECK(trl_pyramid_build(c, d_frame, 1, H, W, lay, &pyr, nullptr, s));
    if (level < 0 || level >= lay.L) { trl_set_error("level %d out of range (%d levels)", level, lay.L); return TRL_ERR_INVALID; }
    const PyrLevel& g = lay.lv[level];
    k_export_level<<<(g.h * g.w + 255) / 256, 256, 0, s>>>(pyr + g.pix0, g.h * g.w, d_out);
    TRL_LAUNCH_CHECK();
    *h = g.h; *w = g.w;
    return TRL_OK;
}

// debug / test hook: the raw pyramid workspace of an n-frame batch (every frame, every level, the padding included) as the
// production pass above leaves it; d_out == nullptr: the layout alone
int trl_pyramid_export_batch(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_out, long long* pyr_stride,
                             int32_t* h_levels, int max_levels, int* n_levels, hipStream_t s) {
    PyrLayout lay;
    if (d_out) {
        PyrPx* pyr = nullptr;
        TRL_CHECK(trl_pyramid_build(c, d_frames, n, H, W, lay, &pyr, nullptr, s));
        TRL_HIP(hipMemcpyAsync(d_out, pyr, trl_pyramid_bytes(lay, n), hipMemcpyDeviceToDevice, s));
    } else {
        TRL_CHECK(trl_pyramid_layout(c, H, W, lay));
    }
    *pyr_stride = lay.pyr_stride;
    *n_levels = lay.L;
    for (int l = 0; l < lay.L && l < max_levels; l++) {
        const PyrLevel& g = lay.lv[l];
        h_levels[4 * l + 0] = g.pix0; h_levels[4 * l + 1] = g.h; h_levels[4 * l + 2] = g.w; h_levels[4 * l + 3] = g.pix_pad;
    }
    return TRL_OK;
}

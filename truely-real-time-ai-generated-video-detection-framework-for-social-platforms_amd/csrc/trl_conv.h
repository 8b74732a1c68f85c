// trl_conv.h -- what the implicit-GEMM convolution kernels share (trl_layers.hip, trl_fnconv.hip, trl_bf16.hip): the parts
// that define WHAT a convolution is -- output row -> input window, the k = (ky*KW + kx)*Cin + c walk, the bias-seeded chain,
// the epilogue, the accumulator layouts, the four-chain reduce -- each written once.  Tiles, staging and K-loop schedules stay
// with the kernels.  Everything is __forceinline__ and takes ConvArgs by const reference and the rest by value, so that after
// inlining the compiler sees the same uniform (scalar-register) values as in a hand-written body.
// profiles/conv_refactor_isa.txt compares the device code with the hand-written kernels'; three things it showed are kept
// here on purpose: sums keep the association the kernels had (mfma32_row takes the tile's first row), a value needed in a
// loop is computed once where the row is decoded (ConvRow::image), and a load that belongs under a uniform branch is passed
// as a callable, not as a value (conv_store).
#pragma once
#include "trl_ctx.h"
#include "trl_tailpool.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- output row m -> input window -----------------------------------------------------------------------------------------
// Row m of the GEMM is output pixel (image, oy, ox); its window starts at input pixel (iy0, ix0), which lies in the padding
// when negative.  A row that does not exist (`exists` false: past M, or past the tile) decodes as row 0: its loads stay in
// bounds and its results are never stored.
__device__ __forceinline__ bool conv_inside(const ConvArgs& a, int iy, int ix) { return (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W; }
struct ConvRow {
    int nimg, iy0, ix0;
    const float* image;   // channel 0 of the image's pixel (0, 0), 64-bit: for the kernels that serve inputs past 2^31 elements
    // 32-bit element offset of (image, iy0, ix0, channel 0) from a.x: for the kernels whose launcher checked trl_conv_small
    __device__ __forceinline__ int off(const ConvArgs& a) const { return ((nimg * a.H + iy0) * a.W + ix0) * a.ldx + a.xoff; }
    // tap (ky, kx) of the window lies inside the image, and its channel c there
    __device__ __forceinline__ bool inside(const ConvArgs& a, int ky, int kx) const { return conv_inside(a, iy0 + ky, ix0 + kx); }
    __device__ __forceinline__ const float* ptr(const ConvArgs& a, int ky, int kx, int c) const {
        return image + ((size_t)(iy0 + ky) * a.W + (ix0 + kx)) * a.ldx + c;
    }
};
__device__ __forceinline__ ConvRow conv_row(const ConvArgs& a, int m, bool exists) {
    const int mm = exists ? m : 0;
    const int ohw = a.OH * a.OW;
    const int nimg = mm / ohw;
    const int rem = mm - nimg * ohw;
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    return ConvRow{nimg, oy * a.sh - a.ph, ox * a.sw - a.pw, a.x + (size_t)nimg * a.H * a.W * a.ldx + a.xoff};
}

// ---- the k walk -------------------------------------------------------------------------------------------------------------
// Whole-tap chunks (Cin % BK == 0): every k of a chunk lies in one filter tap, so the cursor is uniform and lives on the scalar
// unit; a thread's gather address is its ConvRow::off plus soff().
struct TapCursor {
    int ky = 0, kx = 0, c0 = 0, k0 = 0;                     // the chunk starts at k0 = (ky*KW + kx)*Cin + c0
    __device__ __forceinline__ TapCursor() {}
    __device__ __forceinline__ TapCursor(const ConvArgs& a, int ks) {   // start at k = ks (a split-K quarter)
        const int tap = ks / a.Cin;
        c0 = ks - tap * a.Cin; ky = tap / a.KW; kx = tap - ky * a.KW; k0 = ks;
    }
    __device__ __forceinline__ int soff(const ConvArgs& a) const { return (ky * a.W + kx) * a.ldx + c0; }
    // the tap of a window that starts at (iy0, ix0) lies inside the image (kernels of layers without padding do not ask)
    __device__ __forceinline__ bool inside(const ConvArgs& a, int iy0, int ix0) const {
        return conv_inside(a, iy0 + ky, ix0 + kx);
    }
    __device__ __forceinline__ void advance(const ConvArgs& a, int bk) {   // next bk channels of the tap, else next tap
        k0 += bk; c0 += bk;
        if (c0 >= a.Cin) { c0 = 0; if (++kx == a.KW) { kx = 0; ++ky; } }
    }
};
// Chunks that may straddle taps: one cursor per float4 slot, advanced with a carry loop instead of two integer divisions per
// load (f32 MFMA shares the FP32 pipe with the VALU on gfx950, so every VALU instruction in the K loop is paid in matrix
// throughput).
struct SlotCursor {
    int c, kx, ky;
    __device__ __forceinline__ void start(const ConvArgs& a, int k) {
        const int tap = k / a.Cin;
        c = k - tap * a.Cin; ky = tap / a.KW; kx = tap - ky * a.KW;
    }
    __device__ __forceinline__ void advance(const ConvArgs& a, int bk) {   // (on copies: the carry loop then stays in registers)
        int cc = c + bk, x = kx, y = ky;
        while (cc >= a.Cin) {
            cc -= a.Cin;
            if (++x == a.KW) { x = 0; ++y; }
        }
        c = cc; kx = x; ky = y;
    }
};

// ---- chain head and epilogue ----------------------------------------------------------------------------------------------
// Every accumulator starts at the bias: the head of the oracle's fmaf chain.  Of the four chains of a split-K layer only
// chain 0 does (first_chain).
__device__ __forceinline__ float conv_bias(const ConvArgs& a, int n, bool first_chain = true) {
    return (first_chain && a.bias != nullptr && n < a.Cout) ? a.bias[n] : 0.f;
}
// Per-column epilogue constants live in registers.  The residual reaches conv_finish as a VALUE from the small-map kernels,
// which request the residual values of a lane's outputs before the K loop (stores may alias the residual buffer as far as the
// compiler knows: per-element load/store pairs would serialise on memory latency -- the first version of fn_conv spent 80 % of
// its time there), and as a callable that loads it from the trl_layers.hip kernels (conv_store), called only when the layer
// has a residual: the load stays under that branch, at the store.
struct ConvCol { float sc, sf, sl; };
__device__ __forceinline__ ConvCol conv_col(const ConvArgs& a, int n) {
    ConvCol c;
    const bool ok = n < a.Cout;
    c.sc = (a.scale && ok) ? a.scale[n] : 1.f;
    c.sf = (a.scale && ok) ? a.shift[n] : 0.f;
    c.sl = (a.act == TRL_ACT_PRELU && ok) ? a.slope[n] : 0.f;
    return c;
}
__device__ __forceinline__ float conv_residual(float r) { return r; }
template <typename F> __device__ __forceinline__ float conv_residual(F load) { return load(); }
template <typename R>
__device__ __forceinline__ float conv_finish(const ConvArgs& a, const ConvCol& c, float v, R r) {
    if (a.scale) v = __builtin_fmaf(v, c.sc, c.sf);
    if (a.res) {
        v = v * a.res_scale;
        v = v + conv_residual(r);
    }
    if (a.act == TRL_ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (a.act == TRL_ACT_PRELU) v = v > 0.f ? v : c.sl * v;
    return v;
}
__device__ __forceinline__ void conv_store(const ConvArgs& a, const ConvCol& c, int mr, int n, float v) {
    a.y[(size_t)mr * a.ldy + a.yoff + n] = conv_finish(a, c, v, [&]() { return a.res[(size_t)mr * a.ldres + n]; });
}
// ConvArgs::ysplit / yskip: how much further right output column n is stored (honoured by the trl_fnconv.hip kernels only)
__device__ __forceinline__ int conv_yskip(const ConvArgs& a, int n) { return n >= a.ysplit ? a.yskip : 0; }

// ---- accumulator register -> row of the MFMA tile (the column is lane & 31 / lane & 15) ---------------------------------------
// (the tile's first row goes in, not on top: the sum keeps the association the kernels' address arithmetic was tuned with)
__device__ __forceinline__ int mfma32_row(int row0, int i, int h) { return row0 + (i & 3) + 8 * (i >> 2) + 4 * h; }   // 32x32: i < 16, h = lane >> 5
__device__ __forceinline__ int mfma16_row(int row0, int q, int kq) { return row0 + kq * 4 + q; }                      // 16x16: q < 4, kq = lane >> 4

// ---- the pooling epilogue of conv_tap / conv_tap48 (geometry and the part / side / fix-up scheme: trl_tailpool.h) -----------------
// The kernels' POOL template flag is 0 (store the map) or the pooled layer's geometry: the row <-> cell arithmetic is then
// constants, multiplications and shifts -- with S, k and st in registers each cell costs integer divisions on the pipe the MFMAs
// use, more than its nine comparisons.
constexpr int conv_pool_flag(int S, int k, int st) { return (S << 8) | (k << 4) | st; }
template <int POOL, int BM> constexpr TailPool conv_pool_geom() { return TailPool{POOL >> 8, (POOL >> 4) & 15, POOL & 15, BM}; }
template <int POOL> struct ConvArgsOf { typedef ConvPoolArgs type; };
template <> struct ConvArgsOf<0> { typedef ConvArgs type; };
// what trl_conv_pool_family admits -- bias + PReLU, no folded BN, no residual -- said to the compiler, so that conv_finish in the
// epilogue is its PReLU expression and no test of the layer's options per accumulator
__device__ __forceinline__ void conv_pool_assume(const ConvArgs& a) {
    __builtin_assume(a.scale == nullptr);
    __builtin_assume(a.res == nullptr);
    __builtin_assume(a.act == TRL_ACT_PRELU);
}
// One pass: T holds columns nbase .. nbase + PWC - 1 of the finished tile, [BM][PWC].  A thread takes four channels of a cell the
// tile touches and reduces the window elements that lie in the tile, in maxpool_kernel's order and with its comparison.
template <int POOL, int BM, int PWC>
__device__ __forceinline__ void conv_pool_pass(const ConvPoolArgs& a, const float* T, int m0, int nbase, int tid) {
    constexpr TailPool tp = conv_pool_geom<POOL, BM>();
    constexpr int G = PWC / 4;                            // float4 groups per cell
    static_assert(tp.ok() && PWC % 4 == 0 && 256 % G == 0, "pooling epilogue geometry");
    const int t = m0 / BM;
    const int gend = (a.M / tp.per()) * tp.cells();       // cells of the launch
    const int g0 = tp.tile_cell0(t);
    int g1 = tp.tile_cell1(t);
    g1 = g1 < gend ? g1 : gend;
    const int c4 = tid % G;
#pragma unroll 1
    for (int g = g0 + tid / G; g < g1; g += 256 / G) {
        const int f = tp.first_row(g) - m0;               // tile row of the window's first element; < 0: it lies in the tile before
        f32x4 best = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
        for (int ky = 0; ky < tp.k; ky++)
#pragma unroll
            for (int kx = 0; kx < tp.k; kx++) {
                const int lr = f + ky * tp.S + kx;
                if ((unsigned)lr < (unsigned)BM) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(T + lr * PWC + 4 * c4);
#pragma unroll
                    for (int j = 0; j < 4; j++) best[j] = v[j] > best[j] ? v[j] : best[j];
                }
            }
        float* dst = (f < 0 ? a.side : a.y) + ((size_t)g * a.ldy + a.yoff + nbase + 4 * c4);
        *reinterpret_cast<f32x4*>(dst) = best;
    }
}

// ---- the four-chain tail of conv_splitk4 / conv_splitk4_tap ---------------------------------------------------------------
// Wave w holds chain w's partial 32x64 tile (two 32x32 accumulators).  Partials to LDS as [wave][tn][reg][lane] (8,192 floats),
// then each thread combines eight outputs as (c0 + c1) + (c2 + c3) -- the oracle's order -- finishes and stores them: element
// e = tid + 256 j of the [tn][reg][lane] tile, so a thread's column is its lane's in both halves and its registers are wave + 4 jj.
__device__ __forceinline__ void conv_split4_tail(const ConvArgs& a, float* red, const f32x16 (&acc)[2], int m0, int n0, int tid, int wave) {
    const int lane = tid & 63;
    __syncthreads();                                     // every wave is done with the staging buffers `red` overlays
#pragma unroll
    for (int tn = 0; tn < 2; tn++)
#pragma unroll
        for (int i = 0; i < 16; i++) red[((wave * 2 + tn) * 16 + i) * 64 + lane] = acc[tn][i];
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const int n = n0 + tn * 32 + (lane & 31);
        if (n >= a.Cout) continue;
        const ConvCol col = conv_col(a, n);
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const int e = tid + 256 * (4 * tn + jj);
            const int mr = mfma32_row(m0, (e >> 6) & 15, lane >> 5);
            if (mr < a.M) conv_store(a, col, mr, n, (red[e] + red[2048 + e]) + (red[4096 + e] + red[6144 + e]));
        }
    }
}

// ---- host: one launch of an f32 / 16-bit conv kernel of 256 threads, its choice recorded for the debug plans ------------------
typedef void (*ConvKernel)(ConvArgs);
inline int conv_launch(int family, int bm, int bn, int bk, int pad, ConvKernel k, const ConvArgs& a, dim3 grid, hipStream_t s) {
    g_trl_conv_choice = TrlConvChoice{family, bm, bn, bk, pad, 1};
    k<<<grid, 256, 0, s>>>(a);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
// a kernel with a PAD twin: the padded instantiation when the layer has spatial padding
inline int conv_launch_twin(int family, int bm, int bn, int bk, ConvKernel padded, ConvKernel plain, const ConvArgs& a, dim3 grid,
                            hipStream_t s) {
    const bool pad = a.ph || a.pw;
    return conv_launch(family, bm, bn, bk, pad, pad ? padded : plain, a, grid, s);
}

// trl_layers.hip -- generic NHWC layer kernels for gfx950 (MI355X).
//
// conv_igemm: implicit-GEMM convolution on the f32 matrix cores.
//   GEMM view   M = N*OH*OW output pixels, N = Cout, K = KH*KW*Cin, k = (ky*KW+kx)*Cin + c.
//   MFMA        v_mfma_f32_32x32x2_f32: one instruction = two chained fmaf per accumulator
//               (k, k+1), bit-identical to the scalar chain acc = fmaf(x[k], w[k], acc) with k
//               ascending (MI355X_MICROARCH "FP32-input MFMA").  The K loop below walks k in
//               ascending order and the accumulator starts at the bias, so the result equals
//               the oracle's conv2d() bit for bit whatever the tile shape.
//   layout      output channel on the MFMA column (= lane), pixels on the rows: per-channel
//               epilogue constants are lane constants and a store instruction writes 128-byte
//               channel runs of NHWC.
//   staging     A (pixels x k) gathered from NHWC into LDS as [k][m]; B (k x cout) as [k][n];
//               ds_read_b32 operand reads are conflict-free (32 consecutive floats per half-wave).
//               Next chunk's global loads are issued before the MFMAs of the current chunk.
//
// What every conv kernel shares -- row decode, the k cursors, the bias seed, the epilogue, the accumulator-to-row maps, the
// four-chain tail, the launch helpers -- is in trl_conv.h; the kernels below are tiles, loaders and K-loop schedules.
#include "trl_conv.h"

namespace {

template <int BM, int BN, int WM, int WN, int BK, bool VEC>
__global__ __launch_bounds__(256) void conv_igemm(ConvArgs a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int KG = BK / 4;                                   // float4 groups along k per chunk
    constexpr int ASLOTS = BM * KG, APT = (ASLOTS + 255) / 256;
    constexpr int BSLOTS = BK * (BN / 4), BPT = (BSLOTS + 255) / 256;
    static_assert(WM * WN == 4, "4 waves");
    __shared__ __attribute__((aligned(16))) float As[BK * BM];
    __shared__ __attribute__((aligned(16))) float Bs[BK * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= trl_live_rows(a)) return;     // device-sized batch: nothing of this tile exists (block-uniform)

    // ---- per-thread A row ------------------------------------------------------------------
    const int row = tid % BM;
    const int m = m0 + row;
    const bool mvalid = m < a.M;
    const ConvRow px = conv_row(a, m, mvalid);             // 64-bit addressing: this kernel serves inputs past 2^31 elements

    float4 areg[APT];
    float4 breg[BPT];
    const int kpad = (a.K + 15) & ~15;   // rows present in the zero-padded weight matrix

    SlotCursor cur[APT];                                   // the vector path's per-slot im2col cursors
#pragma unroll
    for (int i = 0; i < APT; i++) cur[i].start(a, 4 * ((tid + i * 256) / BM));
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int i = 0; i < APT; i++) {
            const int slot = tid + i * 256;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (slot < ASLOTS && mvalid) {
                const int k = k0 + 4 * (slot / BM);
                if (VEC) {
                    if (k < a.K && px.inside(a, cur[i].ky, cur[i].kx))
                        v = *reinterpret_cast<const float4*>(px.ptr(a, cur[i].ky, cur[i].kx, cur[i].c));
                } else {
                    float t[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int kk = k + j;
                        t[j] = 0.f;
                        if (kk < a.K) {
                            const int tap = kk / a.Cin, c = kk - tap * a.Cin;
                            const int ky = tap / a.KW, kx = tap - ky * a.KW;
                            if (px.inside(a, ky, kx)) t[j] = *px.ptr(a, ky, kx, c);
                        }
                    }
                    v = make_float4(t[0], t[1], t[2], t[3]);
                }
            }
            areg[i] = v;
            if (VEC) cur[i].advance(a, BK);   // to the next chunk
        }
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            const int slot = tid + i * 256;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (slot < BSLOTS) {
                const int kk = slot / (BN / 4), n = n0 + 4 * (slot % (BN / 4));
                if (n < a.ldw && k0 + kk < kpad) v = *reinterpret_cast<const float4*>(a.w + (size_t)(k0 + kk) * a.ldw + n);
            }
            breg[i] = v;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < APT; i++) {
            const int slot = tid + i * 256;
            if (slot < ASLOTS) {
                const int g = slot / BM;
                As[(4 * g + 0) * BM + row] = areg[i].x;
                As[(4 * g + 1) * BM + row] = areg[i].y;
                As[(4 * g + 2) * BM + row] = areg[i].z;
                As[(4 * g + 3) * BM + row] = areg[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            const int slot = tid + i * 256;
            if (slot < BSLOTS) {
                const int kk = slot / (BN / 4), n4 = slot % (BN / 4);
                *reinterpret_cast<float4*>(&Bs[kk * BN + 4 * n4]) = breg[i];
            }
        }
    };

    // ---- accumulators start at the bias (chain head) ---------------------------------------
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const float b = conv_bias(a, n0 + (wn * TN + tn) * 32 + r);
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[tm][tn][i] = b;
    }

    const int nchunks = (a.K + BK - 1) / BK;
    load_chunk(0);
    for (int ch = 0; ch < nchunks; ch++) {
        store_chunk();
        __syncthreads();
        if (ch + 1 < nchunks) load_chunk((ch + 1) * BK);
#pragma unroll
        for (int s = 0; s < BK / 2; s++) {
            float av[TM], bv[TN];
#pragma unroll
            for (int tm = 0; tm < TM; tm++) av[tm] = As[(2 * s + h) * BM + (wm * TM + tm) * 32 + r];
#pragma unroll
            for (int tn = 0; tn < TN; tn++) bv[tn] = Bs[(2 * s + h) * BN + (wn * TN + tn) * 32 + r];
#pragma unroll
            for (int tm = 0; tm < TM; tm++)
#pragma unroll
                for (int tn = 0; tn < TN; tn++)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- epilogue ------------------------------------------------------------------------------
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const int n = n0 + (wn * TN + tn) * 32 + r;
        if (n >= a.Cout) continue;
        const ConvCol col = conv_col(a, n);
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int mr = mfma32_row(m0 + (wm * TM + tm) * 32, i, h);
                if (mr < a.M) conv_store(a, col, mr, n, acc[tm][tn][i]);
            }
        }
    }
}

// ---- split-K(4) variant --------------------------------------------------------------------------------
// Tiny maps with long reductions (OH*OW <= 9, K >= 512: FaceNet's 3x3 / 1x1-spatial tail, the R/O-Net dense
// layers) have few output tiles and a serial chain of K/2 dependent 64-cycle MFMAs each.  The oracle defines
// their accumulation as four chains over consecutive quarters of k combined as (c0+c1)+(c2+c3); here wave w of
// a workgroup owns quarter w of one 32x64 output tile: staging is wave-private (no workgroup barrier in the K
// loop), the four SIMDs of the CU work on the same tile, and the chain per wave is four times shorter.
__global__ __launch_bounds__(256) void conv_splitk4(ConvArgs a) {
    constexpr int BM = 32, BN = 64, BK = 32;
    __shared__ __attribute__((aligned(16))) float As[4][BK * BM];
    __shared__ __attribute__((aligned(16))) float Bs[4][BK * BN];     // later: the 4 x (32x64) partial tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= trl_live_rows(a)) return;     // device-sized batch: nothing of this tile exists (block-uniform)
    const int segK = a.K >> 2, ks = wave * segK, ke = ks + segK;

    const int m = m0 + r;
    const bool mvalid = m < a.M;
    const ConvRow px = conv_row(a, m, mvalid);             // 64-bit addressing, as conv_igemm

    // A: 32 rows x 8 float4 groups per chunk = 4 slots per lane (same row, groups h, h+2, h+4, h+6)
    SlotCursor cur[4];
#pragma unroll
    for (int i = 0; i < 4; i++) cur[i].start(a, ks + 4 * (h + 2 * i));
    float4 areg[4], breg[8];
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + 4 * (h + 2 * i);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (mvalid && k < ke && px.inside(a, cur[i].ky, cur[i].kx))
                v = *reinterpret_cast<const float4*>(px.ptr(a, cur[i].ky, cur[i].kx, cur[i].c));
            areg[i] = v;
            cur[i].advance(a, BK);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int slot = lane + 64 * i;
            const int kk = slot >> 4, n = n0 + 4 * (slot & 15);
            breg[i] = (k0 + kk < ke && n < a.ldw) ? *reinterpret_cast<const float4*>(a.w + (size_t)(k0 + kk) * a.ldw + n)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float* Aw = As[wave];
    float* Bw = Bs[wave];
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int g = h + 2 * i;
            Aw[(4 * g + 0) * BM + r] = areg[i].x; Aw[(4 * g + 1) * BM + r] = areg[i].y;
            Aw[(4 * g + 2) * BM + r] = areg[i].z; Aw[(4 * g + 3) * BM + r] = areg[i].w;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int slot = lane + 64 * i;
            *reinterpret_cast<float4*>(&Bw[(slot >> 4) * BN + 4 * (slot & 15)]) = breg[i];
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const float b = conv_bias(a, n0 + tn * 32 + r, wave == 0);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[tn][i] = b;
    }
    load_chunk(ks);
    for (int k0 = ks; k0 < ke; k0 += BK) {
        store_chunk();                                   // wave-private staging: LDS ops of one wave stay in order
        if (k0 + BK < ke) load_chunk(k0 + BK);
#pragma unroll
        for (int s = 0; s < BK / 2; s++) {
            const float av = Aw[(2 * s + h) * BM + r];
            const float b0 = Bw[(2 * s + h) * BN + r], b1 = Bw[(2 * s + h) * BN + 32 + r];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
        }
    }
    conv_split4_tail(a, &Bs[0][0], acc, m0, n0, tid, wave);   // the staging buffers become the partial tiles
}

// conv_splitk4_tap: conv_splitk4 with whole-tap chunks (Cin % BKC == 0 and (K/4) % BKC == 0): the im2col cursor of a
// wave's quarter is a scalar, gather addresses are a per-lane 32-bit offset plus that scalar (see conv_tap).
template <int BKC, bool PAD>
__global__ __launch_bounds__(256) void conv_splitk4_tap(ConvArgs a) {
    constexpr int BM = 32, BN = 64;
    constexpr int AS = BKC / 8, BSL = BKC / 4;                        // float4 slots per lane: A (rows x k-groups), B
    __shared__ __attribute__((aligned(16))) float As[4][BKC * BM];
    __shared__ __attribute__((aligned(16))) float Bs[4][32 * BN];     // staging uses BKC rows; later the 4 x (32x64) partial tiles
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= trl_live_rows(a)) return;     // device-sized batch: nothing of this tile exists (block-uniform)
    const int segK = a.K >> 2, ks = wave * segK;

    const int m = m0 + r;
    const ConvRow px = conv_row(a, m, m < a.M);
    const int aoff = px.off(a) + 4 * h;
    int bn = n0 + 4 * (lane & 15);
    bn = bn < a.ldw ? bn : 0;
    const int boff = (lane >> 4) * a.ldw + bn;

    TapCursor cur(a, ks);                                    // scalar cursor of the wave's quarter
    f32x4 areg[AS], breg[BSL];
    auto load_chunk = [&]() __attribute__((always_inline)) {
        const int soff = cur.soff(a);
        bool inside = true;
        if (PAD) inside = cur.inside(a, px.iy0, px.ix0);
#pragma unroll
        for (int i = 0; i < AS; i++) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (inside) v = *reinterpret_cast<const f32x4*>(a.x + (aoff + soff + 8 * i));
            areg[i] = v;
        }
        const float* wrow = a.w + (size_t)cur.k0 * a.ldw;
#pragma unroll
        for (int i = 0; i < BSL; i++) breg[i] = *reinterpret_cast<const f32x4*>(wrow + (boff + 4 * i * a.ldw));
        cur.advance(a, BKC);
    };
    float* Aw = As[wave];
    float* Bw = Bs[wave];
    auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < AS; i++) {
            const int g = h + 2 * i;
            Aw[(4 * g + 0) * BM + r] = areg[i][0]; Aw[(4 * g + 1) * BM + r] = areg[i][1];
            Aw[(4 * g + 2) * BM + r] = areg[i][2]; Aw[(4 * g + 3) * BM + r] = areg[i][3];
        }
#pragma unroll
        for (int i = 0; i < BSL; i++) *reinterpret_cast<f32x4*>(&Bw[((lane >> 4) + 4 * i) * BN + 4 * (lane & 15)]) = breg[i];
    };

    f32x16 acc[2];
#pragma unroll
    for (int tn = 0; tn < 2; tn++) {
        const float b = conv_bias(a, n0 + tn * 32 + r, wave == 0);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[tn][i] = b;
    }
    const int nchunks = segK / BKC;
    load_chunk();
    for (int ch = 0; ch < nchunks; ch++) {
        store_chunk();                                   // wave-private staging: LDS ops of one wave stay in order
        if (ch + 1 < nchunks) load_chunk();
#pragma unroll
        for (int s = 0; s < BKC / 2; s++) {
            const float av = Aw[(2 * s + h) * BM + r];
            const float b0 = Bw[(2 * s + h) * BN + r], b1 = Bw[(2 * s + h) * BN + 32 + r];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, acc[1], 0, 0, 0);
        }
    }
    conv_split4_tail(a, &Bs[0][0], acc, m0, n0, tid, wave);   // the staging buffers become the partial tiles
}

// conv_tap: the same implicit GEMM for layers whose K chunks never straddle a filter tap (Cin % BK == 0): the
// im2col cursor (ky, kx, c0) of a chunk is then UNIFORM and lives on the scalar unit, a thread's gather address is
// one 32-bit per-thread offset plus that scalar, rows past M re-read row 0 (their results are never stored) and the
// weight matrix is addressed the same way.  The K loop of conv_igemm spends ~160 VALU instructions per chunk on
// per-slot cursors and bounds tests; f32 MFMA and VALU share the FP32 pipe on gfx950, so that was ~30 % of the
// loop.  Here it is ~20.  Same k order, same bias-seeded chain: bit-identical results.
// PAD = the layer has spatial padding (taps falling outside the image load nothing and contribute zeros).
// POOL != 0 (conv_pool_flag: the geometry of the max pool behind the layer): the map is not stored -- the finished tile is staged in
// LDS, 32 columns at a time over the dead A operand buffer, and the part of every pooling window that lies in this tile is reduced there (trl_tailpool.h).
template <int BM, int BN, int WM, int WN, int BK, bool PAD, int POOL = 0>
__global__ __launch_bounds__(256) void conv_tap(typename ConvArgsOf<POOL>::type a) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int KG = BK / 4;                                   // float4 groups along k per chunk
    constexpr int ASLOTS = BM * KG, APT = (ASLOTS + 255) / 256;
    constexpr int BSLOTS = BK * (BN / 4), BPT = (BSLOTS + 255) / 256;
    constexpr int LDA = BK + 1;                                  // A tile [m][k], odd row stride: operand reads (lane = row) and the staging writes are conflict-free
    static_assert(WM * WN == 4 && BK % 4 == 0 && BK % 2 == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) float As[BM * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[BK * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (m0 >= trl_live_rows(a)) return;     // device-sized batch: nothing of this tile exists (block-uniform)

    // ---- A slots: slot = tid + 256 i -> (k-group = slot % KG, row = slot / KG).  The KG lanes of a row read the BK contiguous
    // channels one pixel contributes to a chunk, so a wave's load touches 64 / KG pixels' lines instead of 64 (row-per-lane
    // gathers spend the vector L1's request rate, not its bandwidth: round 2).  Element offset of
    // (image, iy0, ix0, channel 4 g) from a.x; rows past M re-read row 0 (never stored).
    int aoff[APT], adst[APT], iy0v[APT], ix0v[APT];
#pragma unroll
    for (int i = 0; i < APT; i++) {
        const int slot = tid + 256 * i;
        const int g = slot % KG, row = slot / KG;
        const int m = m0 + row;
        const ConvRow px = conv_row(a, m, m < a.M && row < BM);
        iy0v[i] = px.iy0; ix0v[i] = px.ix0;
        aoff[i] = px.off(a) + 4 * g;                            // < 2^31: checked by the launcher
        adst[i] = row * LDA + 4 * g;
    }
    // ---- per-thread B slot: (k row kk0, column n) ------------------------------------------------------------
    const int bkk = tid / (BN / 4), bn4 = tid % (BN / 4);
    int bn = n0 + 4 * bn4;
    bn = bn < a.ldw ? bn : 0;                                   // columns past the matrix re-read column 0 (never stored)
    const int boff = bkk * a.ldw + bn;
    constexpr int BKSTEP = 256 / (BN / 4);                       // k-row stride between a thread's B slots

    float4 areg[APT];
    float4 breg[BPT];
    TapCursor cur;                                              // scalar cursor of the NEXT chunk to load
    auto load_chunk = [&]() {
        const int soff = cur.soff(a);                           // scalar
#pragma unroll
        for (int i = 0; i < APT; i++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            bool ok = ASLOTS % 256 == 0 || tid + i * 256 < ASLOTS;
            if (PAD) ok &= cur.inside(a, iy0v[i], ix0v[i]);
            if (ok) v = *reinterpret_cast<const float4*>(a.x + (aoff[i] + soff));
            areg[i] = v;
        }
        const float* wrow = a.w + (size_t)cur.k0 * a.ldw;       // scalar
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BSLOTS % 256 == 0 || tid + i * 256 < BSLOTS) v = *reinterpret_cast<const float4*>(wrow + (boff + BKSTEP * i * a.ldw));
            breg[i] = v;
        }
        cur.advance(a, BK);
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < APT; i++) {
            if (ASLOTS % 256 == 0 || tid + i * 256 < ASLOTS) {
                As[adst[i] + 0] = areg[i].x; As[adst[i] + 1] = areg[i].y;
                As[adst[i] + 2] = areg[i].z; As[adst[i] + 3] = areg[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            if (BSLOTS % 256 == 0 || tid + i * 256 < BSLOTS)
                *reinterpret_cast<float4*>(&Bs[(bkk + BKSTEP * i) * BN + 4 * bn4]) = breg[i];
        }
    };

    // ---- accumulators start at the bias (chain head) ---------------------------------------
    f32x16 acc[TM][TN];
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const float b = conv_bias(a, n0 + (wn * TN + tn) * 32 + r);
#pragma unroll
        for (int tm = 0; tm < TM; tm++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[tm][tn][i] = b;
    }

    const int nchunks = a.K / BK;
    load_chunk();
    for (int ch = 0; ch < nchunks; ch++) {
        store_chunk();
        __syncthreads();
        if (ch + 1 < nchunks) load_chunk();
#pragma unroll
        for (int s = 0; s < BK / 2; s++) {
            float av[TM], bv[TN];
#pragma unroll
            for (int tm = 0; tm < TM; tm++) av[tm] = As[((wm * TM + tm) * 32 + r) * LDA + 2 * s + h];
#pragma unroll
            for (int tn = 0; tn < TN; tn++) bv[tn] = Bs[(2 * s + h) * BN + (wn * TN + tn) * 32 + r];
#pragma unroll
            for (int tm = 0; tm < TM; tm++)
#pragma unroll
                for (int tn = 0; tn < TN; tn++)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- pooling epilogue: bias + PReLU as conv_finish does, then one 32-column half of the tile at a time ------------------------
    if constexpr (POOL != 0) {
        static_assert(TN == 1 && BM * 32 <= BM * LDA, "a [BM][32] half tile fits the A buffer");
        conv_pool_assume(a);
        const ConvCol col = conv_col(a, n0 + wn * 32 + r);
        for (int p = 0; p < WN; p++) {
            if (wn == p) {
#pragma unroll
                for (int tm = 0; tm < TM; tm++)
#pragma unroll
                    for (int i = 0; i < 16; i++) As[mfma32_row((wm * TM + tm) * 32, i, h) * 32 + r] = conv_finish(a, col, acc[tm][0][i], 0.f);
            }
            __syncthreads();
            conv_pool_pass<POOL, BM, 32>(a, As, m0, n0 + p * 32, tid);
            __syncthreads();
        }
        return;
    }

    // ---- epilogue ------------------------------------------------------------------------------
#pragma unroll
    for (int tn = 0; tn < TN; tn++) {
        const int n = n0 + (wn * TN + tn) * 32 + r;
        if (n >= a.Cout) continue;
        const ConvCol col = conv_col(a, n);
#pragma unroll
        for (int tm = 0; tm < TM; tm++) {
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int mr = mfma32_row(m0 + (wm * TM + tm) * 32, i, h);
                if (mr < a.M) conv_store(a, col, mr, n, acc[tm][tn][i]);
            }
        }
    }
}

// conv_tap48: whole-tap implicit GEMM for Cout = 48 (R-Net conv2, 31 k candidates x 81 pixels per step): a 128 x 48 tile on
// v_mfma_f32_16x16x4_f32 -- three 16-column tiles instead of two 32-column ones, so no MFMA cycle is spent on the 16 padding
// columns a 64-wide tile would carry (25 % of that layer).  Same LDS layout ([k][m], [k][n]) and loader as conv_tap; each of the
// 4 waves owns 32 rows = 2 x 3 accumulator tiles; k = 4s + (lane >> 4) ascending, bias-seeded: the oracle's chain.
// POOL: as conv_tap's, 16 columns (one accumulator tile column) at a time.
template <int BK, bool PAD, int POOL = 0>
__global__ __launch_bounds__(256) void conv_tap48(typename ConvArgsOf<POOL>::type a) {
    constexpr int BM = 128, BN = 48;
    constexpr int KG = BK / 4;
    constexpr int ASLOTS = BM * KG, APT = (ASLOTS + 255) / 256;
    constexpr int BSLOTS = BK * (BN / 4), BPT = (BSLOTS + 255) / 256;
    constexpr int GSTEP = 256 / BM;
    static_assert(BK % 4 == 0, "k-steps of 4");
    __shared__ __attribute__((aligned(16))) float As[BK * BM];
    __shared__ __attribute__((aligned(16))) float Bs[BK * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * BM;
    __builtin_assume(a.Cout == BN);         // the launcher's condition: no column of the tile lies past the layer's
    if (m0 >= trl_live_rows(a)) return;     // device-sized batch: nothing of this tile exists (block-uniform)

    const int row = tid % BM, g0 = tid / BM;
    // (row decode and cursor written out, not ConvRow / TapCursor: with them this kernel's reordered code measured 1.2 % slower,
    // profiles/conv_refactor_timing.txt; as it stands its device code equals the hand-written kernel's)
    const int m = m0 + row;
    const int mm = m < a.M ? m : 0;
    const int ohw = a.OH * a.OW;
    const int nimg = mm / ohw;
    const int rem = mm - nimg * ohw;
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    const int iy0 = oy * a.sh - a.ph, ix0 = ox * a.sw - a.pw;
    const int aoff = ((nimg * a.H + iy0) * a.W + ix0) * a.ldx + a.xoff + 4 * g0;
    // B slots: slot = tid + 256 i -> (k row, column group of 4); 12 groups per row
    int boff[BPT], bdst[BPT];
#pragma unroll
    for (int i = 0; i < BPT; i++) {
        const int slot = tid + 256 * i, kk = slot / (BN / 4), n4 = slot - kk * (BN / 4);
        boff[i] = kk * a.ldw + 4 * n4;
        bdst[i] = kk * BN + 4 * n4;
    }

    float4 areg[APT];
    float4 breg[BPT];
    int ky = 0, kx = 0, c0 = 0, k0 = 0;
    auto load_chunk = [&]() {
        const int soff = (ky * a.W + kx) * a.ldx + c0;
        bool inside = true;
        if (PAD) inside = (unsigned)(iy0 + ky) < (unsigned)a.H && (unsigned)(ix0 + kx) < (unsigned)a.W;
#pragma unroll
        for (int i = 0; i < APT; i++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((ASLOTS % 256 == 0 || tid + i * 256 < ASLOTS) && inside)
                v = *reinterpret_cast<const float4*>(a.x + (aoff + soff + 4 * GSTEP * i));
            areg[i] = v;
        }
        const float* wrow = a.w + (size_t)k0 * a.ldw;
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BSLOTS % 256 == 0 || tid + i * 256 < BSLOTS) v = *reinterpret_cast<const float4*>(wrow + boff[i]);
            breg[i] = v;
        }
        k0 += BK; c0 += BK;
        if (c0 >= a.Cin) { c0 = 0; if (++kx == a.KW) { kx = 0; ++ky; } }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < APT; i++) {
            if (ASLOTS % 256 == 0 || tid + i * 256 < ASLOTS) {
                const int g = g0 + GSTEP * i;
                As[(4 * g + 0) * BM + row] = areg[i].x;
                As[(4 * g + 1) * BM + row] = areg[i].y;
                As[(4 * g + 2) * BM + row] = areg[i].z;
                As[(4 * g + 3) * BM + row] = areg[i].w;
            }
        }
#pragma unroll
        for (int i = 0; i < BPT; i++) {
            if (BSLOTS % 256 == 0 || tid + i * 256 < BSLOTS) *reinterpret_cast<float4*>(&Bs[bdst[i]]) = breg[i];
        }
    };

    f32x4 acc[2][3];
#pragma unroll
    for (int tn = 0; tn < 3; tn++) {
        const float b = conv_bias(a, tn * 16 + l15);
#pragma unroll
        for (int tm = 0; tm < 2; tm++) acc[tm][tn] = f32x4{b, b, b, b};
    }

    const int nchunks = a.K / BK;
    load_chunk();
    for (int ch = 0; ch < nchunks; ch++) {
        store_chunk();
        __syncthreads();
        if (ch + 1 < nchunks) load_chunk();
#pragma unroll
        for (int s = 0; s < BK / 4; s++) {
            float av[2], bv[3];
#pragma unroll
            for (int tm = 0; tm < 2; tm++) av[tm] = As[(4 * s + kq) * BM + wave * 32 + tm * 16 + l15];
#pragma unroll
            for (int tn = 0; tn < 3; tn++) bv[tn] = Bs[(4 * s + kq) * BN + tn * 16 + l15];
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int tn = 0; tn < 3; tn++)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tm], bv[tn], acc[tm][tn], 0, 0, 0);
        }
        __syncthreads();
    }

    if constexpr (POOL != 0) {
        static_assert(BM * 16 <= BK * BM, "a [BM][16] tile column fits the A buffer");
        conv_pool_assume(a);
#pragma unroll
        for (int tn = 0; tn < 3; tn++) {
            const ConvCol col = conv_col(a, tn * 16 + l15);
#pragma unroll
            for (int tm = 0; tm < 2; tm++)
#pragma unroll
                for (int q = 0; q < 4; q++) As[mfma16_row(wave * 32 + tm * 16, q, kq) * 16 + l15] = conv_finish(a, col, acc[tm][tn][q], 0.f);
            __syncthreads();
            conv_pool_pass<POOL, BM, 16>(a, As, m0, tn * 16, tid);
            __syncthreads();
        }
        return;
    }

#pragma unroll
    for (int tn = 0; tn < 3; tn++) {
        const int n = tn * 16 + l15;
        const ConvCol col = conv_col(a, n);
#pragma unroll
        for (int tm = 0; tm < 2; tm++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int mr = mfma16_row(m0 + wave * 32 + tm * 16, q, kq);
                if (mr >= a.M) continue;
                conv_store(a, col, mr, n, acc[tm][tn][q]);
            }
        }
    }
}

// ---- launchers: one per kernel family; the recorded choice and the PAD twin are conv_launch_twin's business ---------------
template <int BM, int BN, int WM, int WN, int BK>
int launch_tap(const ConvArgs& a, dim3 grid, hipStream_t s) {
    return conv_launch_twin(TRL_FNK_CONV_TAP, BM, BN, BK, conv_tap<BM, BN, WM, WN, BK, true>, conv_tap<BM, BN, WM, WN, BK, false>, a, grid, s);
}
template <int BK>
int launch_tap48(const ConvArgs& a, hipStream_t s) {
    return conv_launch_twin(TRL_FNK_TAP48, 128, 48, BK, conv_tap48<BK, true>, conv_tap48<BK, false>, a, dim3((a.M + 127) / 128, 1), s);
}
template <int BKC>
int launch_splitk4_tap(const ConvArgs& a, dim3 grid, hipStream_t s) {
    return conv_launch_twin(TRL_FNK_SPLITK4_TAP, 32, 64, BKC, conv_splitk4_tap<BKC, true>, conv_splitk4_tap<BKC, false>, a, grid, s);
}

template <int BM, int BN, int WM, int WN, int BK>
int launch_cfg(const ConvArgs& a, bool vec, hipStream_t s) {
    dim3 grid((a.M + BM - 1) / BM, (a.Cout + BN - 1) / BN);
    if (vec && trl_conv_small(a)) {   // whole-tap chunks (conv_tap) whenever the channel count allows it
        if (BK >= 64 && a.Cin % 64 == 0) return launch_tap<BM, BN, WM, WN, 64>(a, grid, s);
        if (a.Cin % 32 == 0) return launch_tap<BM, BN, WM, WN, 32>(a, grid, s);
        if (BM == 128 && BN == 64 && a.Cin % 28 == 0) return launch_tap<BM, BN, WM, WN, 28>(a, grid, s);
        if (a.Cin % 16 == 0) return launch_tap<BM, BN, WM, WN, 16>(a, grid, s);
    }
    if (vec) return conv_launch(TRL_FNK_IGEMM_VEC, BM, BN, BK, 0, conv_igemm<BM, BN, WM, WN, BK, true>, a, grid, s);
    return conv_launch(TRL_FNK_IGEMM_SCALAR, BM, BN, 16, 0, conv_igemm<BM, BN, WM, WN, 16, false>, a, grid, s);
}

// ---- max pool -------------------------------------------------------------------------------
template <int V>   // V channels per thread (4 when every stride / offset is a multiple of 4 floats)
__global__ void maxpool_kernel(const float* __restrict__ x, int N, int H, int W, int C, int ldx, int xoff,
                               int k, int st, float* __restrict__ y, int ldy, int yoff, int OH, int OW,
                               const int32_t* __restrict__ n_dev, int n_base) {
    const int CV = C / V;
    if (n_dev) {   // device-sized batch: the first clamp(*n_dev - n_base, 0, N) items exist
        int t = *n_dev - n_base;
        N = t < 0 ? 0 : (t > N ? N : t);
    }
    const size_t total = (size_t)N * OH * OW * CV;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % CV) * V;
        size_t pix = idx / CV;
        const int ox = (int)(pix % OW); pix /= OW;
        const int oy = (int)(pix % OH);
        const int n = (int)(pix / OH);
        float best[V];
#pragma unroll
        for (int j = 0; j < V; j++) best[j] = -INFINITY;
        for (int ky = 0; ky < k; ky++) {
            const int iy = oy * st + ky;
            if (iy >= H) break;
            for (int kx = 0; kx < k; kx++) {
                const int ix = ox * st + kx;
                if (ix >= W) break;
                const float* p = x + (((size_t)n * H + iy) * W + ix) * ldx + xoff + c;
                if (V == 4) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    best[0] = v.x > best[0] ? v.x : best[0]; best[1] = v.y > best[1] ? v.y : best[1];
                    best[2 % V] = v.z > best[2 % V] ? v.z : best[2 % V]; best[3 % V] = v.w > best[3 % V] ? v.w : best[3 % V];
                } else {
                    best[0] = p[0] > best[0] ? p[0] : best[0];
                }
            }
        }
        float* q = y + (((size_t)n * OH + oy) * OW + ox) * ldy + yoff + c;
        if (V == 4) *reinterpret_cast<float4*>(q) = make_float4(best[0], best[1 % V], best[2 % V], best[3 % V]);
        else q[0] = best[0];
    }
}

// The fix-up behind a pooling epilogue: block b - 1 takes the cells cut by the boundary in front of tile b, whose second part lies in
// `side`, and finishes them: pooled = side > pooled ? side : pooled (the scan's own comparison, trl_tailpool.h).  Boundaries at or
// past the live rows have no cell of a live candidate.
__global__ __launch_bounds__(128) void pool_fixup_kernel(float* __restrict__ y, const float* __restrict__ side, int ld, int yoff, int C,
                                                          TailPool tp, int N, const int32_t* __restrict__ n_dev, int n_base) {
    if (n_dev) {   // device-sized batch, as maxpool_kernel
        int t = *n_dev - n_base;
        N = t < 0 ? 0 : (t > N ? N : t);
    }
    const int b = blockIdx.x + 1;
    if ((long long)b * tp.BM >= (long long)N * tp.per()) return;
    const int g0 = tp.cut_cell0(b), gend = N * tp.cells();
    int g1 = tp.cut_cell1(b);
    g1 = g1 < gend ? g1 : gend;
    const int G = C / 4;
    for (int w = threadIdx.x; w < (g1 - g0) * G; w += blockDim.x) {
        const int g = g0 + w / G, c4 = w - (w / G) * G;
        const size_t e = (size_t)g * ld + yoff + 4 * c4;
        const float4 A = *reinterpret_cast<const float4*>(y + e), B = *reinterpret_cast<const float4*>(side + e);
        *reinterpret_cast<float4*>(y + e) = make_float4(B.x > A.x ? B.x : A.x, B.y > A.y ? B.y : A.y, B.z > A.z ? B.z : A.z, B.w > A.w ? B.w : A.w);
    }
}

// AdaptiveAvgPool2d(1): sequential row-major sum / count (oracle order)
__global__ void gap_kernel(const float* __restrict__ x, int N, int HW, int C, float* __restrict__ y) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * C) return;
    const int n = idx / C, c = idx - n * C;
    float s = 0.f;
    for (int p = 0; p < HW; p++) s = s + x[((size_t)n * HW + p) * C + c];
    y[idx] = s / (float)HW;
}

// F.normalize(p=2, dim=1, eps=1e-12) on [n][512]; one wave per row.
__global__ __launch_bounds__(64) void l2norm512_kernel(const float* __restrict__ x, const uint8_t* __restrict__ valid,
                                                       int n, float* __restrict__ y) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= n) return;
    const float* v = x + (size_t)row * 512;
    float* o = y + (size_t)row * 512;
    if (valid && !valid[row]) {
        for (int i = 0; i < 8; i++) o[lane + 64 * i] = 0.f;
        return;
    }
    float nrm = sqrtf(trl_wave_dot512(v, v, lane));
    if (nrm < 1e-12f) nrm = 1e-12f;
    for (int i = 0; i < 8; i++) o[lane + 64 * i] = v[lane + 64 * i] / nrm;
}

// trl_facenet_features: what l2norm512_kernel reads, copied out (zero rows where !valid)
__global__ __launch_bounds__(64) void feat512_kernel(const float* __restrict__ x, const uint8_t* __restrict__ valid, int n, float* __restrict__ y) {
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= n) return;
    const bool live = !valid || valid[row];
    for (int i = 0; i < 8; i++) y[(size_t)row * 512 + lane + 64 * i] = live ? x[(size_t)row * 512 + lane + 64 * i] : 0.f;
}

// Carry of the drift state machine between consecutive windows of one clip (trl_drift_update): what model.py's loop variables
// `previous_embedding`, `consecutive_count` and `ai_detected_frames` hold between two sampled frames (model.py:60-75).
struct DriftState {
    float prev[512];                 // embedding of the last frame that had one (model.py:75)
    int32_t has_prev, run, hits, pad;
};
static_assert(sizeof(DriftState) == TRL_DRIFT_STATE_BYTES, "drift state layout");

// server/model.py:60-61 -- cosine similarity of every embedded frame with the previous embedded frame.
// One wave per sampled frame; the three 512-long dots use the oracle's fixed lane order (trl_wave_dot512).
// `st` (optional): the window continues a clip -- a frame with no embedded predecessor inside the window compares with st->prev.
__global__ __launch_bounds__(256) void drift_sims_kernel(const float* __restrict__ emb, const uint8_t* __restrict__ valid, int n,
                                                         float* __restrict__ sims, const DriftState* __restrict__ st) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    float sim = 2.0f;                       // 2.0 = "no comparison happened"
    if (valid[i]) {
        int prev = i - 1;
        while (prev >= 0 && !valid[prev]) prev--;   // frames without a face neither compare nor replace `previous` (model.py:48-75)
        const float* pv = prev >= 0 ? emb + (size_t)prev * 512 : ((st && st->has_prev) ? st->prev : nullptr);
        if (pv) {
            const float* cur = emb + (size_t)i * 512;
            const float d = trl_wave_dot512(cur, pv, lane);
            const float na = sqrtf(trl_wave_dot512(cur, cur, lane)), nb = sqrtf(trl_wave_dot512(pv, pv, lane));
            sim = d / (na * nb);
        }
    }
    if (lane == 0) sims[i] = sim;
}

// server/model.py:62-66,70,86-95 -- the run-length state machine is a scan over the similarities: staged in
// LDS in chunks, walked by one lane, then the score in double like the reference's Python floats.
// `st` (optional): counters start from the carried state, which then takes the window's final counters and last embedding.
__global__ __launch_bounds__(256) void drift_scan_kernel(const float* __restrict__ sims, int n, long long frame_count, int fps,
                                                         uint8_t* __restrict__ flags, int32_t* __restrict__ result,
                                                         DriftState* __restrict__ st, const float* __restrict__ emb,
                                                         const uint8_t* __restrict__ valid) {
    __shared__ float sh[4096];
    __shared__ uint8_t fl[4096];
    __shared__ int last_valid;
    const float thr_sim = 0.99f;   // model.py:16
    const int thr_frames = 15;     // model.py:17
    int run = st ? st->run : 0, hits = st ? st->hits : 0;
    if (threadIdx.x == 0) last_valid = -1;
    for (int base = 0; base < n; base += 4096) {
        const int m = (n - base) < 4096 ? (n - base) : 4096;
        for (int t = threadIdx.x; t < m; t += blockDim.x) sh[t] = sims[base + t];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int t = 0; t < m; t++) {
                const float sim = sh[t];
                uint8_t f = 0;
                if (sim != 2.0f) {          // a comparison happened: every value but the sentinel, NaN and +-inf included
                    run = (sim < thr_sim) ? run + 1 : 0;   // (NaN and +inf are not below the threshold: model.py:62-65 resets)
                    if (run > thr_frames) { hits++; f = 1; }
                }
                fl[t] = f;
            }
        }
        __syncthreads();
        if (flags) for (int t = threadIdx.x; t < m; t += blockDim.x) flags[base + t] = fl[t];
        if (st) for (int t = threadIdx.x; t < m; t += blockDim.x) if (valid[base + t]) atomicMax(&last_valid, base + t);
        __syncthreads();
    }
    if (st) {                               // (the similarities were computed by the previous kernel: st->prev is free to change)
        __syncthreads();
        const int lv = last_valid;
        if (lv >= 0) for (int t = threadIdx.x; t < 512; t += blockDim.x) st->prev[t] = emb[(size_t)lv * 512 + t];
    }
    if (threadIdx.x == 0) {
        if (st) { st->run = run; st->hits = hits; if (last_valid >= 0) st->has_prev = 1; }
        long long total = 0;
        const int score = trl_drift_score_value(hits, run, frame_count, fps, &total);
        result[0] = score; result[1] = run; result[2] = hits; result[3] = (int32_t)total;
    }
}

}  // namespace

int trl_launch_conv(const ConvArgs& a, hipStream_t s) {
    if (a.M <= 0) return TRL_OK;
    if (trl_fn_eligible(a)) return trl_launch_fn_group(&a, 1, s);   // small maps (FaceNet's 7x7 / 3x3 / 1x1 stages): trl_fnconv.hip
    const bool vec = trl_conv_vec(a), small = trl_conv_small(a);
    if (trl_fn_split4_rule(a)) {                                    // four chains: one wave per quarter of k, a 32x64 tile per workgroup
        if (!vec) { trl_set_error("split-K layer needs Cin %% 4 == 0 and 16-byte aligned input"); return TRL_ERR_INVALID; }
        const dim3 grid((a.M + 31) / 32, (a.Cout + 63) / 64);
        const int segK = a.K >> 2;
        if (small && a.Cin % 32 == 0 && segK % 32 == 0) return launch_splitk4_tap<32>(a, grid, s);
        if (small && a.Cin % 16 == 0 && segK % 16 == 0) return launch_splitk4_tap<16>(a, grid, s);
        return conv_launch(TRL_FNK_SPLITK4, 32, 64, 32, 0, conv_splitk4, a, grid, s);
    }
    // Cout == 48 with whole-tap chunks: the 128 x 48 tile (no padded MFMA columns)
    if (vec && small && a.Cout == 48 && a.ldw >= 48 && a.M >= 16384) {
        if (a.Cin % 32 == 0) return launch_tap48<32>(a, s);
        if (a.Cin % 28 == 0) return launch_tap48<28>(a, s);
    }
    // Deep K chunks (BK = 64) when K is long: a chunk's MFMAs (BK/2 x 64 cycles per wave tile) must cover
    // the global-load round trip of the next chunk, the only latency hiding a lone workgroup per CU has.
    const bool deep = a.K >= 192;
    if (a.Cout <= 32) return deep ? launch_cfg<128, 32, 4, 1, 64>(a, vec, s) : launch_cfg<128, 32, 4, 1, 16>(a, vec, s);
    if (a.M >= 16384) return deep ? launch_cfg<128, 64, 2, 2, 32>(a, vec, s) : launch_cfg<128, 64, 2, 2, 16>(a, vec, s);
    if (a.M >= 1024) return deep ? launch_cfg<64, 64, 2, 2, 64>(a, vec, s) : launch_cfg<64, 64, 2, 2, 16>(a, vec, s);
    return deep ? launch_cfg<32, 128, 1, 4, 64>(a, vec, s) : launch_cfg<32, 128, 1, 4, 16>(a, vec, s);
}

// ---- conv + pool in one launch ---------------------------------------------------------------------------------------------------
// The conditions under which trl_launch_conv above reaches conv_tap<128,64,2,2,32,false> or conv_tap48<28,false>, restated on
// shapes (the scratch is 256-byte aligned; trl_launch_conv_pool refuses a misaligned x), and the pools those have an epilogue for.
int trl_conv_pool_family(const ConvArgs& a, int pk, int pst) {
    if (a.M < 16384 || a.M > (1 << 30) || a.OH != a.OW || a.M != a.N * a.OH * a.OW || a.ph || a.pw || a.lowp) return 0;
    if (a.res || a.scale || a.act != TRL_ACT_PRELU) return 0;      // bias + PReLU only (conv_pool_assume)
    if (a.Cin % 4 || a.ldx % 4 || a.xoff % 4 || !trl_conv_small(a) || trl_fn_split4_rule(a)) return 0;
    if (!a.m_dev && a.M == 16384) return 0;                        // (may be the small-map family's)
    if (a.ldy != a.Cout || a.yoff) return 0;                       // the pooled map and the side buffer are dense
    if (!TailPool{a.OH, pk, pst, TRL_TAIL_POOL_BM}.ok()) return 0;
    const int flag = conv_pool_flag(a.OH, pk, pst);
    if (a.Cout == 48 && a.ldw >= 48 && a.Cin % 32 != 0 && a.Cin % 28 == 0) return flag == conv_pool_flag(9, 3, 2) ? TRL_FNK_TAP48 : 0;
    if (a.Cout == 64 && a.ldw >= 64 && a.K >= 192 && a.Cin % 32 == 0)
        return flag == conv_pool_flag(21, 3, 2) || flag == conv_pool_flag(8, 2, 2) ? TRL_FNK_CONV_TAP : 0;
    return 0;
}

int trl_launch_conv_pool(const ConvPoolArgs& a, hipStream_t s) {
    const int family = trl_conv_pool_family(a, a.pk, a.pst);
    const TailPool tp{a.OH, a.pk, a.pst, TRL_TAIL_POOL_BM};
    if (!family || !trl_conv_vec(a) || trl_fn_eligible(a) || (((uintptr_t)a.y | (uintptr_t)a.side) & 15) || (tp.can_straddle() && !a.side)) {
        trl_set_error("conv + pool launch on a layer without a pooling epilogue");
        return TRL_ERR_STATE;
    }
    const dim3 grid((a.M + 127) / 128, 1);
    const int flag = conv_pool_flag(a.OH, a.pk, a.pst);
    g_trl_conv_choice = TrlConvChoice{family, 128, family == TRL_FNK_TAP48 ? 48 : 64, family == TRL_FNK_TAP48 ? 28 : 32, 0, 1};
    if (family == TRL_FNK_TAP48) conv_tap48<28, false, conv_pool_flag(9, 3, 2)><<<grid, 256, 0, s>>>(a);
    else if (flag == conv_pool_flag(21, 3, 2)) conv_tap<128, 64, 2, 2, 32, false, conv_pool_flag(21, 3, 2)><<<grid, 256, 0, s>>>(a);
    else conv_tap<128, 64, 2, 2, 32, false, conv_pool_flag(8, 2, 2)><<<grid, 256, 0, s>>>(a);
    TRL_LAUNCH_CHECK();
    if (tp.can_straddle() && grid.x > 1) {
        pool_fixup_kernel<<<grid.x - 1, 128, 0, s>>>(a.y, a.side, a.ldy, a.yoff, a.Cout, tp, a.N, a.m_dev, a.m_base);
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

int trl_launch_maxpool(const float* x, int N, int H, int W, int C, int ldx, int xoff, int k, int st, int ceil_mode,
                       float* y, int ldy, int yoff, int OH, int OW, hipStream_t s, const int32_t* n_dev, int n_base) {
    (void)ceil_mode;
    const bool v4 = (C % 4 == 0) && (ldx % 4 == 0) && (xoff % 4 == 0) && (ldy % 4 == 0) && (yoff % 4 == 0) &&
                    (((uintptr_t)x & 15) == 0) && (((uintptr_t)y & 15) == 0);
    const size_t total = (size_t)N * OH * OW * (v4 ? C / 4 : C);
    if (total == 0) return TRL_OK;
    size_t blocks = (total + 255) / 256;
    if (blocks > 32768) blocks = 32768;
    if (v4) maxpool_kernel<4><<<(unsigned)blocks, 256, 0, s>>>(x, N, H, W, C, ldx, xoff, k, st, y, ldy, yoff, OH, OW, n_dev, n_base);
    else maxpool_kernel<1><<<(unsigned)blocks, 256, 0, s>>>(x, N, H, W, C, ldx, xoff, k, st, y, ldy, yoff, OH, OW, n_dev, n_base);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

int trl_launch_gap(const float* x, int N, int HW, int C, float* y, hipStream_t s) {
    if (N * C == 0) return TRL_OK;
    gap_kernel<<<(N * C + 255) / 256, 256, 0, s>>>(x, N, HW, C, y);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

int trl_launch_l2norm512(const float* x, const uint8_t* valid, int n, float* y, hipStream_t s) {
    if (n <= 0) return TRL_OK;
    l2norm512_kernel<<<n, 64, 0, s>>>(x, valid, n, y);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

int trl_launch_feat512(const float* x, const uint8_t* valid, int n, float* y, hipStream_t s) {
    if (n <= 0) return TRL_OK;
    feat512_kernel<<<n, 64, 0, s>>>(x, valid, n, y);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

int trl_launch_drift(const float* emb, const uint8_t* valid, int n, long long frame_count, int fps, float* sims,
                     uint8_t* flags, int32_t* result, hipStream_t s, void* state) {
    DriftState* st = (DriftState*)state;
    if (n > 0) {
        drift_sims_kernel<<<(n + 3) / 4, 256, 0, s>>>(emb, valid, n, sims, st);
        TRL_LAUNCH_CHECK();
    }
    drift_scan_kernel<<<1, 256, 0, s>>>(sims, n, frame_count, fps, flags, result, st, emb, valid);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

// trl_logits.hip -- InceptionResnetV1's classifier head: logits = feat @ W + b for n rows of 512 features against a
// [512][C] f32 weight matrix (vggface2: C = 8631, casia-webface: 10575; 17.7 / 21.7 MB).
//
// None of the conv launchers fits the shape: M is a handful of rows (a server) to a few thousand (the bench), N is ten thousand
// and no multiple of anything, and at small M the whole cost is one pass over the weights.  So:
//   * a workgroup owns a row tile of 32 faces and 128 classes; each of its 4 waves owns a SLAB of 32 classes and all 32 rows;
//   * the row tile's features sit in LDS ([32][514] words: the two pad words put the 64 lanes of an A-operand read -- row l & 31,
//     k = 2 s + (l >> 5) -- on 64 different banks), rows past n as zeros;
//   * a slab's weights never touch LDS: lane l reads w[2 s + (l >> 5)][c0 + (l & 31)], which IS the B operand of
//     v_mfma_f32_32x32x2_f32 -- one dword per lane, two whole 128-byte lines per wave instruction (the widest the [512][C]
//     layout allows a 32-class slab: its k-rows lie ld floats apart).  They stream through a three-deep register ring of 32
//     k-steps, so 64 loads (16 KB per wave) are in flight while 32 MFMAs issue;
//   * 256 MFMAs over ascending k on ONE accumulator seeded with the bias: per output the chain
//     acc = b[c]; for k = 0..511: acc = fmaf(feat[r][k], w[k][c], acc), whatever n, tile or slab;
//   * the epilogue stores rows < n and columns < C only (a register of the accumulator is 32 consecutive classes of one row).
// 65.8 KB of LDS and < 256 VGPRs: two workgroups per CU, one fills its tile while the other's chain runs.  The grid's fast
// index is the row tile, so the workgroups in flight share a few 128-class weight groups (L2) at large n.
// Up to 16 rows the same chain runs on v_mfma_f32_16x16x4_f32 instead (k_logits16 below): there only the chain's latency counts.
// Measured figures, the streaming and MFMA floors and the generic conv launcher on the same product: DESIGN.md section 7.
#include <utility>

#include "trl_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LG_K = 512;             // features per row
constexpr int LG_LDF = LG_K + 2;      // LDS row pitch in words
constexpr int LG_ROWS = 32;           // rows of a tile
constexpr int LG_CHUNK = 32;          // k-steps (of 2) per ring slot
constexpr int LG_NCHUNK = LG_K / 2 / LG_CHUNK;
constexpr int LG_LDS_BYTES = LG_ROWS * LG_LDF * 4;

template <int... I, typename F>
__device__ __forceinline__ void lg_static_for(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

__global__ __launch_bounds__(256) void k_logits(const float* __restrict__ feat, int n, const float* __restrict__ w, int ldw,
                                                const float* __restrict__ bias, int C, float* __restrict__ y, long long ld) {
    extern __shared__ float lg_feat[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * LG_ROWS;
    const int live = n - row0 < LG_ROWS ? n - row0 : LG_ROWS;
    // ---- the row tile -> LDS (float4 where the caller's pointer allows it) ----
    const float* src = feat + (size_t)row0 * LG_K;
    if ((reinterpret_cast<uintptr_t>(feat) & 15) == 0) {
#pragma unroll 4
        for (int t = tid; t < LG_ROWS * LG_K / 4; t += 256) {
            const int r = t >> 7, q = t & 127;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < live) v = *reinterpret_cast<const float4*>(src + (size_t)r * LG_K + 4 * q);
            float2* d = reinterpret_cast<float2*>(lg_feat + r * LG_LDF + 4 * q);   // (rows are 8-byte aligned: 514 words)
            d[0] = make_float2(v.x, v.y);
            d[1] = make_float2(v.z, v.w);
        }
    } else {
#pragma unroll 4
        for (int t = tid; t < LG_ROWS * LG_K; t += 256) {
            const int r = t >> 9, k = t & 511;
            lg_feat[r * LG_LDF + k] = r < live ? src[(size_t)r * LG_K + k] : 0.f;
        }
    }
    __syncthreads();
    const int c0 = (blockIdx.y * 4 + wave) * 32;
    if (c0 >= C) return;                                 // (behind the only barrier)
    const int j = lane & 31, h = lane >> 5;
    const float* wp = w + (size_t)h * ldw + c0 + j;      // in bounds: ld of the device matrix is C rounded up to 32, zero filled
    const float* xp = lg_feat + j * LG_LDF + h;
    const size_t step = (size_t)2 * ldw;
    float wb[3][LG_CHUNK], xa[2][LG_CHUNK];
    auto load_w = [&](int ch, float* o) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) o[u] = wp[(size_t)(ch * LG_CHUNK + u) * step];
    };
    auto load_x = [&](int ch, float* o) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) o[u] = xp[2 * (ch * LG_CHUNK + u)];
    };
    load_w(0, wb[0]);
    load_w(1, wb[1]);
    load_x(0, xa[0]);
    const float b = bias[c0 + j];                        // (vectors are padded to 128 floats)
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; q++) acc[q] = b;
    lg_static_for(std::make_integer_sequence<int, LG_NCHUNK>{}, [&](auto CH) __attribute__((always_inline)) {
        constexpr int ch = decltype(CH)::value;
        if constexpr (ch + 2 < LG_NCHUNK) load_w(ch + 2, wb[(ch + 2) % 3]);
        if constexpr (ch + 1 < LG_NCHUNK) load_x(ch + 1, xa[(ch + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[ch & 1][u], wb[ch % 3][u], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    });
    // C/D map of the 32x32 forms: column = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
    const int col = c0 + j;
    if (col < C) {
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = (q & 3) + 8 * (q >> 2) + 4 * h;
            if (r < live) y[(size_t)(row0 + r) * (size_t)ld + col] = acc[q];
        }
    }
}

// n <= 16 (a server's handful of faces): the same chain on v_mfma_f32_16x16x4_f32.  Nothing but the chain's own latency is left
// to shorten at such n -- 256 dependent 32x32x2 steps of 64 cycles are 6.8 us at 2.4 GHz, whatever the bandwidth -- and the
// 16x16x4 form walks the 512 k in 128 dependent steps of 40 cycles: 2.1 us.  A wave owns 16 classes and the 16 rows, a workgroup
// 64 classes (twice the workgroups, so the weight stream spreads over more CUs); lane l feeds A = feat[l & 15][4 s + (l >> 4)]
// from LDS ([16][516] words: 4 i + kk is a different bank for each lane) and B = w[4 s + (l >> 4)][c0 + (l & 15)] from global
// memory (four 64-byte pieces per wave instruction; the neighbouring wave reads the other half of each line).  Within one
// instruction the four k are taken in ascending order, as the two of the 32x32x2 form are (the PNet kernels rest on both).
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int LG16_ROWS = 16;
constexpr int LG16_LDF = LG_K + 4;
constexpr int LG16_NCHUNK = LG_K / 4 / LG_CHUNK;

__global__ __launch_bounds__(256) void k_logits16(const float* __restrict__ feat, int n, const float* __restrict__ w, int ldw,
                                                  const float* __restrict__ bias, int C, float* __restrict__ y, long long ld) {
    __shared__ float lg_feat[LG16_ROWS * LG16_LDF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 4
    for (int t = tid; t < LG16_ROWS * LG_K; t += 256) {
        const int r = t >> 9, k = t & 511;
        lg_feat[r * LG16_LDF + k] = r < n ? feat[(size_t)r * LG_K + k] : 0.f;
    }
    __syncthreads();
    const int c0 = (blockIdx.x * 4 + wave) * 16;
    if (c0 >= C) return;
    const int j = lane & 15, kk = lane >> 4;
    const float* wp = w + (size_t)kk * ldw + c0 + j;     // in bounds: c0 + 15 < C rounded up to 32 <= ldw
    const float* xp = lg_feat + j * LG16_LDF + kk;
    const size_t step = (size_t)4 * ldw;
    float wb[3][LG_CHUNK], xa[2][LG_CHUNK];
    auto load_w = [&](int ch, float* o) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) o[u] = wp[(size_t)(ch * LG_CHUNK + u) * step];
    };
    auto load_x = [&](int ch, float* o) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) o[u] = xp[4 * (ch * LG_CHUNK + u)];
    };
    load_w(0, wb[0]);
    load_w(1, wb[1]);
    load_x(0, xa[0]);
    const float b = bias[c0 + j];
    f32x4 acc = {b, b, b, b};
    lg_static_for(std::make_integer_sequence<int, LG16_NCHUNK>{}, [&](auto CH) __attribute__((always_inline)) {
        constexpr int ch = decltype(CH)::value;
        if constexpr (ch + 2 < LG16_NCHUNK) load_w(ch + 2, wb[(ch + 2) % 3]);
        if constexpr (ch + 1 < LG16_NCHUNK) load_x(ch + 1, xa[(ch + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < LG_CHUNK; u++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ch & 1][u], wb[ch % 3][u], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    });
    // C/D map of the 16x16 forms: column = lane & 15, row = 4 (lane >> 4) + q
    const int col = c0 + j;
    if (col < C) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = 4 * kk + q;
            if (r < n) y[(size_t)r * (size_t)ld + col] = acc[q];
        }
    }
}

}  // namespace

// w: the device matrix [512][ldw] of trl_load_weights (ldw >= C rounded up to 32, padding zero), bias padded likewise
int trl_launch_logits(const float* feat, int n, const float* w, int ldw, const float* bias, int C, float* y, long long ld, hipStream_t s) {
    if (n <= 0 || C <= 0) return TRL_OK;
    if (ldw < (C + 31) / 32 * 32 || ld < C) { trl_set_error("logits: bad leading dimension"); return TRL_ERR_INVALID; }
    if (n <= LG16_ROWS) {
        k_logits16<<<(unsigned)((C + 63) / 64), 256, 0, s>>>(feat, n, w, ldw, bias, C, y, ld);
        TRL_LAUNCH_CHECK();
        return TRL_OK;
    }
    TRL_HIP(hipFuncSetAttribute((const void*)k_logits, hipFuncAttributeMaxDynamicSharedMemorySize, LG_LDS_BYTES));   // above the default 64 KB
    const dim3 grid((unsigned)((n + LG_ROWS - 1) / LG_ROWS), (unsigned)((C + 127) / 128));
    k_logits<<<grid, 256, LG_LDS_BYTES, s>>>(feat, n, w, ldw, bias, C, y, ld);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

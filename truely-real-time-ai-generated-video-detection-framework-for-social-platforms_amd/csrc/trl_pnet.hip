// trl_pnet.hip -- MTCNN stage 1 (PNet over the image pyramid) for gfx950, the dominant kernel of the
// hot path (83 % of the conv FLOPs at 720p; server/model.py:47 -> detect_face stage 1).
//
// Per batch of frames: the image pyramid of every frame (trl_pyramid.hip: u8 BGR -> every level as three floats per pixel), then
// ONE fused launch over it.
//
//  k_pnet_fused   ONE persistent launch over all (frame, level, 16x16-cell tile) work items.  Per tile,
//                 entirely in LDS / registers:
//                   42x42x3 input tile -> conv1 3x3 (3->10) + 2x2 ceil max-pool + PReLU (the pool is an
//                   elementwise max over accumulators, or two DPP steps) -> conv2 3x3 (10->16) + PReLU
//                   -> conv3 3x3 (16->32) + PReLU -> 1x1 heads (32->2+4) -> softmax -> thr0 ->
//                   generateBoundingBox record appended to the (frame, level) candidate list.
//                 All four layers run on the f32 matrix cores -- the layers with few output channels (conv1: 10, heads: 6)
//                 on v_mfma_f32_4x4x1_16B_f32 with the weight block broadcast (no padding of N to 16), conv2 on
//                 v_mfma_f32_16x16x4_f32, conv3 on v_mfma_f32_32x32x2_f32 -- k ascending, accumulator seeded with the
//                 bias: the same fmaf chain as the oracle, so maps and candidates are bit-identical.  conv3 is first screened on
//                 v_mfma_f32_32x32x16_f16 with a rigorous error bound: only the M-tiles that may hold a candidate take the f32 chain.
//                 conv1 / conv2 / head weights live in registers for the whole launch (6+23+4 VGPRs per lane),
//                 conv3's in LDS; activations never leave the CU: HBM traffic is the pyramid read only.  f32 MFMA and VALU share the FP32 pipe, so the loops carry almost no VALU: the
//                 tile decode is scalar (multiply-high by host magic numbers), LDS addresses are lane bases +
//                 compile-time offsets, pooling precedes PReLU when the slopes allow, edge logic only on edge tiles.
//                 blockIdx -> tile mapping keeps an XCD on a contiguous run of tiles (halo rows of
//                 neighbouring tiles hit the same L2).
//  k_pnet_confirm The few conv3 M-tiles (32 cells) the screen confirms are not run inside the persistent kernel, where one wave's exact
//                 chain keeps the other three of its workgroup at the tile's last barrier: the DEFER instantiation queues them (the
//                 M-tile's conv2 rows, 4.9 KB) and this ordinary kernel, launched right behind it, runs the same chain on every queued
//                 M-tile, one wave each.  The queue is a block of the cascade workspace with a capacity that follows the content
//                 (trl_capacity.h); launches that cannot defer, and content that confirms most M-tiles, run the chain inline.
#include "trl_pyramid.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TS = 16;            // output cells per tile side
constexpr int IN_T = 2 * TS + 10; // 42 input pixels
constexpr int P1_T = TS + 4;      // 20 pooled cells
constexpr int C2_T = TS + 2;      // 18 conv2 cells
constexpr int C2_LD = 17;         // padded channel stride of the conv2 tile (bank spread for conv3 reads)
constexpr int REGION_A = C2_T * C2_T * C2_LD;        // 5508 floats: input tile, later conv2 output
constexpr int REGION_B = P1_T * P1_T * 10 + 224;     // 4000 floats of pooled conv1 + the reach of conv2's zero-weight k padding (k = 90, 91 of the last cells: finite, zeroed once)
static_assert(3 * 7 * 256 <= REGION_A, "input tile (+ the 28 overhang pixels of the 7x256 copy) fits region A");
static_assert(P1_T * P1_T * 10 <= REGION_B, "pooled tile fits region B");
// Phase 3 reuses region B (dead between conv2 and the next tile's conv1) for the fp16 screen's activation operands: the conv2 tile
// in fp16 as [half of the channels][324 cells][8] (16 bytes per item: one aligned ds_read_b128 per tap), then the error weight
// m = sum of g[channel] |x| of every item as [2][324] floats, from float offset SCR_XM.
constexpr int SCR_XM = 2 * C2_T * C2_T * 4;          // 2592 floats of fp16 tile in front of the error weights
// Horizontal carry between consecutive tiles of a tile row (a workgroup takes RUNS of consecutive tiles): the right-most 4 pooled
// columns and 2 conv2 columns of tile (ty, tx) ARE the left-most ones of tile (ty, tx + 1) -- the halo that 16x16-cell tiles
// otherwise compute twice (conv1 x1.56, conv2 x1.27 of the useful work).  They are kept in LDS across the tile boundary, and a tile
// that follows its left neighbour computes only 16 new pooled columns (80 instead of 100 conv1 M-tiles) and 16 new conv2 columns
// (18 instead of 21 M-tiles).  Same values: every cell is the same fmaf chain over the same pixels whichever tile computes it.
constexpr int CARRY_P = P1_T * 4 * 10;               // 800 floats: pooled rows x 4 columns x 10 channels
constexpr int CARRY_C = C2_T * 2 * C2_LD;            // 612 floats: conv2 rows x 2 columns x 17 (padded channels)
// Vertical carry (round 3): the tiles of a level are walked in BANDS of BAND tile rows, column by column (top tile, the tiles below
// it, then the next column), so a lower tile follows its upper neighbour in the same workgroup: ITS first 4 pooled rows and
// 2 conv2 rows are the upper tile's last ones.  A tile with both carries computes 16 x 16 new pooled cells (one super unit per
// wave and nothing else) and 16 x 16 new conv2 cells (16 M-tiles, four per wave).  The horizontal strips need one slot per band row:
// three rows (two of three tiles carry vertically) fill the 80 KB a workgroup may use at two workgroups per CU; two rows were 1.5 %
// slower, four do not fit.
constexpr int BAND = 3;
constexpr int VCARRY_P = 4 * P1_T * 10;              // 800 floats: 4 pooled rows x 20 columns x 10 channels (contiguous in the tile)
constexpr int VCARRY_C = 2 * C2_T * C2_LD;           // 612 floats: 2 conv2 rows x 18 columns x 17
constexpr int DYN_LDS = (144 * 32 + BAND * (CARRY_P + CARRY_C) + VCARRY_P + VCARRY_C) * 4;   // conv3 weights + the carry strips (dynamic: static LDS is capped at 64 KB)
static_assert((2 * C2_T * C2_LD * 4) % 16 == 0 && 4 * C2_T * C2_LD * 4 == TRL_DEFER_BLOCK, "an M-tile's 4 conv2 rows: 16-byte words of region A, one queue block");
static_assert((144 * 32) % 4 == 0 && CARRY_P % 4 == 0 && CARRY_C % 4 == 0 && VCARRY_P % 4 == 0, "strips stay 16-byte aligned");

// A level as k_pnet_fused reads it.  The kernel indexes lv[] by sizeof(PLevel) and loads its members by their offsets, so both are
// pinned: the words `kept*` (and PnetArgs::kept) are where members of the pyramid kernels lay before those moved to trl_pyramid.hip;
// nothing writes or reads them, and taking them out would change the fused kernel's code.
struct PLevel {
    int h, w, oh, ow;        // level size, PNet map size
    int tiles_x, tile0;      // tiles per row, first tile index of the level inside a frame
    int tiles_y;             // tile rows
    unsigned bmagic;         // ceil(2^32 / (BAND * tiles_x)): band of a tile index
    int pix0;                // pixel offset of the level inside a frame's pyramid
    int kept0[9];
    unsigned txmagic;        // ceil(2^32 / tiles_x): tile decode stays on the scalar unit
    int kept1[19];
    float scale;
    int cap, rec0;           // candidate records of the level: slots per frame, first slot inside a frame's block (LvLayout)
};
static_assert(sizeof(PLevel) == 164 && offsetof(PLevel, txmagic) == 72 && offsetof(PLevel, scale) == 152, "k_pnet_fused's argument layout");
struct PnetArgs {
    const PyrPx* pyr; long long pyr_stride;    // pixels per frame
    int n_frames, L, tiles_per_frame, H, W;
    unsigned tpf_magic;                        // ceil(2^32 / tiles_per_frame)
    long long kept;
    PLevel lv[16];
    const float *w1, *w2, *w3, *wh;            // [Kpad][32] zero padded
    const float *b1, *b2, *b3, *bh, *s1, *s2, *s3;
    float thr; int rec_stride;                 // record slots per frame (LvLayout::S)
    float dthr;                                // logit-difference prefilter: no cell with logit1 - logit0 < dthr can reach thr (-inf: off)
    float scrB; int screen;                    // fp16 conv3 screen: |d_screen - d_exact| <= sum over the cell's 3x3x16 inputs of scrG[channel] |x| + scrB
    float scrG[16];                            // (screen = 0: every M-tile exact)
    int dbg_skip;                              // timing-only ablation mask (TRL_PNET_SKIP); read by the DBG instantiation only
    int32_t* lvl_cnt; Cand* lvl_rec; int32_t* flags;
    int32_t* xcd_next;                         // per-XCD dynamic tile cursor (8 counters, zeroed before the launch)
    int run;                                   // consecutive tiles a workgroup takes per cursor fetch (>= 1)
    unsigned long long* clk;                   // the CLK_* words (trl_ctx.h): CLK_START = earliest workgroup start, CLK_END = latest workgroup end (device wall clock); DBG: the phase clocks
    int prof;                                  // DBG instantiation: accumulate the per-phase wave clocks
    char* q; int q_cap; int32_t* q_cnt;        // DEFER: the confirm queue (q_cap slots of TRL_DEFER_SLOT bytes) and its slot counter (zeroed with xcd_next)
};

// ---- fused PNet --------------------------------------------------------------------------------------

// A-operand k offsets.  k = 4s+kq walks (tap, channel) of a [pixel][C] LDS tile whose rows are E floats
// further apart than D consecutive k: offset = k + E*(k/D).  With s a compile-time constant only the step
// whose four k straddle a multiple of D depends on the lane (kq >= thr), so no per-lane offset tables.
template <int D, int E>
__device__ __forceinline__ int koff(int s, int kq, int e1, int e2, int e3) {
    const int q0 = (4 * s) / D, r0 = (4 * s) % D, thr = D - r0;    // folded after unrolling
    const int add = thr == 1 ? e1 : (thr == 2 ? e2 : (thr == 3 ? e3 : 0));
    return 4 * s + E * q0 + kq + add;
}

// UNIT: no PReLU slope of the net exceeds 1 (negative slopes included); then prelu(v) == max(v, slope*v) exactly (trl_common.h).
// Weights with a slope above 1 (a trained checkpoint's are unconstrained) take the general instantiation, which costs the same
// two VALU instructions per value: med3(v, slope*v, +-inf) (trl_prelu_med3).  Both pool conv1 BEFORE its PReLU -- with the
// window's min next to its max when a conv1 slope is negative (the NEG1 instantiations, trl_prelu_pooled).
template <bool UNIT>
__device__ __forceinline__ float prelu_t(float v, float sl, float sel) { return UNIT ? vmax_nc(v, sl * v) : trl_prelu_med3(v, sl, sel); }
template <bool UNIT>
__device__ __forceinline__ float prelu_pooled_t(float m, float n, float sl, float sel) {
    return UNIT ? vmax_nc(m, sl * (sl < 0.f ? n : m)) : trl_prelu_pooled(m, n, sl, sel);
}

// ---- conv1 on v_mfma_f32_4x4x1_16B_f32 -----------------------------------------------------------------------------------------
// 16x16x4 tiles pad conv1's N = 10 to 16 (and K = 27 to 28): 40 % of their issue cycles multiply zeros.  The 4x4x1 block
// instruction computes sixteen independent 4x4 outer-product blocks, ONE k per instruction, and can broadcast block `abid` of the A
// register to all sixteen (cbsz = 4).  A UNIT = 16 pool cells x their 4 conv1 positions: block b = cell, lane-in-block j = position
// (dy, dx); the B operand is the lane's pixel value at k; the A operand is W[k][4 cg + i] for one of three channel groups, broadcast
// from block k & 15 of register k >> 4 -- the whole 27 x 12 weight matrix (+ the bias as a 28th "k" against a constant 1) lives in
// 6 VGPRs.  84 instructions x 8 cycles per 64 pixels instead of 4 x 7 x 32: -25 % issue cycles; the chain per output is still
// acc = bias, k ascending (fma(bias, 1, 0) == bias exactly).  The 2x2 pool window of a cell is the block's four lanes: two DPP max.
template <int CB, int AB>
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, CB, AB, 0); }
// max / min over the four lanes of each quad, four values at a time; one asm block per group so that no DPP instruction reads a
// register written by one of the two instructions in front of it (gfx9 DPP hazard) whatever the scheduler does around the block
__device__ __forceinline__ void quad_max4(const f32x4& v, float (&o)[4]) {
    float t0, t1, t2, t3;
    asm("v_max_f32_dpp %4, %8, %8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %5, %9, %9 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %6, %10, %10 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %7, %11, %11 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %0, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %1, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %2, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_max_f32_dpp %3, %7, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
}
__device__ __forceinline__ void quad_min4(const f32x4& v, float (&o)[4]) {
    float t0, t1, t2, t3;
    asm("v_min_f32_dpp %4, %8, %8 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %5, %9, %9 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %6, %10, %10 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %7, %11, %11 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %0, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %1, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %2, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_min_f32_dpp %3, %7, %7 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
        : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]));
}
// per-lane select on a wave-uniform 64-bit lane mask (one v_cndmask: hipcc turned the ?: on lane-index tests into exec-mask branches)
__device__ __forceinline__ float lane_sel(float if0, float if1, unsigned long long mask) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if0), "v"(if1), "s"(mask));
    return r;
}
template <int... I, typename F>
__device__ __forceinline__ void pn_static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }

// ---- conv3 -> heads -> candidates of ONE M-tile (32 cells = 2 output rows), register to register ---------------------------------
// Written once for the two places that run them: phase 3 of k_pnet_fused (the inline instantiations: the M-tile of the conv2 tile
// in region A) and k_pnet_confirm (the M-tile's 4 conv2 rows in a wave's own LDS area, laid out like region A's rows: mt = 0).
//
// conv3 runs TRANSPOSED on mfma_f32_32x32x2: the A operand is the weight (rows = output channels), the B operand the
// activation (columns = the 32 cells of the M-tile = 2 output rows), the same two LDS words per lane and k-step as the
// other way round and the same chain per output (acc = bias, k ascending).  Lane l then holds 16 channels --
// 8 (q >> 2) + (q & 3) + 4 hh -- of ONE cell (l & 31): exactly what the heads' B operand wants, so nothing is staged
// through LDS between conv3 and the heads (round 3 measured that round trip and the idle chain behind it at 6 % of the
// kernel).  `between(sx, u)` is called after MFMA u of sixth sx: the previous M-tile's head chain rides in those slots.
// R: conv2 rows [.][18][17], B3S: the conv3 weights [k][32], T3: bias[32], slopes[32], head bias[8] as f32x4 (all LDS).
template <bool UNIT, typename Between>
__device__ __forceinline__ void pn_conv3(const float* R, const float* B3S, const f32x4* T3, int mt, int l31, int hh, f32x16& P, Between&& between) {
    const int y = mt * 2 + (l31 >> 4), x = l31 & 15;
    const int base = (y * C2_T + x) * C2_LD + hh;
    f32x16 acc;
#pragma unroll
    for (int qa = 0; qa < 4; qa++) {
        const f32x4 b4 = T3[2 * qa + hh];                       // bias of channels 8 qa + 4 hh .. + 3
        acc[4 * qa] = b4[0]; acc[4 * qa + 1] = b4[1]; acc[4 * qa + 2] = b4[2]; acc[4 * qa + 3] = b4[3];
    }
    // 6 x 12 k-steps, double buffered: the operands of sixth i+1 are requested before the MFMAs of sixth i
    // issue, so only the first sixth's LDS latency is exposed.
    float xa[2][12], wb[2][12];
    auto read_sixth = [&](int sx, float* xo, float* wo) {
#pragma unroll
        for (int u = 0; u < 12; u++) {
            const int s = sx * 12 + u, tap = s >> 3, ky = tap / 3, kx = tap - ky * 3;
            xo[u] = R[base + (ky * C2_T + kx) * C2_LD + 2 * (s & 7)];
            wo[u] = B3S[(2 * s + hh) * 32 + l31];
        }
    };
    read_sixth(0, xa[0], wb[0]);
    pn_static_for(std::make_integer_sequence<int, 6>{}, [&](auto SX) __attribute__((always_inline)) {
        constexpr int sx = decltype(SX)::value;
        if (sx < 5) read_sixth(sx + 1, xa[(sx + 1) & 1], wb[(sx + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        pn_static_for(std::make_integer_sequence<int, 12>{}, [&](auto UU) __attribute__((always_inline)) {
            constexpr int u = decltype(UU)::value;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[sx & 1][u], xa[sx & 1][u], acc, 0, 0, 0);
            between(SX, UU);
        });
        __builtin_amdgcn_sched_barrier(0);
    });
#pragma unroll
    for (int qa = 0; qa < 4; qa++) {
        const f32x4 s4 = T3[8 + 2 * qa + hh];                   // PReLU slopes of the same channels
#pragma unroll
        for (int qb = 0; qb < 4; qb++) P[4 * qa + qb] = prelu_t<UNIT>(acc[4 * qa + qb], s4[qb], UNIT ? 0.f : trl_prelu_sel(s4[qb]));
    }
}
// heads (1x1, 32 -> 2 + 4) on v_mfma_f32_4x4x1_16B_f32: sixteen 4x4 blocks per instruction, ONE k per instruction.
// Block b of lanes 4b..4b+3 = cells 4(b & 7) .. +3 (the B operand: the cell's conv3 value at k), outputs
// 4(b >> 3) .. +3 (the A operand: weights W[k][4(b >> 3) + i], broadcast inside each group of eight blocks from block
// k & 7 of register k >> 3 -- cbsz = 3, abid = k & 7): one instruction does both output groups of all 32 cells and
// every lane ends up holding ITS cell's logits.  Same chain: acc = bias, k ascending.  Channel k of cell c sits in
// lane c + 32 ((k >> 2) & 1), register 4 (k >> 3) + (k & 3): one v_permlane32_swap of the register with a copy of
// itself yields the lower half's value in every lane (k & 4 == 0) and the upper half's (k & 4 == 4).
struct PnHeads {
    float WH[4];                 // the lane's head weights: load()
    unsigned hlo[4], hhi[4];     // the swapped registers of the current group of eight k
    __device__ __forceinline__ void load(const float* wh, int lane) {
#pragma unroll
        for (int r = 0; r < 4; r++) WH[r] = wh[(((lane >> 2) & 7) + 8 * r) * 32 + 4 * (lane >> 5) + (lane & 3)];
    }
    template <int k>
    __device__ __forceinline__ void step(const f32x16& P, f32x4& hq) {
        constexpr int ga = k >> 3, gb = k & 7;
        if constexpr (gb == 0) {
#pragma unroll
            for (int qb = 0; qb < 4; qb++) {
                const unsigned v = __float_as_uint(P[4 * ga + qb]);
                const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                hlo[qb] = r[0]; hhi[qb] = r[1];
            }
        }
        const float bk = __uint_as_float(gb < 4 ? hlo[gb & 3] : hhi[gb & 3]);
        hq = __builtin_amdgcn_mfma_f32_4x4x1f32(WH[ga], bk, hq, 3, gb, 0);
    }
    __device__ __forceinline__ void all(const f32x16& P, f32x4& hq) {
        pn_static_for(std::make_integer_sequence<int, 32>{}, [&](auto H_T) __attribute__((always_inline)) { step<decltype(H_T)::value>(P, hq); });
    }
};
// lanes 0..31: {logit0, logit1, reg0, reg1} of cell = lane; lanes 32..63: {reg2, reg3, -, -} of cell = lane - 32
// The softmax (two exps and a division: ~55 VALU beside the other workgroup's MFMAs) runs only for an M-tile in which
// some cell's logit difference comes within reach of the threshold (a.dthr: a bound with a wide margin, fill_args) --
// one compare and a scalar branch for the ~90 % of the M-tiles that hold no candidate.
// (f, l): frame and level; (oy0, ox0): the M-tile's first output cell in the level's map of oh x ow cells; fscale: the level's scale
__device__ __forceinline__ void pn_emit(const PnetArgs& a, int f, int l, int oy0, int ox0, int oh, int ow, float fscale, int dbg_skip, int lane,
                                        const f32x4& hq) {
    if (__builtin_amdgcn_ballot_w64(lane < 32 && hq[1] - hq[0] >= a.dthr) == 0) return;
    const float p = trl_softmax2_p1(hq[0], hq[1]);
    const auto u2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(hq[0]), __float_as_uint(hq[0]), false, false);
    const auto u3 = __builtin_amdgcn_permlane32_swap(__float_as_uint(hq[1]), __float_as_uint(hq[1]), false, false);
    if (lane < 32) {                                // one lane per cell of the 32-row tile
        const int oy = oy0 + (lane >> 4), ox = ox0 + (lane & 15);
        if (oy < oh && ox < ow) {
            if (p >= a.thr && !(dbg_skip & 32)) {      // (bit 32: timing-only ablations emit no candidates)
                const int seg = f * a.L + l;
                const int sl = atomicAdd(&a.lvl_cnt[seg], 1);
                if (sl < a.lv[l].cap) {            // (scalar loads inside the rare branch: the tile descriptor stays as small as it was)
                    Cand c;
                    c.x1 = floorf((2.f * (float)ox + 1.f) / fscale);
                    c.y1 = floorf((2.f * (float)oy + 1.f) / fscale);
                    c.x2 = floorf((2.f * (float)ox + 12.f) / fscale);
                    c.y2 = floorf((2.f * (float)oy + 12.f) / fscale);
                    c.score = p;
                    c.r0 = hq[2]; c.r1 = hq[3]; c.r2 = __uint_as_float(u2[1]); c.r3 = __uint_as_float(u3[1]);
                    c.cell = oy * ow + ox;
                    a.lvl_rec[(size_t)f * a.rec_stride + a.lv[l].rec0 + sl] = c;
                } else {
                    a.flags[FLG_LEVEL] = 1;
                }
            }
        }
    }
}

// DBG: diagnostic instantiation -- records the launch's execution span on the device wall clock (TRL_PNET_CLOCK=1) and honours
// the timing-only phase ablation mask (TRL_PNET_SKIP, tools/pnet_phase_pmc.sh).  The production instantiation (DBG = false)
// carries neither: no instrumentation and no ablation tests on the hot path.
// DEFER: an M-tile the screen confirms is not run here: the wave takes a slot of the confirm queue and copies what the exact chain
// reads -- the M-tile's 4 conv2 rows, 72 consecutive cells of region A -- into it; k_pnet_confirm, launched behind this kernel,
// runs conv3, the heads and the candidate write of every queued M-tile, one wave each and no barrier between them.  The
// instantiation holds no conv3, no head chain and no candidate write.
template <bool UNIT, bool NEG1, bool DBG, bool DEFER>
__global__ __launch_bounds__(256, 2) void k_pnet_fused(PnetArgs a) {
    __shared__ __attribute__((aligned(16))) float RA[REGION_A];   // input tile [42][42][3]  ->  conv2 out [324][17]
    __shared__ __attribute__((aligned(16))) float RB[REGION_B];   // pooled [400][10] (+ the reach of conv2's zero-weight k padding)
    __shared__ __attribute__((aligned(16))) float T3all[108];     // conv3 bias[32], PReLU slopes[32] (a lane's 16 channels differ per register), head bias[8],
                                                                  // screen: logit-difference weights f32(w1 - w0)[32], bias f32(b1 - b0) (phase 3)
    extern __shared__ __attribute__((aligned(16))) float DYN[];  // DYN_LDS bytes
    float* const B3S = DYN;                                       // conv3 weights [k][cout]: read per k-chain batch, not held in VGPRs
    float* const CP0 = DYN + 144 * 32;                            // per band row: carried pooled columns [20][4][10], conv2 columns [18][2][17]
    float* const VP = CP0 + BAND * (CARRY_P + CARRY_C);           // carried pooled rows [4][20][10]
    float* const VC = VP + VCARRY_P;                              // carried conv2 rows  [2][18][17]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: every M-tile index below is SALU work
    const int dbg_skip = DBG ? a.dbg_skip : 0;                   // a compile-time 0 in production
    if (DBG && tid == 0) atomicMin(&a.clk[CLK_START], (unsigned long long)wall_clock64());   // tuning build: execution span of the launch (first workgroup start .. last workgroup end)
    const int l15 = lane & 15, kq = lane >> 4;      // 16x16x4 operand coordinates
    const int l31 = lane & 31, hh = lane >> 5;      // 32x32x2 operand coordinates

    // ---- B operands: every weight matrix stays in registers for the whole launch -----------------------------
    for (int i = tid; i < 144 * 32; i += 256) B3S[i] = a.w3[i];          // conv3 B operand [k][32] in LDS (18 KB)
    float B2[23];
#pragma unroll
    for (int s = 0; s < 23; s++) B2[s] = a.w2[(4 * s + kq) * 32 + l15];
    PnHeads hd;
    if constexpr (!DEFER) hd.load(a.wh, lane);                            // heads: see phase 3
    // (vectors are zero padded to 128 floats)
    const float bias2 = a.b2[l15], slope2 = a.s2[l15];
    if (tid < 32) { T3all[tid] = a.b3[tid]; T3all[32 + tid] = a.s3[tid]; if (tid < 8) T3all[64 + tid] = a.bh[tid]; }   // (published by the barrier below)
    if (tid < 32) { T3all[72 + tid] = a.wh[tid * 32 + 1] - a.wh[tid * 32]; if (tid == 0) T3all[104] = a.bh[1] - a.bh[0]; }
    // general instantiation only: the per-channel med3 selector (+inf: max(v, s v), -inf: min(v, s v)); dead code when UNIT
    const float sel2 = trl_prelu_sel(slope2);
    const f32x4 bias2v = {bias2, bias2, bias2, bias2};

    // LDS beyond the live tiles is read by zero-weight k padding: it must hold finite values
    for (int i = tid; i < REGION_A; i += 256) RA[i] = 0.f;
    for (int i = tid; i < REGION_B; i += 256) RB[i] = 0.f;
    __syncthreads();

    const int e2_2 = kq >= 2 ? 170 : 0;                                                      // conv2: D = 30, E = 200-30
    // conv1 on 4x4x1 blocks: block xb = pool cell of the unit, xj = (dy, dx); weights + bias of channel group cg packed 16 k per register
    const int xb = lane >> 2, xj = lane & 3, xdy = xj >> 1, xdx = xj & 1;
    float WC[3][2];
#pragma unroll
    for (int cg = 0; cg < 3; cg++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = xb + 16 * h;
            WC[cg][h] = k < 27 ? a.w1[k * 32 + 4 * cg + xj] : (k == 27 ? a.b1[4 * cg + xj] : 0.f);
        }
    float xone = 1.0f;
    asm volatile("" : "+v"(xone));                        // a VGPR holding 1.0 (the bias "k"): not re-materialised per use
    const int xcg = xj < 3 ? xj : 2;                      // lane j < 3 finishes channel group j of its cell (lane 3 idles in the epilogue)
    const float sl4[4] = {a.s1[4 * xcg], a.s1[4 * xcg + 1], a.s1[4 * xcg + 2], a.s1[4 * xcg + 3]};
    // wide unit of pooled row wave + 4 i, columns 4..19: input lane base and store base (+ immediates per i)
    const int c1x_w = ((2 * wave + xdy) * IN_T + 8 + 2 * xb + xdx) * 3;
    const int c1x_sw = (wave * P1_T + 4 + xb) * 10 + 4 * xj;
    // SUPER unit: the 64 cells (row wave + 4 j, column 4 + xb), ONE conv1 position per pass: the pool window is then four
    // accumulators of the SAME lane (no cross-lane step), and every lane finishes its own cell
    const int c1s_l = ((2 * wave + 8 * xj) * IN_T + 8 + 2 * xb) * 3;
    const int c1s_s = ((wave + 4 * xj) * P1_T + 4 + xb) * 10;

    const int total_tiles = a.tiles_per_frame * a.n_frames;
    // XCD-aware persistent schedule: blocks sharing blockIdx%8 (one XCD) walk one contiguous 1/8 of the tiles
    const int xcd = blockIdx.x & 7;
    const int chunk = (total_tiles + 7) / 8;
    const int t_begin = xcd * chunk, t_end = (t_begin + chunk < total_tiles) ? t_begin + chunk : total_tiles;

    // tile -> (frame, level, ty, tx), all on the scalar unit: divisions are multiply-high by host magic numbers
    // (an integer division would expand into a VALU float-reciprocal sequence, paid in MFMA issue slots), the
    // level is a branch-free count over a first-tile table held in SGPRs.
    // the level of a tile index: lane i holds the first tile of level i (lanes past the last level: INT_MAX), so the level is one
    // compare and a ballot count -- sixteen thresholds in SGPRs pushed other uniform values into VGPRs and the whole decode onto the
    // vector unit (84 VALU per tile beside the other workgroup's MFMAs)
    const int lvl_t0v = lane < a.L ? a.lv[lane < 16 ? lane : 15].tile0 : 0x7fffffff;
    auto sdiv = [](int n, unsigned magic, int d) {
        int q = (int)__umulhi((unsigned)n, magic);
        if (q * d > n) q--;
        if (n - q * d >= d) q++;
        return q;
    };
    // A decoded tile carries the fields of its level that the loop reads: they are fetched HERE (scalar loads from the argument
    // block, issued while the previous tile is in phase 3), not at the top of the tile's own iteration -- left to itself hipcc
    // indexed a.lv[] with a VGPR and put a vector-memory round trip (~1,100 clocks per tile, measured with TRL_PNET_CLOCK) in
    // front of phase 0.
    struct TileId { int f, l, ty, tx, h, w, oh, ow, tiles_x, pix0, rib, rows; float scale; };   // rib: row inside the band, rows: tile rows of the band
    auto decode = [&](int tile) {
        TileId t;
        // (readfirstlane: at the SGPR limit hipcc parks uniform values in VGPRs, and everything computed from one runs on the vector
        // unit -- 84 VALU per tile for this decode; pinned to SGPRs here, it is scalar work again)
        const int tpf = __builtin_amdgcn_readfirstlane(a.tiles_per_frame);
        t.f = __builtin_amdgcn_readfirstlane(sdiv(tile, __builtin_amdgcn_readfirstlane(a.tpf_magic), tpf));
        const int tt = tile - t.f * tpf;
        t.l = __popcll(__ballot(tt >= lvl_t0v)) - 1;
        const PLevel& g = a.lv[t.l];
        t.h = g.h; t.w = g.w; t.oh = g.oh; t.ow = g.ow; t.tiles_x = g.tiles_x; t.pix0 = g.pix0; t.scale = g.scale;
        // band order: index inside the level -> (band, column, row inside the band); the last band of a level may be one row high
        const int tq = tt - g.tile0;
        const int band = sdiv(tq, g.bmagic, BAND * t.tiles_x);
        const int rb = tq - band * (BAND * t.tiles_x);
        t.rows = g.tiles_y - BAND * band < BAND ? g.tiles_y - BAND * band : BAND;
        static_assert(BAND == 2 || BAND == 3, "column of a band position: rb / rows for rows in 1..3");
        t.tx = __builtin_amdgcn_readfirstlane(t.rows == 3 ? (rb * 43691) >> 17 : (t.rows == 2 ? rb >> 1 : rb));   // (rb < 98304)
        t.rib = rb - t.tx * t.rows;
        t.ty = BAND * band + t.rib;
        return t;
    };
    // The next tile's 42x42 input pixels are fetched into registers while the current tile is in phase 3
    // (7 float4 per thread) and dropped into LDS at the top of the next iteration: the HBM/L2 latency of the
    // only global read of the kernel is off the critical path.  Thread t owns pixels p = t + 256 i; since
    // 256 = 6*42 + 4, (iy, ix) of pixel i follow from (iy0, ix0) with one conditional wrap, and the address is
    // a scalar tile base plus a 32-bit lane offset.  Interior tiles (the bulk) load without bounds tests.
    const int pin_iy0 = tid / IN_T, pin_ix0 = tid - pin_iy0 * IN_T;
    int ctid = tid;          // the thread index, laundered once per tile (see the strip copies below)
    float4 pre[7];
    auto issue_input = [&](const TileId& t) {
        const TileId& g = t;
        const int gy0 = t.ty * 2 * TS, gx0 = t.tx * 2 * TS;
        const char* srcb = reinterpret_cast<const char*>(a.pyr + (long long)t.f * a.pyr_stride + g.pix0 + (long long)gy0 * g.w + gx0);
        const int w16 = g.w * 12;                  // bytes per pyramid row (12 B pixels)
        const int hrem = g.h - gy0, wrem = g.w - gx0;
        // (the thread's first pixel laundered per call: hoisted out of the tile loop, the per-pixel rows, columns and wrap masks
        // derived from it stay in ~20 VGPRs and 14 SGPRs for the whole launch, at the register limit; recomputed, they are a
        // handful of VALU per tile)
        int iy0 = pin_iy0, ix0 = pin_ix0;
        asm volatile("" : "+v"(iy0), "+v"(ix0));
        if (hrem >= IN_T && wrem >= IN_T) {
            const unsigned v0 = (unsigned)(iy0 * w16 + ix0 * 12);
#pragma unroll
            for (int i = 0; i < 7; i++) {
                unsigned vo = v0 + (unsigned)(i * (6 * w16 + 48)) + ((ix0 >= IN_T - 4 * i) ? (unsigned)(w16 - IN_T * 12) : 0u);
                if (i == 6) vo = (ctid < IN_T * IN_T - 6 * 256) ? vo : 0u;     // p >= 42*42: reload pixel 0 (lands in the RA tail)
                { const f32x3_nt v3 = *reinterpret_cast<const f32x3_nt*>(srcb + vo); pre[i] = make_float4(v3[0], v3[1], v3[2], 0.f); }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 7; i++) {
                const bool wrap = ix0 >= IN_T - 4 * i;
                const int iy = iy0 + 6 * i + (wrap ? 1 : 0), ix = ix0 + 4 * i - (wrap ? IN_T : 0);
                const bool ok = iy < hrem && ix < wrem && (i < 6 || ctid < IN_T * IN_T - 6 * 256);
                pre[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) { const f32x3_nt v3 = *reinterpret_cast<const f32x3_nt*>(srcb + (unsigned)(iy * w16 + ix * 12)); pre[i] = make_float4(v3[0], v3[1], v3[2], 0.f); }
            }
        }
    };
    // Carry strips <-> tiles, a handful of instructions per tile (VALU beside the MFMAs is paid in matrix throughput): the pooled
    // strip is 20 rows x 40 floats = 10 float4 per row (16 threads per row, 10 active: rows 0..15 in one pass, 16..19 in a second);
    // the conv2 strip is 18 rows x 34 floats = 17 float2 per row (32 threads per row, 17 active: three passes).  (Splitting the
    // copies -- reads at the top of a phase, writes at its end -- hides their LDS round trips but holds ~20 registers across the
    // phases: the kernel then spills ~25 lane constants to scratch and loses 5 %: measured, reverted.)
    typedef float f32x2c __attribute__((ext_vector_type(2)));
    // (the copies index with `ctid`, the thread index laundered once per tile: their ~12 lane addresses are then recomputed, one VALU
    // each, instead of hoisted out of the tile loop and -- at 256 VGPRs -- spilled; a scratch reload waits on vmcnt(0), i.e. on
    // the next tile's input loads that are in flight for exactly that reason)
    auto copy_pooled = [&](auto SAVE_T, float* CP) {
        constexpr bool SAVE = decltype(SAVE_T)::value;          // tile -> strip (columns 16..19), or strip -> tile (columns 0..3)
        const int q = ctid & 15;
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            const int r = (ctid >> 4) + 16 * pass;
            if (q < 10 && (pass == 0 || ctid < 64)) {
                f32x4* t = reinterpret_cast<f32x4*>(RB + r * (P1_T * 10) + (SAVE ? 16 * 10 : 0) + 4 * q);
                f32x4* c = reinterpret_cast<f32x4*>(CP + r * 40 + 4 * q);
                if (SAVE) *c = *t; else *t = *c;
            }
        }
    };
    auto copy_conv2 = [&](auto SAVE_T, float* CC) {
        constexpr bool SAVE = decltype(SAVE_T)::value;          // columns 16..17 -> strip, or strip -> columns 0..1
        const int q = ctid & 31;
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {
            const int r = (ctid >> 5) + 8 * pass;
            if (q < 17 && (pass < 2 || ctid < 64)) {
                f32x2c* t = reinterpret_cast<f32x2c*>(RA + r * (C2_T * C2_LD) + (SAVE ? 16 * C2_LD : 0) + 2 * q);
                f32x2c* c = reinterpret_cast<f32x2c*>(CC + r * 34 + 2 * q);
                if (SAVE) *c = *t; else *t = *c;
            }
        }
    };
    // vertical strips: contiguous in both tiles (whole rows), one float4 per thread
    auto copy_rows = [&](auto SAVE_T) {                          // pooled rows 16..19 -> VP, or VP -> rows 0..3 (RB)
        constexpr bool SAVE = decltype(SAVE_T)::value;
        if (ctid < VCARRY_P / 4) {
            f32x4* t = reinterpret_cast<f32x4*>(RB + (SAVE ? 16 * P1_T * 10 : 0)) + ctid;
            f32x4* c = reinterpret_cast<f32x4*>(VP) + ctid;
            if (SAVE) *c = *t; else *t = *c;
        }
    };
    auto copy_rows2 = [&](auto SAVE_T) {                         // conv2 rows 16..17 -> VC, or VC -> rows 0..1 (RA)
        constexpr bool SAVE = decltype(SAVE_T)::value;
        static_assert((16 * C2_T * C2_LD) % 4 == 0 && VCARRY_C % 4 == 0, "float4 copies");
        if (ctid < VCARRY_C / 4) {
            f32x4* t = reinterpret_cast<f32x4*>(RA + (SAVE ? 16 * C2_T * C2_LD : 0)) + ctid;
            f32x4* c = reinterpret_cast<f32x4*>(VC) + ctid;
            if (SAVE) *c = *t; else *t = *c;
        }
    };
    // Dynamic schedule inside the XCD's chunk: a workgroup takes the next RUN of a.run consecutive tile indices (band order: see
    // decode) of its XCD from an atomic cursor, so one that starts late (another stream's kernel still on its CU) or loses time
    // simply processes fewer runs; inside a run the next tile is tile + 1 (the tile below, or the top of the next column: its
    // neighbours' carry strips are then in LDS); the cursor value for the tile after a run is fetched at the top of the run's
    // last tile and travels through LDS (the loop's own barriers order it).
    __shared__ int next_tile_s;
    int run_len = a.run;
    if (tid == 0) next_tile_s = t_begin + atomicAdd(&a.xcd_next[xcd], run_len);
    __syncthreads();
    int tile = __builtin_amdgcn_readfirstlane(next_tile_s);
    __syncthreads();
    TileId cur = decode(tile < t_end ? tile : 0), nxt = cur;
    if (tile < t_end) issue_input(cur);
    int rot = 0, tile_nxt = tile, run_pos = 0;
    // who left the strips: tile index of the last saver of each horizontal slot and of the vertical strips (a tile carries only
    // from exactly its neighbour's index, so a stale entry can never match)
    int hs_tile[BAND], vs_tile = -1;
#pragma unroll
    for (int i = 0; i < BAND; i++) hs_tile[i] = -1;
    // DBG + TRL_PNET_CLOCK: shader-clock time of every wave in each phase and at each barrier, summed over the launch (clk[CLK_PHASE + 8 wave + k])
    unsigned long long pt[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_last = 0;
    const bool prof = DBG && a.prof != 0;
    auto stamp = [&](int k) {
        if (DBG && prof) { const unsigned long long t = clock64(); pt[k] += t - pt_last; pt_last = t; }
    };
    if (DBG && prof) pt_last = clock64();
    unsigned nscr = 0, ncnf = 0;                  // DBG: M-tiles this wave screened / confirmed (clk[CLK_SCREENED], clk[CLK_CONFIRMED])
    for (; tile < t_end; tile = tile_nxt, cur = nxt, rot++) {
        const int f = cur.f, l = cur.l, ty = cur.ty, tx = cur.tx;
        const TileId& g = cur;
        asm volatile("" : "+v"(ctid));
        const int vrows = (g.oh - ty * TS < TS) ? g.oh - ty * TS : TS;      // valid output rows of this tile
        // left neighbour = `rows` positions back in the band order, upper neighbour = the previous position
        const bool carry = tx > 0 && (g.rib == 0 ? hs_tile[0] : (g.rib == 1 ? hs_tile[1] : hs_tile[BAND - 1])) == tile - g.rows;
        const bool vcarry = g.rib > 0 && vs_tile == tile - 1;
        const bool last_of_run = run_pos + 1 >= run_len;
        const bool feeds_next = run_pos + g.rows < run_len && tx + 1 < g.tiles_x;   // the right neighbour is a later tile of this run
        const bool feeds_down = !last_of_run && g.rib + 1 < g.rows;                   // the next tile of the run is the tile below
        float* const CP = CP0 + g.rib * (CARRY_P + CARRY_C);
        float* const CC = CP + CARRY_P;
        if (feeds_next) { if (g.rib == 0) hs_tile[0] = tile; else if (g.rib == 1) hs_tile[1] = tile; else hs_tile[BAND - 1] = tile; }
        if (feeds_down) vs_tile = tile;
        int cursor = tile + 1 - t_begin;
        // Guided self-scheduling: near the end of the XCD's chunk the runs shrink (down to single tiles), so the workgroups of an XCD
        // finish within a tile of each other instead of within a run.  Any run length is correct: a run is whatever atomicAdd hands out.
        int rem = (t_end - tile - 64 * run_len) >> 7;      // ~ tiles left per pair of workgroups (the cursor runs ~64 runs ahead of this tile)
        const int next_len = rem < 1 ? 1 : (rem > a.run ? a.run : rem);
        if (tid == 0 && last_of_run) cursor = atomicAdd(&a.xcd_next[xcd], next_len);   // in flight during phases 0-2, published at the barrier that ends phase 2
        run_pos = last_of_run ? 0 : run_pos + 1;
        run_len = last_of_run ? next_len : run_len;

        // ---- phase 0: prefetched input tile -> RA as [42][42][3] ---------------------------------------------
        stamp(7);
        if (!(dbg_skip & 16)) {
#pragma unroll
        for (int i = 0; i < 7; i++) {        // p < 1792: the 28 pixels past the tile land in RA's tail (finite, never a live operand)
            float* d = RA + 3 * tid + 768 * i;
            d[0] = pre[i].x; d[1] = pre[i].y; d[2] = pre[i].z;
        }
        }
        stamp(0);
        __syncthreads();
        stamp(1);

        // ---- phase 1: conv1 + 2x2 ceil max-pool + PReLU -> RB as [20][20][10] ------------------------------
        // conv1 (3 -> 10 channels, K = 27) runs on the 4x4x1 block instruction (see mfma4 above): wave w owns pooled rows w, w+4,
        // .., w+16.  Rows w .. w+12 x the 16 columns a carrying tile computes are ONE super unit of 64 cells (lane = cell, one
        // conv1 position per pass, the pool = an elementwise max of the four passes' accumulators); the fifth row and -- in a tile
        // without a left neighbour -- columns 0..3 run as quad units (block = cell, lanes = the four positions, pool = two DPP max).
        // Every LDS address is a per-lane base plus a compile-time offset; 420 block instructions of 8 cycles per wave and carry
        // tile against 20 x 7 16x16x4 instructions of 32 cycles before (N = 10 padded to 16, K = 27 to 28).
        if (!(dbg_skip & 2)) {
            const int vy = g.h - 2 - ty * 2 * TS, vx = g.w - 2 - tx * 2 * TS;   // valid conv1 extent inside the tile
            // max-pool commutes with PReLU when the slope is >= 0 (monotone): pool first, one PReLU per cell.  With a negative
            // slope somewhere the window's min is pooled as well and max_i prelu(v_i) = max(m, s n) (trl_prelu_pooled): still
            // one PReLU per pooled cell, never four before the pool.
            // Interior tiles (every conv1 pixel of the tile inside the level) also skip the ceil-mode masks.
            const bool fast = vy >= 2 * P1_T && vx >= 2 * P1_T;
            // CARRY: pooled columns 0..3 come from the left neighbour (CP, written in its phase 2): only column groups pg = 1..4 are
            // computed -- 20 M-tiles per wave instead of 25
            if (carry) copy_pooled(std::false_type{}, CP);
            if (vcarry) copy_rows(std::false_type{});      // (rows 0..3 of the strip columns arrive twice, with the same values)
            // Units of this wave: the wide units (columns 4..19) of its five pooled rows wave + 4 i; a tile that does not carry also
            // computes columns 0..3 as five NARROW units (4 rows x 4 columns each): narrow unit `wave` goes to this wave, narrow unit 4
            // to one wave in turn.  Units run in pairs (six independent accumulator chains keep the 8-cycle instruction issuing back to
            // back); the loop is not unrolled -- four instantiations of the body (edge masks x one / two units) instead of the old
            // path's four fully unrolled 25-tile sequences keeps the kernel's code inside the instruction cache.
            struct XU { int lb, sb, row, col; };
            auto wide_u = [&](int i) { XU u; u.lb = c1x_w + i * (8 * IN_T * 3); u.sb = c1x_sw + i * (4 * P1_T * 10); u.row = wave + 4 * i; u.col = 4 + xb; return u; };
            auto narrow_u = [&](int n) {
                XU u; u.row = 4 * n + (xb >> 2); u.col = xb & 3;
                u.lb = ((2 * u.row + xdy) * IN_T + 2 * u.col + xdx) * 3; u.sb = (u.row * P1_T + u.col) * 10 + 4 * xj;
                return u;
            };
            auto x_epi = [&](auto EDGE_T, const XU& u, const f32x4 (&acc)[3]) {
                constexpr bool EDGE = decltype(EDGE_T)::value;
                const float ninf = -__builtin_inff();
                const bool pv = !EDGE || ((2 * u.row + xdy < vy) && (2 * u.col + xdx < vx));     // this lane's conv1 pixel lies inside the level
                float m[3][4], n[3][4];
#pragma unroll
                for (int cg = 0; cg < 3; cg++) {
                    f32x4 v = acc[cg];
                    if (EDGE) { v[0] = pv ? v[0] : ninf; v[1] = pv ? v[1] : ninf; v[2] = pv ? v[2] : ninf; v[3] = pv ? v[3] : ninf; }
                    quad_max4(v, m[cg]);
                    if (NEG1) {
                        f32x4 w = acc[cg];
                        if (EDGE) { w[0] = pv ? w[0] : -ninf; w[1] = pv ? w[1] : -ninf; w[2] = pv ? w[2] : -ninf; w[3] = pv ? w[3] : -ninf; }
                        quad_min4(w, n[cg]);
                    }
                }
                const bool cv = !EDGE || ((2 * u.row < vy) && (2 * u.col < vx));                 // the cell exists (its (0,0) pixel does)
                float o[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float pm = lane_sel(lane_sel(m[2][r], m[1][r], 0x2222222222222222ull), m[0][r], 0x1111111111111111ull);   // lane j: group j
                    const float sel = UNIT ? 0.f : trl_prelu_sel(sl4[r]);
                    if (NEG1) {
                        const float pn = lane_sel(lane_sel(n[2][r], n[1][r], 0x2222222222222222ull), n[0][r], 0x1111111111111111ull);
                        o[r] = prelu_pooled_t<UNIT>(pm, pn, sl4[r], sel);
                    } else {
                        o[r] = prelu_t<UNIT>(pm, sl4[r], sel);
                    }
                    if (EDGE) o[r] = cv ? o[r] : 0.f;
                }
                if (xj < 3) {                                    // lane j stores channels 4j .. 4j+3 of its cell (j = 2: channels 8, 9)
                    *reinterpret_cast<f32x2c*>(RB + u.sb) = f32x2c{o[0], o[1]};
                    if (xj < 2) *reinterpret_cast<f32x2c*>(RB + u.sb + 2) = f32x2c{o[2], o[3]};
                }
            };
            auto x_units = [&](auto EDGE_T, auto HASB_T, const XU& A, const XU& B) {
                constexpr bool HASB = decltype(HASB_T)::value;
                f32x4 accA[3], accB[3];
                float xa[2][9], xc[2][9];
                auto rd = [&](int t, float* xo, int lb) {        // k = 9 t + u sits at lb + 126 t + u of the [42][42][3] tile
#pragma unroll
                    for (int u = 0; u < 9; u++) xo[u] = RA[lb + 126 * t + u];
                };
                rd(0, xa[0], A.lb);
                if (HASB) rd(0, xc[0], B.lb);
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int cg = 0; cg < 3; cg++) {                 // the chain starts at the bias: slot k = 27 of the weight registers x 1.0
                    accA[cg] = mfma4<4, 11>(WC[cg][1], xone, z);
                    if (HASB) accB[cg] = mfma4<4, 11>(WC[cg][1], xone, z);
                }
                pn_static_for(std::make_integer_sequence<int, 3>{}, [&](auto T) __attribute__((always_inline)) {
                    constexpr int t = decltype(T)::value;
                    if (t < 2) { rd(t + 1, xa[(t + 1) & 1], A.lb); if (HASB) rd(t + 1, xc[(t + 1) & 1], B.lb); }
                    __builtin_amdgcn_sched_barrier(0);
                    pn_static_for(std::make_integer_sequence<int, 9>{}, [&](auto UU) __attribute__((always_inline)) {
                        constexpr int u = decltype(UU)::value, k = 9 * t + u;
#pragma unroll
                        for (int cg = 0; cg < 3; cg++) {
                            accA[cg] = mfma4<4, (k & 15)>(WC[cg][k >> 4], xa[t & 1][u], accA[cg]);
                            if (HASB) accB[cg] = mfma4<4, (k & 15)>(WC[cg][k >> 4], xc[t & 1][u], accB[cg]);
                        }
                    });
                    __builtin_amdgcn_sched_barrier(0);
                });
                x_epi(EDGE_T, A, accA);
                if (HASB) x_epi(EDGE_T, B, accB);
            };
            // Rows wave, wave+4, wave+8, wave+12 x columns 4..19 as ONE super unit: pass p computes conv1 position (dy, dx) = (p >> 1, p & 1)
            // of all 64 cells (lane = cell); two passes run interleaved (six chains), the pool is an elementwise max of the passes'
            // accumulators -- 24 VALU per 64 cells where four quad units spend 96 DPP max and 32 selects -- and each lane applies the
            // PReLU to, and stores, its own cell's ten channels.
            auto x_super = [&](auto EDGE_T) {
                constexpr bool EDGE = decltype(EDGE_T)::value;
                const float ninf = -__builtin_inff();
                const int srow = wave + 4 * xj + (vcarry ? 4 : 0), scol = 4 + xb;   // a vertically carried tile computes rows 4..19
                const int sv_l = vcarry ? 8 * IN_T * 3 : 0, sv_s = vcarry ? 4 * P1_T * 10 : 0;
                f32x4 mx[3], mn[3];
                pn_static_for(std::make_integer_sequence<int, 2>{}, [&](auto PP) __attribute__((always_inline)) {
                    constexpr int pp = decltype(PP)::value;      // passes 2 pp (dx = 0) and 2 pp + 1 (dx = 1) of conv1 row parity dy = pp
                    const int lbA = c1s_l + sv_l + pp * (IN_T * 3), lbB = lbA + 3;
                    f32x4 accA[3], accB[3];
                    float xa[2][9], xc[2][9];
                    auto rd = [&](int t, float* xo, int lb) {
#pragma unroll
                        for (int u = 0; u < 9; u++) xo[u] = RA[lb + 126 * t + u];
                    };
                    rd(0, xa[0], lbA); rd(0, xc[0], lbB);
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int cg = 0; cg < 3; cg++) { accA[cg] = mfma4<4, 11>(WC[cg][1], xone, z); accB[cg] = mfma4<4, 11>(WC[cg][1], xone, z); }
                    pn_static_for(std::make_integer_sequence<int, 3>{}, [&](auto T) __attribute__((always_inline)) {
                        constexpr int t = decltype(T)::value;
                        if (t < 2) { rd(t + 1, xa[(t + 1) & 1], lbA); rd(t + 1, xc[(t + 1) & 1], lbB); }
                        __builtin_amdgcn_sched_barrier(0);
                        pn_static_for(std::make_integer_sequence<int, 9>{}, [&](auto UU) __attribute__((always_inline)) {
                            constexpr int u = decltype(UU)::value, k = 9 * t + u;
#pragma unroll
                            for (int cg = 0; cg < 3; cg++) {
                                accA[cg] = mfma4<4, (k & 15)>(WC[cg][k >> 4], xa[t & 1][u], accA[cg]);
                                accB[cg] = mfma4<4, (k & 15)>(WC[cg][k >> 4], xc[t & 1][u], accB[cg]);
                            }
                        });
                        __builtin_amdgcn_sched_barrier(0);
                    });
                    const bool pvA = !EDGE || ((2 * srow + pp < vy) && (2 * scol < vx)), pvB = !EDGE || ((2 * srow + pp < vy) && (2 * scol + 1 < vx));
#pragma unroll
                    for (int cg = 0; cg < 3; cg++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const float va = EDGE ? (pvA ? accA[cg][r] : ninf) : accA[cg][r], vb = EDGE ? (pvB ? accB[cg][r] : ninf) : accB[cg][r];
                            mx[cg][r] = pp == 0 ? vmax_nc(va, vb) : vmax3_nc(mx[cg][r], va, vb);
                            if (NEG1) {
                                const float wa = EDGE ? (pvA ? accA[cg][r] : -ninf) : accA[cg][r], wb = EDGE ? (pvB ? accB[cg][r] : -ninf) : accB[cg][r];
                                mn[cg][r] = pp == 0 ? vmin_nc(wa, wb) : vmin3_nc(mn[cg][r], wa, wb);
                            }
                        }
                });
                const bool cv = !EDGE || ((2 * srow < vy) && (2 * scol < vx));
                float o[12];
#pragma unroll
                for (int c = 0; c < 10; c++) {
                    const float sl = a.s1[c];                    // uniform: a scalar load, the multiply takes it as an SGPR operand
                    const float sel = UNIT ? 0.f : trl_prelu_sel(sl);
                    o[c] = NEG1 ? prelu_pooled_t<UNIT>(mx[c >> 2][c & 3], mn[c >> 2][c & 3], sl, sel) : prelu_t<UNIT>(mx[c >> 2][c & 3], sl, sel);
                    if (EDGE) o[c] = cv ? o[c] : 0.f;
                }
#pragma unroll
                for (int c = 0; c < 10; c += 2) *reinterpret_cast<f32x2c*>(RB + c1s_s + sv_s + c) = f32x2c{o[c], o[c + 1]};
            };
            if (fast) x_super(std::false_type{}); else x_super(std::true_type{});
            // ... the fifth row (wave + 16) and, in a tile that does not carry, the narrow units as quad units (pool = the block's lanes).
            // A vertically carried tile has no fifth row (rows 4..19 are the super unit); without a left neighbour its columns 0..3 of
            // rows 4..19 are narrow units 1..4, one per wave; with both carries there is nothing left.
            const int extra_wave = rot & 3;                      // the wave that takes narrow unit 4 of a tile that does not carry
#pragma unroll 1
            for (int pr = 2; pr < 4; pr++) {
                if (vcarry && (carry || pr == 3)) break;
                if (pr == 3 && (carry || wave != extra_wave)) break;
                const XU A = vcarry ? narrow_u(wave + 1) : (pr < 3 ? wide_u(4) : narrow_u(4));
                const XU B = narrow_u(wave);
                const bool two = pr == 2 && !carry && !vcarry;
                if (fast) { if (two) x_units(std::false_type{}, std::true_type{}, A, B); else x_units(std::false_type{}, std::false_type{}, A, B); }
                else { if (two) x_units(std::true_type{}, std::true_type{}, A, B); else x_units(std::true_type{}, std::false_type{}, A, B); }
            }
        }
        stamp(2);
        __syncthreads();
        stamp(3);

        // ---- phase 2: conv2 + PReLU -> RA as [324][17] ---------------------------------------------------------
        if (!(dbg_skip & 4)) {
            // 21 M-tiles of 16 rows (last one 4 rows); wave w takes pairs (w, w+4), (w+8, w+12), (w+16, w+20).
            // RA (the input tile) is dead since the barrier above, so the epilogue may overwrite it.
            // The A operands of pair j+1 are requested right after the MFMAs of pair j are issued, so their LDS
            // latency hides under that pair's tail and epilogue (same registers: MFMA sources are read at issue).
            // The 21 M-tiles split 6/5/5/5 over the waves; the 6-tile role rotates with the tile counter so that no
            // SIMD (wave i of both resident workgroups sits on SIMD i) is the long pole every time.
            const int w2 = (wave + rot) & 3;
            const int lim2 = C2_T * (vrows + 3 < C2_T ? vrows + 3 : C2_T);   // conv2 cells conv3 reads: rows 0 .. vrows+2
            // the pooled columns the right neighbour will not recompute (RB is read-only during this phase; CP was consumed
            // before the barrier that ended phase 1)
            if (feeds_next) copy_pooled(std::true_type{}, CP);
            if (feeds_down) copy_rows(std::true_type{});
            if (vcarry) copy_rows2(std::false_type{});       // conv2 rows 0..1 come from the upper neighbour (VC, written in its phase 3)
            if (carry) copy_conv2(std::false_type{}, CC);    // conv2 columns 0..1 from the left neighbour (CC, written in its phase 3)
            const int r0 = vcarry ? 2 : 0;                      // first conv2 row this tile computes
            float xa[23], xb[23];
            if (carry) {
                // conv2 columns 0..1 come from the left neighbour (CC, written in its phase 3); the 16 new columns of row y are
                // ONE M-tile: 18 M-tiles (instead of 21), wave role w2 takes rows w2, w2+4, .., every address a lane base + immediate
                const int rows2 = vrows + 3 < C2_T ? vrows + 3 : C2_T;          // conv2 rows conv3 reads
                const int cbase = (2 + l15) * 10;
                auto read_rows = [&](int j) {
                    int yA = r0 + w2 + 8 * j;
                    yA = yA < C2_T ? yA : C2_T - 1;                         // (rows past the tile are not computed: stay inside it)
                    const int yB = (yA + 4 < C2_T) ? yA + 4 : yA;
#pragma unroll
                    for (int s = 0; s < 23; s++) xa[s] = RB[yA * (P1_T * 10) + cbase + koff<30, 170>(s, kq, 0, e2_2, 0)];
                    if (yA + 4 < C2_T) {
#pragma unroll
                        for (int s = 0; s < 23; s++) xb[s] = RB[yB * (P1_T * 10) + cbase + koff<30, 170>(s, kq, 0, e2_2, 0)];
                    }
                };
                read_rows(0);
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int yA = r0 + w2 + 8 * j, yB = yA + 4;
                    const bool hasA = yA < rows2, hasB = yB < rows2;         // (rows2 <= 18: also bounds the row index)
                    f32x4 accA = bias2v, accB = bias2v;
                    __builtin_amdgcn_sched_barrier(0);
                    if (!hasA) {
                    } else if (hasB) {
                        accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0], B2[0], bias2v, 0, 0, 0);
                        accB = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[0], B2[0], bias2v, 0, 0, 0);
#pragma unroll
                        for (int s = 1; s < 23; s++) {
                            accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], B2[s], accA, 0, 0, 0);
                            accB = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[s], B2[s], accB, 0, 0, 0);
                        }
                    } else {
                        accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0], B2[0], bias2v, 0, 0, 0);
#pragma unroll
                        for (int s = 1; s < 23; s++) accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], B2[s], accA, 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if (j < 2) read_rows(j + 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (hasA) RA[(yA * C2_T + 2 + kq * 4 + q) * C2_LD + l15] = prelu_t<UNIT>(accA[q], slope2, sel2);
                        if (hasB) RA[(yB * C2_T + 2 + kq * 4 + q) * C2_LD + l15] = prelu_t<UNIT>(accB[q], slope2, sel2);
                    }
                }
            } else {
            // (a vertically carried tile without a left neighbour: rows 2..17 = cells 36..323 = 18 M-tiles, the same walk shifted)
            const int c0 = r0 * C2_T, nmt2 = vcarry ? 18 : 21;
            auto read_pair2 = [&](int j) {
                const int mtA = w2 + 8 * j, mtB = (mtA + 4 < 21) ? mtA + 4 : mtA;
                int mA = c0 + mtA * 16 + l15; mA = mA < 324 ? mA : 323;
                int mB = c0 + mtB * 16 + l15; mB = mB < 324 ? mB : 323;
                const int yA = mA / C2_T, xA = mA - yA * C2_T, yB = mB / C2_T, xB = mB - yB * C2_T;
                const int baseA = (yA * P1_T + xA) * 10, baseB = (yB * P1_T + xB) * 10;
#pragma unroll
                for (int s = 0; s < 23; s++) xa[s] = RB[baseA + koff<30, 170>(s, kq, 0, e2_2, 0)];
                if (j < 2 || w2 == 0) {
#pragma unroll
                    for (int s = 0; s < 23; s++) xb[s] = RB[baseB + koff<30, 170>(s, kq, 0, e2_2, 0)];
                }
            };
            read_pair2(0);
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int mtA = w2 + 8 * j, mtB = mtA + 4;
                // Tiles on the bottom edge of a level hold fewer than 16 valid output rows: conv2 cells below the rows conv3 will
                // read are skipped (M-tile m covers cells 16m.. of the 18-wide grid).  Uniform per wave, no barrier inside.
                const bool hasB = mtB < nmt2 && c0 + 16 * mtB < lim2;  // j == 2: only wave role 0 has a second tile (M-tile 20)
                const bool hasA = mtA < nmt2 && c0 + 16 * mtA < lim2;
                f32x4 accA = bias2v, accB = bias2v;
                __builtin_amdgcn_sched_barrier(0);
                if (!hasA) {
                } else if (hasB) {
                    accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0], B2[0], bias2v, 0, 0, 0);     // C operand = the bias quad (see conv1)
                    accB = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[0], B2[0], bias2v, 0, 0, 0);
#pragma unroll
                    for (int s = 1; s < 23; s++) {
                        accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], B2[s], accA, 0, 0, 0);
                        accB = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[s], B2[s], accB, 0, 0, 0);
                    }
                } else {
                    accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0], B2[0], bias2v, 0, 0, 0);
#pragma unroll
                    for (int s = 1; s < 23; s++) accA = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], B2[s], accA, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (j < 2) read_pair2(j + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int ra = c0 + mtA * 16 + kq * 4 + q;
                    if (hasA && ra < 324) RA[ra * C2_LD + l15] = prelu_t<UNIT>(accA[q], slope2, sel2);
                    const int rb = c0 + mtB * 16 + kq * 4 + q;
                    if (hasB && rb < 324) RA[rb * C2_LD + l15] = prelu_t<UNIT>(accB[q], slope2, sel2);
                }
            }
            }   // !carry
        }
        if (tid == 0) next_tile_s = t_begin + cursor;   // the cursor's atomic has had phases 0-2 to return
        stamp(4);
        __syncthreads();
        stamp(5);

        // The screen's activation operands, once per tile: RA's 324 x 16 conv2 values rounded to fp16 (the same plain cast screen()
        // applied per tap and M-tile, about eight times per cell) into XH, and the error weight m = sum of g[channel] |x| over each cell's
        // 8-channel half into XM (g: pnet_screen_bound's per-channel coefficients; eight fmaf, the order every cell's sum is taken in).
        // Both live in RB: its last readers are phase 2's copy_pooled / copy_rows and conv2's A operands, all in front of the barrier
        // above, and its next writer is the next tile's phase 1 (copy_pooled / copy_rows in, then the units), two barriers on; phase 1
        // rewrites all 400 x 10 pooled words of every tile, whatever it carries (strip columns 0..3 and / or rows 0..3 copied in, the
        // rest computed), so phase 2 never reads a word written here as an f32: that alone keeps conv2's zero-weight k padding
        // finite.  Beyond it: a word of XH has an fp16 in its upper half, whose five exponent bits and top three mantissa bits
        // are the f32's exponent, so a finite or infinite fp16 (mantissa bits 000 under an all-ones exponent at most) never makes
        // it 255 -- only the fp16 NaN of a conv2 value that is already a NaN can; XM is clamped to the largest finite float, which
        // changes no decision: every |x| above 65504 confirms its M-tile.  The zeroed tail RB[4000..] that the k padding of the
        // last cells reaches is not touched.
        // Item i = 324 half + cell.  Thread t takes cell t of half 0, cell t of half 1, then cells 256..323: waves 0, 1 their half 0,
        // waves 2, 3 their half 1.  Consecutive lanes read RA 17 floats apart and write consecutive 16-byte / 4-byte slots.  In front
        // of the next tile's prefetch: its 21 registers are not live yet.
        if (a.screen) {
            static_assert(SCR_XM + 2 * 324 <= P1_T * P1_T * 10, "fp16 conv2 tile + error weights stay inside the pooled tile");
#pragma unroll
            for (int p = 0; p < 3; p++) {
                // the channel half is uniform per wave, so its eight error weights are scalar operands (loaded from the argument block)
                const int half = p < 2 ? p : wave >> 1;
                int cell = ctid;
                if (p == 2) { cell = ctid & 127; cell = 256 + (cell < 324 - 256 ? cell : 324 - 256 - 1); }   // (the spare threads repeat the last cell: same values, no branch)
                const int i = 324 * half + cell;
                const float* src = RA + cell * C2_LD + 8 * half;
                const float* gs = a.scrG + 8 * half;
                f16x8 hv;
                float m = 0.f, mx = 0.f;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const float v = src[j], av = fabsf(v);
                    mx = fmaxf(mx, av);
                    m = __builtin_fmaf(gs[j], av, m);
                    hv[j] = (_Float16)v;
                }
                *reinterpret_cast<f16x8*>(RB + 4 * i) = hv;
                // the overflow rule, explicit: an item with an |x| beyond fp16 (or a sum that is not a finite float: a NaN input) stores
                // the largest finite float -- no f32 infinity in region B; screen()'s E then reaches that value and the M-tile confirms
                RB[SCR_XM + i] = mx > 65504.f ? 3.402823466e38f : fminf(m, 3.402823466e38f);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();   // (uniform: a.screen is a kernel argument)
        }

        // next tile's input: global loads into registers only (RA is still read by phase 3)
        tile_nxt = __builtin_amdgcn_readfirstlane(next_tile_s);
        if (tile_nxt < t_end) { nxt = decode(tile_nxt); if (!(dbg_skip & 1)) issue_input(nxt); }
        // the conv2 columns / rows the right / lower neighbour will not recompute (RA is read-only until the barrier that ends the
        // tile) are copied behind the wave's last conv3 M-tile, in front of the last head chain
        auto strips_get = [&]() __attribute__((always_inline)) {
            if (feeds_next) copy_conv2(std::true_type{}, CC);
            if (feeds_down) copy_rows2(std::true_type{});
        };

        // ---- phase 3: conv3 + PReLU -> heads -> candidates, register to register -------------------------------------
        if (!(dbg_skip & 8)) {
            const float fscale = g.scale;
            const f32x4* T3 = reinterpret_cast<const f32x4*>(T3all);
            // the exact chain of an M-tile of this tile (pn_conv3, PnHeads, pn_emit above)
            [[maybe_unused]] auto conv3 = [&](int mt, f32x16& P, auto&& between) __attribute__((always_inline)) { pn_conv3<UNIT>(RA, B3S, T3, mt, l31, hh, P, between); };
            [[maybe_unused]] auto emit = [&](int mt, const f32x4& hq) __attribute__((always_inline)) {
                pn_emit(a, f, l, ty * TS + mt * 2, tx * TS, g.oh, g.ow, fscale, dbg_skip, lane, hq);
            };
            // 8 M-tiles of 32 cells = 2 output rows each; wave w takes M-tiles w and w + 4 (a bottom-edge tile may have neither or
            // only the first: those output rows lie below the level).  The head chain of the first rides in the MFMA stream of the
            // second -- one 8-cycle block instruction after every second 64-cycle one, so its 32 dependent steps never wait.
            const int mt0 = wave, mt1 = wave + 4;
            const bool has0 = 2 * mt0 < vrows, has1 = 2 * mt1 < vrows;
            bool cf0 = has0, cf1 = has1;                        // M-tiles that take the exact f32 path
            // fp16 screen: conv3 of each M-tile on v_mfma_f32_32x32x16_f16, one instruction per 3x3 tap
            // (K = the 16 conv2 channels), in the transposed layout of conv3 below -- lane l: cell l & 31, channels
            // 8 (q >> 2) + (q & 3) + 4 hh.  The activations come from the tile's fp16 copy in region B (one 16-byte read per tap, the
            // error weight of the same eight values beside it), the weights are rounded from LDS as they are read.  Then PReLU and
            // the logit difference d (one 16-term chain per half, the halves added): an M-tile is confirmed when some valid cell
            // has d + E >= dthr (E = sum over the cell's 3x3x16 conv2 inputs of g[channel] |x|, + B), d is not finite or an input
            // exceeds fp16.  A cell the exact path would let through the prefilter (d_exact >= dthr) always confirms its M-tile, so
            // the records are unchanged.
            if (has0 && a.screen) {
                const int sb0 = 324 * hh + (mt0 * 2 + (l31 >> 4)) * C2_T + (l31 & 15);   // item of the lane's cell and channel half (XH / XM above)
                auto screen = [&](int mt, int sb) __attribute__((always_inline)) {
                    f32x16 S;
#pragma unroll
                    for (int qa = 0; qa < 4; qa++) {
                        const f32x4 b4 = T3[2 * qa + hh];
#pragma unroll
                        for (int qb = 0; qb < 4; qb++) S[4 * qa + qb] = b4[qb];
                    }
                    float em = 0.f;
#pragma unroll
                    for (int tap = 0; tap < 9; tap++) {
                        const int to = (tap / 3) * C2_T + tap % 3;
                        f16x8 wv;
#pragma unroll
                        for (int j = 0; j < 8; j++) wv[j] = (_Float16)B3S[(tap * 16 + 8 * hh + j) * 32 + l31];
                        const f16x8 xv = *reinterpret_cast<const f16x8*>(RB + 4 * (sb + to));
                        em += RB[SCR_XM + sb + to];
                        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv, xv, S, 0, 0, 0);
                    }
                    float part = 0.f;
#pragma unroll
                    for (int qa = 0; qa < 4; qa++) {
                        const f32x4 s4 = T3[8 + 2 * qa + hh], w4 = T3[18 + 2 * qa + hh];   // slopes, difference weights
#pragma unroll
                        for (int qb = 0; qb < 4; qb++)
                            part = __builtin_fmaf(w4[qb], prelu_t<UNIT>(S[4 * qa + qb], s4[qb], UNIT ? 0.f : trl_prelu_sel(s4[qb])), part);
                    }
                    const auto pp = __builtin_amdgcn_permlane32_swap(__float_as_uint(part), __float_as_uint(part), false, false);
                    const auto px = __builtin_amdgcn_permlane32_swap(__float_as_uint(em), __float_as_uint(em), false, false);
                    const float d = (part + __uint_as_float(pp[1])) + T3all[104];
                    // E = the 18 error weights of the cell's field + B; an item beyond fp16 stored the largest finite float, so E is
                    // at least that (or overflows): every such cell confirms, as does one whose E a finite float cannot hold
                    const float E = (em + __uint_as_float(px[1])) + a.scrB;
                    const int oy = ty * TS + mt * 2 + (lane >> 4), ox = tx * TS + (lane & 15);
                    const bool hit = !(d + E < a.dthr) || !(fabsf(d) <= 3.402823466e38f) || !(E < 3.402823466e38f);
                    return __builtin_amdgcn_ballot_w64(lane < 32 && oy < g.oh && ox < g.ow && hit) != 0;
                };
                cf0 = screen(mt0, sb0);
                if (has1) cf1 = screen(mt1, sb0 + 8 * C2_T);   // M-tile mt0 + 4: 8 conv2 rows down
                if (DBG) { nscr += has1 ? 2 : 1; ncnf += (cf0 ? 1 : 0) + (cf1 ? 1 : 0); }
            }
            if constexpr (DEFER) {
                // a confirmed M-tile goes to the queue: one slot (the counter keeps counting past the capacity: the host learns the
                // need), the M-tile's 72 conv2 cells = 306 16-byte words from region A (read-only until the barrier that ends the
                // tile), the header.  A launch whose queue is full raises FLG_DEFER and is run again (trl_capacity.h)
                auto defer = [&](int mt) __attribute__((always_inline)) {
                    int slot = 0;
                    if (lane == 0) slot = atomicAdd(a.q_cnt, 1);
                    slot = __builtin_amdgcn_readfirstlane(slot);
                    if (slot < a.q_cap) {
                        char* const dst = a.q + (size_t)slot * TRL_DEFER_SLOT;
                        const f32x4* src = reinterpret_cast<const f32x4*>(RA + mt * (2 * C2_T * C2_LD));
                        f32x4* d4 = reinterpret_cast<f32x4*>(dst + TRL_DEFER_HDR);
#pragma unroll
                        for (int i = 0; i < (TRL_DEFER_BLOCK / 16 + 63) / 64; i++) {
                            const int j = lane + 64 * i;
                            if (j < TRL_DEFER_BLOCK / 16) d4[j] = src[j];
                        }
                        if (lane == 0) {
                            int* h = reinterpret_cast<int*>(dst);
                            *reinterpret_cast<i32x4*>(h) = i32x4{f, l, ty, tx};
                            h[4] = mt;
                        }
                    } else if (lane == 0) {
                        a.flags[FLG_DEFER] = 1;
                    }
                };
                if (cf0) defer(mt0);
                if (cf1) defer(mt1);
                strips_get();
            } else if (cf0 && cf1) {
                f32x16 P0;
                f32x4 hq0 = T3[16 + hh];                        // head bias of this half's output group
                conv3(mt0, P0, [](auto, auto) {});
                {
                    f32x16 P1;
                    f32x4 hq1 = T3[16 + hh];
                    conv3(mt1, P1, [&](auto SX, auto UU) __attribute__((always_inline)) {
                        constexpr int sx = decltype(SX)::value, u = decltype(UU)::value, h = sx * 6 + (u >> 1);
                        if constexpr ((u & 1) == 1 && h < 32) {          // (pinned: the scheduler would bunch the block instructions)
                            __builtin_amdgcn_sched_barrier(0);
                            hd.template step<h>(P0, hq0);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    });
                    strips_get();
                    hd.all(P1, hq1);
                    emit(mt0, hq0);
                    emit(mt1, hq1);
                }
            } else if (cf0 || cf1) {
                const int mt = cf0 ? mt0 : mt1;
                f32x16 P0;
                f32x4 hq0 = T3[16 + hh];
                conv3(mt, P0, [](auto, auto) {});
                strips_get();
                hd.all(P0, hq0);
                emit(mt, hq0);
            } else {
                strips_get();
            }
        } else {
            strips_get();
        }
        stamp(6);
        __syncthreads();   // RA / RB are rewritten by the next tile
        stamp(7);
    }
    if (DBG && prof && lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) atomicAdd(&a.clk[CLK_PHASE + 8 * wave + k], pt[k]);
        if (wave == 0) atomicAdd(&a.clk[CLK_ROT], (unsigned long long)rot);
    }
    // (a DEFER launch counts into CLK_PEND_SCREENED / CLK_PEND_CONFIRMED: k_pnet_span adds them to the totals unless the queue overflowed -- that launch's records
    // are dropped and its re-run counts the same M-tiles again)
    if (DBG && lane == 0 && nscr) { atomicAdd(&a.clk[DEFER ? CLK_PEND_SCREENED : CLK_SCREENED], (unsigned long long)nscr); atomicAdd(&a.clk[DEFER ? CLK_PEND_CONFIRMED : CLK_CONFIRMED], (unsigned long long)ncnf); }
    if (DBG && tid == 0) atomicMax(&a.clk[CLK_END], (unsigned long long)wall_clock64());
}

// The second pass behind a DEFER launch: the exact f32 chain of every queued M-tile, ONE wave per slot, no barrier between the
// waves once the conv3 weights are in LDS.  The grid is sized by the queue's capacity; workgroups past the device-side count
// return at once (k_mtcnn_front's convention).  A wave loads its slot's 4 conv2 rows into its own LDS area, laid out like region
// A's rows, and runs what the inline instantiations run for M-tile 0 of such a tile: pn_conv3, the head chain, pn_emit -- the same
// instructions in the same order per output, so the records are the inline path's bit for bit; their order inside a level's list
// is arbitrary on both paths (atomicAdd slots; the list kernels sort on (score, cell) keys).  8 waves per workgroup: 58 KB of LDS,
// two workgroups per CU, 4 waves per SIMD (<= 128 VGPRs): the matrix pipe has another wave's chain to run while one waits on LDS.
constexpr int CONFIRM_WAVES = 8;
template <bool UNIT>
__global__ __launch_bounds__(64 * CONFIRM_WAVES, 4) void k_pnet_confirm(PnetArgs a) {
    __shared__ __attribute__((aligned(16))) float B3S[144 * 32];
    __shared__ __attribute__((aligned(16))) float WA[CONFIRM_WAVES][4 * C2_T * C2_LD];
    __shared__ __attribute__((aligned(16))) float T3all[72];     // conv3 bias[32], PReLU slopes[32], head bias[8]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int asked = *a.q_cnt;                                  // slots the fused launch asked for: beyond q_cap it stored nothing
    if (blockIdx.x == 0 && tid == 0) a.flags[FLG_DEFER_N] = asked;
    const int n = asked < a.q_cap ? asked : a.q_cap;
    if ((int)blockIdx.x * CONFIRM_WAVES >= n) return;
    for (int i = tid; i < 144 * 32; i += 64 * CONFIRM_WAVES) B3S[i] = a.w3[i];
    if (tid < 32) { T3all[tid] = a.b3[tid]; T3all[32 + tid] = a.s3[tid]; if (tid < 8) T3all[64 + tid] = a.bh[tid]; }
    const int slot = blockIdx.x * CONFIRM_WAVES + wave;
    const char* const src = a.q + (size_t)(slot < n ? slot : 0) * TRL_DEFER_SLOT;
    if (slot < n) {
        const f32x4* s4 = reinterpret_cast<const f32x4*>(src + TRL_DEFER_HDR);
        f32x4* d4 = reinterpret_cast<f32x4*>(WA[wave]);
#pragma unroll
        for (int i = 0; i < (TRL_DEFER_BLOCK / 16 + 63) / 64; i++) {
            const int j = lane + 64 * i;
            if (j < TRL_DEFER_BLOCK / 16) d4[j] = s4[j];
        }
    }
    PnHeads hd;
    hd.load(a.wh, lane);
    __syncthreads();
    if (slot >= n) return;
    const int* h = reinterpret_cast<const int*>(src);
    const int f = h[0], l = h[1], ty = h[2], tx = h[3], mt = h[4];
    const PLevel& g = a.lv[l];
    const int l31 = lane & 31, hh = lane >> 5;
    const f32x4* T3 = reinterpret_cast<const f32x4*>(T3all);
    f32x16 P;
    f32x4 hq = T3[16 + hh];
    pn_conv3<UNIT>(WA[wave], B3S, T3, 0, l31, hh, P, [](auto, auto) {});
    hd.all(P, hq);
    pn_emit(a, f, l, ty * TS + mt * 2, tx * TS, g.oh, g.ow, g.scale, 0, lane, hq);
}

}  // namespace

// after a fused launch: CLK_SPAN_SUM += its span, CLK_LAUNCHES += 1, CLK_LAST_SPAN = its span; the start / end stamps are re-armed for
// the next launch; a DEFER launch whose queue held every M-tile: CLK_SCREENED / CLK_CONFIRMED += the M-tiles it screened / confirmed,
// CLK_QUEUED += the M-tiles it queued
__global__ void k_pnet_span(unsigned long long* clk, const int32_t* q_cnt, int q_cap) {
    const unsigned long long t0 = clk[CLK_START], t1 = clk[CLK_END];
    const unsigned long long d = t1 > t0 ? t1 - t0 : 0ull;
    clk[CLK_SPAN_SUM] += d; clk[CLK_LAUNCHES] += 1ull; clk[CLK_LAST_SPAN] = d;
    clk[CLK_START] = ~0ull; clk[CLK_END] = 0ull;
    if (q_cnt) {
        if (*q_cnt <= q_cap) { clk[CLK_SCREENED] += clk[CLK_PEND_SCREENED]; clk[CLK_CONFIRMED] += clk[CLK_PEND_CONFIRMED]; clk[CLK_QUEUED] += (unsigned long long)*q_cnt; }
        clk[CLK_PEND_SCREENED] = clk[CLK_PEND_CONFIRMED] = 0ull;
    }
}

// Error bound of the fp16 conv3 screen: for a cell whose 3x3x16 conv2 inputs satisfy |x| <= X <= 65504,
// |d_screen - d_exact| <= A X + B, d = logit1 - logit0.  Operands round once to fp16 (relative 2^-11, absolute 2^-14 for a
// subnormal kept or flushed), the MFMA sums 145 terms in an unspecified order (taken at 2u per addition), the exact chain is 145
// fmaf; PReLU is Lipschitz with max(1, |slope|); the exact heads are two 33-term chains and a subtraction, the screened
// difference head one 36-term chain over f32(w1 - w0).  Double precision, then A and B rounded up (tools/pnet_screen_audit.py
// states the same bound, tests/test_pnet_screen_cpu.py compares the two).  W [144][32], H [32][32] (zero padded), b3, s3, bh: the
// loader's host copies of conv3.w, heads.w, conv3.b, prelu3, heads.b.
// Every term of A is a sum over the inputs k = (tap, channel) of a non-negative coefficient times X, and X enters only as the
// bound |x_k| <= X: with the coefficients kept apart, |d_screen - d_exact| <= sum_k g_k |x_k| + B, sum_k g_k = A.  The kernel uses
// g^[channel] = max over the nine taps of g_(tap, channel) (pnet_scrG), so that sum_k g^ |x_k| is a sum over the field's nine
// conv2 cells of one number per cell and channel half.  g^ is multiplied by the same 1 + 2^-10 as A and B and rounded up to float.
// That factor also has to cover the kernel's own f32 roundings of E, all of them in sums of non-negative terms: 8 for a cell half's
// eight fmaf, 8 for the nine halves of a lane, 1 for the two lanes' sums, 1 for + B -- no term passes more than 18 roundings, a
// relative loss below 18 * 2^-24 = 2^-19.8 against the 2^-10 granted (d + E is compared without a subtraction, as before).
static void pnet_screen_bound(trl_ctx* c, const float* W, const float* H, const float* b3, const float* s3, const float* bh) {
    c->pnet_screen_ok = 0; c->pnet_scrA = c->pnet_scrB = __builtin_inff();
    for (int i = 0; i < 16; i++) c->pnet_scrG[i] = __builtin_inff();
    for (int i = 0; i < 144 * 32; i++) if (!(fabsf(W[i]) <= 65504.f)) return;   // a weight fp16 cannot hold: no screen for this net
    const double u = ldexp(1.0, -24), uh = ldexp(1.0, -11), tiny = ldexp(1.0, -14);
    auto gamma = [](int n, double uu) { return n * uu / (1.0 - n * uu); };
    const double ge = gamma(145, u), gs = gamma(145, 2 * u), g35 = gamma(35, u), g36 = gamma(36, u);
    double Sa = 0, Sb = fabs((double)bh[0]) + fabs((double)bh[1]);
    double ad = 0, bd = 0, wdP_a = 0, wdP_b = 0;
    double g[144] = {};                            // A's terms, per input k
    for (int co = 0; co < 32; co++) {
        double W1 = 0, D = 0;
        for (int k = 0; k < 144; k++) {
            const double w = W[k * 32 + co], aw = fabs(w);
            W1 += aw;
            D += aw < tiny ? aw : fabs((double)(float)(_Float16)W[k * 32 + co] - w);
        }
        const double b = fabs((double)b3[co]), L = fmax(1.0, fabs((double)s3[co]));
        const double a3 = D * (1 + uh) + W1 * uh + gs * (W1 + D) * (1 + uh) + ge * W1;
        const double b3e = D * tiny + W1 * tiny + gs * (b + (W1 + D) * tiny) + ge * b;
        const double aM = W1 * (1 + ge), bM = b * (1 + ge);
        const double ap = L * (1 + u) * a3 + 2 * u * L * aM, bp = L * (1 + u) * b3e + 2 * u * L * bM;
        const double aP = L * (1 + u) * aM, bP = L * (1 + u) * bM;
        const double w0 = H[co * 32 + 0], w1 = H[co * 32 + 1], wd = fabs(w1 - w0);
        Sa += (fabs(w0) + fabs(w1)) * aP; Sb += (fabs(w0) + fabs(w1)) * bP;
        ad += wd * ap; bd += wd * bp;
        wdP_a += wd * (aP + ap); wdP_b += wd * (bP + bp);
        for (int k = 0; k < 144; k++) {            // the same a3, aM, ap, aP with (|w_k|, D_k) in place of (W1, D)
            const double w = W[k * 32 + co], aw = fabs(w), Dk = aw < tiny ? aw : fabs((double)(float)(_Float16)W[k * 32 + co] - w);
            const double a3k = Dk * (1 + uh) + aw * uh + gs * (aw + Dk) * (1 + uh) + ge * aw, aMk = aw * (1 + ge);
            const double apk = L * (1 + u) * a3k + 2 * u * L * aMk, aPk = L * (1 + u) * aMk;
            g[k] += g35 * (fabs(w0) + fabs(w1)) * aPk + wd * apk + g36 * (1 + u) * wd * (aPk + apk);
        }
    }
    ad += g36 * (1 + u) * wdP_a;
    bd += g36 * (1 + u) * (fabs((double)bh[1] - (double)bh[0]) + wdP_b);
    const double A = (g35 * Sa + ad) * (1 + ldexp(1.0, -10)), B = (g35 * Sb + bd) * (1 + ldexp(1.0, -10));
    auto up = [](double v) { float f = (float)v; return (double)f < v ? nextafterf(f, __builtin_inff()) : f; };
    c->pnet_scrA = up(A); c->pnet_scrB = up(B); c->pnet_screen_ok = 1;
    for (int ci = 0; ci < 16; ci++) {
        double m = 0;
        for (int tap = 0; tap < 9; tap++) m = fmax(m, g[tap * 16 + ci]);
        c->pnet_scrG[ci] = up(m * (1 + ldexp(1.0, -10)));
    }
}

// PNet's layers in c->mt (trl_resolve_nets has checked their shapes: [27][10], [90][16], [144][32], [32][6], each in 32 columns)
enum { PN_CONV1 = 0, PN_CONV2 = 2, PN_CONV3 = 3, PN_HEADS = 4 };

int trl_pnet_prepare(trl_ctx* c, const char* himg) {
    const NetLayerW* l = c->mt[TRL_PNET];
    auto host = [&](const float* dev) { return trl_host_of(c, himg, dev); };
    c->pnet_mono1 = c->pnet_unit = 1;
    for (int i : {PN_CONV1, PN_CONV2, PN_CONV3}) {
        const float* sl = host(l[i].slope);
        for (int k = 0; k < l[i].w->Cout; k++) {
            if (i == PN_CONV1 && !(sl[k] >= 0.f)) c->pnet_mono1 = 0;
            if (!(sl[k] <= 1.f)) c->pnet_unit = 0;
        }
    }
    pnet_screen_bound(c, host(l[PN_CONV3].w->p), host(l[PN_HEADS].w->p), host(l[PN_CONV3].b), host(l[PN_CONV3].slope), host(l[PN_HEADS].b));
    return TRL_OK;
}

// ceil(2^32 / d) for the kernel's sdiv(); d == 1 would need 2^32: 2^32 - 1 gives q = n - 1 (or 0), which sdiv's upward correction
// step turns into n -- no special case on the device
static unsigned sdiv_magic(int d) { return d <= 1 ? 0xFFFFFFFFu : (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); }

static void fill_args(trl_ctx* c, int n, int H, int W, const PyrLayout& lay, const PyrPx* pyr, PnetArgs& a) {
    a.pyr = pyr; a.pyr_stride = lay.pyr_stride;
    a.n_frames = n; a.L = lay.L; a.H = H; a.W = W;
    int tiles = 0;
    for (int l = 0; l < lay.L; l++) {
        const LevelGeom& g = c->lv[l];
        PLevel& p = a.lv[l];
        p.h = g.h; p.w = g.w; p.oh = g.oh; p.ow = g.ow;
        p.tiles_x = (g.ow + TS - 1) / TS;
        p.txmagic = sdiv_magic(p.tiles_x);
        p.tile0 = tiles;
        p.tiles_y = (g.oh + TS - 1) / TS;
        p.bmagic = sdiv_magic(BAND * p.tiles_x);
        tiles += p.tiles_x * p.tiles_y;
        p.pix0 = lay.lv[l].pix0;
        p.scale = (float)g.scale;
        p.cap = c->cb.lay.capl[l]; p.rec0 = c->cb.lay.rec0[l];   // (set by trl_cascade_detect before the fused launch)
    }
    a.tiles_per_frame = tiles;
    a.tpf_magic = sdiv_magic(tiles);
    const NetLayerW* l = c->mt[TRL_PNET];
    a.w1 = l[PN_CONV1].w->p; a.w2 = l[PN_CONV2].w->p; a.w3 = l[PN_CONV3].w->p; a.wh = l[PN_HEADS].w->p;
    a.b1 = l[PN_CONV1].b; a.b2 = l[PN_CONV2].b; a.b3 = l[PN_CONV3].b; a.bh = l[PN_HEADS].b;
    a.s1 = l[PN_CONV1].slope; a.s2 = l[PN_CONV2].slope; a.s3 = l[PN_CONV3].slope;
    a.thr = c->cfg.thr0; a.rec_stride = c->cb.lay.S;
    // p = softmax(logit0, logit1)[1] >= thr needs logit1 - logit0 >= ln(thr / (1 - thr)) up to the rounding of the float softmax
    // (~1e-6 relative); 0.05 below that bound the probability is short of thr by 0.05 thr (1 - thr) >= 4.9e-4 for thr in [0.01, 0.99]
    a.dthr = (a.thr >= 0.01f && a.thr <= 0.99f) ? (float)(log((double)a.thr / (1.0 - (double)a.thr)) - 0.05) : -__builtin_inff();
    a.scrB = c->pnet_scrB; a.screen = c->opt.pnet_screen && c->pnet_screen_ok;
    for (int i = 0; i < 16; i++) a.scrG[i] = c->pnet_scrG[i];
    a.dbg_skip = trl_tune_int("TRL_PNET_SKIP", 0);
    a.lvl_cnt = c->cb.lvl_cnt; a.lvl_rec = c->cb.lvl_rec; a.flags = c->cb.flags;
    a.clk = c->pnet_clk; a.prof = c->pnet_prof ? 1 : 0;
    a.xcd_next = c->pnet_cursor;
    a.q = c->cb.pq; a.q_cap = c->cb.pq ? c->cb.pq_cap : 0; a.q_cnt = c->pnet_cursor + 8;
}

// Deferral applies where the screen is on, leaves something out (thr0 inside the prefilter's range: outside it every M-tile
// confirms) and the net has a DEFER instantiation (no slope above 1); every other launch runs the exact chain inline
bool trl_pnet_can_defer(const trl_ctx* c) {
    return c->opt.pnet_defer && c->opt.pnet_screen && c->pnet_screen_ok && c->pnet_unit && c->cfg.thr0 >= 0.01f && c->cfg.thr0 <= 0.99f &&
           trl_tune_int("TRL_PNET_SKIP", 0) == 0;
}
long long trl_pnet_mtiles(const trl_ctx* c, int L, int n) {
    long long m = 0;
    for (int l = 0; l < L; l++) if (c->lv[l].oh > 0 && c->lv[l].ow > 0) m += (long long)((c->lv[l].ow + TS - 1) / TS) * ((c->lv[l].oh + 1) / 2);
    return m * n;
}

size_t trl_pnet_fused_bytes(trl_ctx* c, int n, int H, int W) {
    PyrLayout lay;
    if (trl_pyramid_layout(c, H, W, lay) != TRL_OK) return 0;
    return trl_pyramid_bytes(lay, n) + 4096;
}

// All pyramid levels of all n frames: the pyramid kernels + one persistent fused launch.
// ev[0..1] bracket the pyramid kernels, ev[2..3] the fused kernel and, where the launch defers, k_pnet_confirm behind it (HIP events
// on the same stream): both are PNet work.
int trl_pnet_fused_all(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, hipEvent_t* ev, hipStream_t s) {
    PyrLayout lay;
    PyrPx* pyr = nullptr;
    TRL_CHECK(trl_pyramid_build(c, d_frames, n, H, W, lay, &pyr, ev, s));
    PnetArgs a;
    fill_args(c, n, H, W, lay, pyr, a);
    const int total_tiles = a.tiles_per_frame * n;
    int grid = 256 * 2;   // 2 resident workgroups per CU (<= 256 VGPRs)
    if (grid > ((total_tiles + 7) / 8) * 8) grid = ((total_tiles + 7) / 8) * 8;
    if (grid < 8) grid = 8;
    TRL_HIP(hipMemsetAsync(c->pnet_cursor, 0, 9 * sizeof(int32_t), s));   // the 8 tile cursors and the confirm queue's slot counter
    // The persistent grid fills every CU: it waits for the end of the device's previous call (another context's cascade tail or
    // embedder) and then runs alone, so the event pair below is its duration; the pyramid kernels queued in front of it are
    // memory-bound and DO overlap that call's narrow kernels (trl_gate_wait, trl_api.hip).
    TRL_CHECK(trl_gate_wait(c, s));
    if (ev) TRL_HIP(hipEventRecord(ev[2], s));   // the event pair brackets PNet's kernels alone (HIP events on the launch's stream)
    // instantiation: slopes all <= 1 or not, a negative conv1 slope or not, diagnostics (TRL_PNET_CLOCK / TRL_PNET_SKIP) or not
#ifdef TRL_TUNING
    const bool dbg = c->pnet_prof || a.dbg_skip || trl_tune_set("TRL_PNET_SPAN");   // the instantiation with clock stamps / ablations
#else
    const bool dbg = false;                              // (not even instantiated in the shipped library)
#endif
    // Tiles per cursor fetch: a run of 24 = 8 columns of a 3-row band (7 of 8 columns carry horizontally, 2 of 3 rows vertically);
    // small batches keep shorter runs, down to single tiles, so that every CU gets work
    // (trl_debug_pnet_run overrides it: tests that exercise the carry path on small frames)
    const int auto_run = (total_tiles / 8) / 128;
    a.run = c->opt.pnet_run > 0 ? c->opt.pnet_run : (auto_run < 1 ? 1 : (auto_run > 8 * BAND ? 8 * BAND : auto_run));
    auto launch = [&](auto kern) {
        // static + dynamic LDS exceed the default 64 KB per workgroup
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, DYN_LDS) != hipSuccess) return false;
        kern<<<grid, 256, DYN_LDS, s>>>(a);
        return true;
    };
    bool launched = false;
#ifdef TRL_TUNING
#define TRL_PK(U, N, D) do { launched = dbg ? launch(k_pnet_fused<U, N, true, D>) : launch(k_pnet_fused<U, N, false, D>); } while (0)
#else
#define TRL_PK(U, N, D) do { launched = launch(k_pnet_fused<U, N, false, D>); } while (0)
#endif
    // (the plan gave the call a confirm queue only where trl_pnet_can_defer held: a UNIT net with the screen on)
    const bool defer = a.q_cap > 0;
    if (defer && !(c->pnet_unit && a.screen)) { trl_set_error("confirm queue planned for a launch that cannot defer"); return TRL_ERR_STATE; }
    if (defer) { if (c->pnet_mono1) TRL_PK(true, false, true); else TRL_PK(true, true, true); }
    else if (c->pnet_unit) { if (c->pnet_mono1) TRL_PK(true, false, false); else TRL_PK(true, true, false); }
    else { if (c->pnet_mono1) TRL_PK(false, false, false); else TRL_PK(false, true, false); }
#undef TRL_PK
    if (!launched) { trl_set_error("k_pnet_fused: %d bytes of dynamic LDS refused", DYN_LDS); return TRL_ERR_HIP; }
    TRL_LAUNCH_CHECK();
    if (defer) {   // the queued M-tiles, right behind it: PNet work, inside the event pair
        k_pnet_confirm<true><<<(a.q_cap + CONFIRM_WAVES - 1) / CONFIRM_WAVES, 64 * CONFIRM_WAVES, 0, s>>>(a);
        TRL_LAUNCH_CHECK();
    }
    if (ev) TRL_HIP(hipEventRecord(ev[3], s));
    if (dbg) {
        k_pnet_span<<<1, 1, 0, s>>>(c->pnet_clk, defer ? a.q_cnt : nullptr, a.q_cap);   // fold the launch's span into the running sums, re-arm the two stamps
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

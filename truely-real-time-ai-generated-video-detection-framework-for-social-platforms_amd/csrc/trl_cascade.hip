// trl_cascade.hip -- the data-dependent part of MTCNN.detect on the device (gfx950).
//
// Restates facenet_pytorch 2.6.0 utils/detect_face.py::detect_face + MTCNN.detect
// (select_largest=True) as called at server/model.py:47, and model.py:49-54 (int cast, clamp; the crops
// of model.py:55-58 are trl_crops.hip's).  Everything stays on the GPU; candidates live in
// fixed-capacity per-frame lists.  One workgroup owns one (frame, level) or one frame segment:
//   sort   : bitonic sort in LDS on a 64-bit key  (~score | tie-break index) -> exactly the order of
//            a stable descending sort, so results do not depend on the order candidates were
//            appended by the PNet kernel's atomics;
//   NMS    : greedy suppression in sorted order, all lanes test one kept box against the rest;
//   compact: ordered compaction by block scan, so list order equals the reference's `pick` order.
// The four list kernels (k_nms_level, k_nms_frame, k_stage2_post, k_stage3_post) share one routine for the first two
// (sort_and_suppress: LDS tier and spill tier) and one for the third (write_rows); a kernel adds its keys, its boxes and its rows.
// All float expressions follow the reference's operation order (one rounding per op,
// -ffp-contract=off), so boxes / keep masks are bit-identical to the oracle.
#include "trl_ctx.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>

// R-/O-Net candidates per launch set: one set covers a 256-frame batch's CAPACITY (160 / 48 candidates per frame + 64: 41 k / 12.4 k;
// 31 k / 8.5 k are live), so no dead second chunk is launched (8 launches x 4.7 us); scratch per chunk = 100 KB / 640 KB per
// candidate (5 / 10.7 GB at the cap, of 288 GB)
// (trl_debug_option("rnet_chunk" / "onet_chunk") shrinks a launch set for tests, so that the multi-chunk path runs on small inputs)

namespace {

__device__ __forceinline__ uint32_t f2ord(float f) {   // ascending-order preserving map
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The 64-bit sort key: ascending keys = descending score, ties by ascending `tie`.  NO_KEY sorts behind every entry.
__device__ __forceinline__ uint64_t sort_key(float score, uint32_t tie) { return ((uint64_t)~f2ord(score) << 32) | tie; }
constexpr uint64_t NO_KEY = ~0ull;

// ---- block primitives ------------------------------------------------------------------------
// The bitonic network's compare-exchange distances j0, j0/2, .., 1 of merge width k on C LDS-resident entries that are entries
// [base, base + C) of the list.  A list that fits LDS is sorted by `for k = 2, 4, .., P: steps(key, id, P, 0, k, k / 2)`.
__device__ void lds_bitonic_steps(uint64_t* key, uint32_t* id, int C, int base, int k, int j0) {
    for (int j = j0; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < C; t += blockDim.x) {
            const int u = t ^ j;
            if (u > t) {
                const bool up = (((base + t) & k) == 0);
                const uint64_t a = key[t], b = key[u];
                if ((a > b) == up) {
                    key[t] = b; key[u] = a;
                    const uint32_t ia = id[t]; id[t] = id[u]; id[u] = ia;
                }
            }
        }
        __syncthreads();
    }
}
__device__ __forceinline__ int next_pow2(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// Does kept box i suppress box j?  MIN_MODE = nms_numpy 'Min' (+1 extents, inter / min(area), keep o <= thr); otherwise torchvision
// nms (inter / (a_i + a_j - inter) > thr suppresses).  One rounding per operation, in the reference's order.
template <bool MIN_MODE>
__device__ __forceinline__ bool nms_suppresses(const float4 bi, const float ai, const float4 bj, const float aj, const float thr) {
    const float xx1 = bi.x > bj.x ? bi.x : bj.x;
    const float yy1 = bi.y > bj.y ? bi.y : bj.y;
    const float xx2 = bi.z < bj.z ? bi.z : bj.z;
    const float yy2 = bi.w < bj.w ? bi.w : bj.w;
    if (MIN_MODE) {
        float w = xx2 - xx1 + 1.f; w = w > 0.f ? w : 0.f;
        float h = yy2 - yy1 + 1.f; h = h > 0.f ? h : 0.f;
        const float inter = w * h;
        const float mn = ai < aj ? ai : aj;
        const float o = inter / mn;
        return !(o <= thr);
    } else {
        float w = xx2 - xx1; w = w > 0.f ? w : 0.f;
        float h = yy2 - yy1; h = h > 0.f ? h : 0.f;
        const float inter = w * h;
        const float ovr = inter / (ai + aj - inter);
        return ovr > thr;
    }
}

template <bool MIN_MODE>
__device__ __forceinline__ float box_area(const float4 b) {   // nms_numpy's +1 extents / torchvision's plain ones
    return MIN_MODE ? (b.z - b.x + 1.f) * (b.w - b.y + 1.f) : (b.z - b.x) * (b.w - b.y);
}

// Greedy NMS over boxes already in descending-score order.  MIN_MODE = facenet_pytorch
// nms_numpy(..., 'Min') (+1 areas, inter/min(area), keep o <= thr); otherwise torchvision nms
// (inter/(a_i+a_j-inter) > thr suppresses).  keep[] receives positions in pick order.
// `preset`: sup[] already holds suppressions by boxes that precede this list (the spill tier's earlier chunks).
// The list is walked in sub-blocks of 64 boxes: wave 0 resolves a sub-block by itself -- lane = box, the next live box is
// broadcast with v_readlane, no barrier between the 64 dependent steps -- then every thread applies the sub-block's kept boxes
// to its share of the later boxes.  Two barriers per 64 boxes instead of one per kept box; a box is kept iff no earlier kept box
// suppresses it, exactly the sequential rule.
template <bool MIN_MODE>
__device__ int block_nms(const float4* box, const float* area, int n, float thr, uint8_t* sup, int* keep, int* nkeep, bool preset = false) {
    __shared__ unsigned long long kept_s;
    if (!preset) for (int t = threadIdx.x; t < n; t += blockDim.x) sup[t] = 0;
    if (threadIdx.x == 0) *nkeep = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int nb = n - b0 < 64 ? n - b0 : 64;
        if (threadIdx.x < 64) {
            const bool have = lane < nb;
            const float4 bm = have ? box[b0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float am = have ? area[b0 + lane] : 0.f;
            bool dead = !have || sup[b0 + lane];
            const int base = *nkeep;
            unsigned long long kept = 0;
            for (int q = 0; q < nb; q++) {
                if ((__ballot(dead) >> q) & 1) continue;          // wave-uniform: box q was suppressed (or preset)
                kept |= 1ull << q;
                const float4 bq = make_float4(__shfl(bm.x, q), __shfl(bm.y, q), __shfl(bm.z, q), __shfl(bm.w, q));
                const float aq = __shfl(am, q);
                if (lane > q && !dead && nms_suppresses<MIN_MODE>(bq, aq, bm, am, thr)) dead = true;
            }
            if ((kept >> lane) & 1) keep[base + __popcll(kept & ((1ull << lane) - 1ull))] = b0 + lane;
            if (lane == 0) { kept_s = kept; *nkeep = base + __popcll(kept); }
        }
        __syncthreads();
        const unsigned long long kept = kept_s;
        for (int j = b0 + 64 + threadIdx.x; j < n; j += blockDim.x) {
            if (sup[j]) continue;
            const float4 bj = box[j];
            const float aj = area[j];
            bool s = false;
            for (unsigned long long m = kept; m; m &= m - 1) {
                const int q = b0 + __ffsll((long long)m) - 1;
                s |= nms_suppresses<MIN_MODE>(box[q], area[q], bj, aj, thr);
            }
            if (s) sup[j] = 1;
        }
        __syncthreads();
    }
    return *nkeep;
}

// exclusive scan of 0/1 flags (n <= capacity); returns total, pos[] = output slot
__device__ int block_compact_positions(const uint8_t* flag, int n, int* pos, int* part /*[blockDim.x + 1]*/) {
    const int tid = threadIdx.x, T = blockDim.x;
    const int per = (n + T - 1) / T;
    const int b = tid * per, e = (b + per < n) ? b + per : n;
    int cnt = 0;
    for (int i = b; i < e; i++) cnt += flag[i];
    part[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < T; i++) { const int v = part[i]; part[i] = run; run += v; }
        part[T] = run;
    }
    __syncthreads();
    int o = part[tid];
    for (int i = b; i < e; i++) { pos[i] = o; o += flag[i]; }
    __syncthreads();
    return part[T];
}

struct Smem {   // carve the dynamic LDS for capacity `cap`
    uint64_t* key; uint32_t* id; float4* box; float* area; float* aux; int* keep; int* pos; uint8_t* sup; uint8_t* flg;
    int* part; int* scal;
    __device__ Smem(unsigned char* base, int cap, int threads = 256) {
        key = (uint64_t*)base;                 // 8
        box = (float4*)(key + cap);            // 16
        id = (uint32_t*)(box + cap);           // 4
        area = (float*)(id + cap);             // 4
        aux = area + cap;                      // 4
        keep = (int*)(aux + cap);              // 4
        pos = keep + cap;                      // 4
        part = pos + cap;                      // threads + 4 ints
        scal = part + threads + 4;             // 8 ints
        sup = (uint8_t*)(scal + 8);            // 1
        flg = sup + cap;                       // 1
    }
    static size_t bytes(int cap, int threads = 256) { return (size_t)cap * 46 + (size_t)(threads + 12) * 4 + 64; }
};

// ---- spill tier: lists longer than the LDS tier ----------------------------------------------------------------------------
// detect_face() has no candidate limit (torchvision's nms and nms_numpy take any number of boxes), so neither has this cascade:
// a list that does not fit the LDS tier is sorted and suppressed by the SAME workgroup in global memory --
//   sort   : the same bitonic network on the same 64-bit keys, compare-exchange distances below the LDS chunk run in LDS,
//            the longer ones in global memory;
//   NMS    : greedy suppression in chunks of the sorted order: a chunk is first tested against every box kept from earlier
//            chunks, then suppressed in LDS like a short list.  A box is kept iff no earlier kept box suppresses it -- the
//            sequential rule, so the pick order and every keep decision equal the LDS tier's (and the reference's).
// Workspace comes from a bump pool in the cascade arena (one atomic per list); a pool that runs out raises a flag and the call is
// re-run with a larger one, like every other capacity (trl_cascade_check).
struct Spill { char* base; unsigned long long cap; int32_t* flags; };   // the pool and the overflow words (trl_capacity.h FLG_*)
__device__ char* spill_alloc(const Spill& sp, size_t bytes) {   // every thread of the workgroup calls it; uniform result
    __shared__ unsigned long long off_s;
    bytes = (bytes + 255) & ~(size_t)255;
    if (threadIdx.x == 0) {
        off_s = atomicAdd(reinterpret_cast<unsigned long long*>(sp.flags + FLG_SPILL_CUR), (unsigned long long)bytes);
        atomicAdd(&sp.flags[FLG_SPILL_LISTS], 1);
        if (off_s + bytes > sp.cap) sp.flags[FLG_SPILL] = 1;      // the cursor keeps counting: the host learns the total need
    }
    __syncthreads();
    const unsigned long long o = off_s;
    __syncthreads();
    return o + bytes <= sp.cap ? sp.base + o : nullptr;
}
__device__ __forceinline__ int pow2_floor(int n) {
    int p = 1;
    while (2 * p <= n) p <<= 1;
    return p;
}
// ascending sort of gk[0..P) (P a power of two, padded with ~0 keys) with payload gi, by one workgroup; lk / li: LDS for C entries
__device__ void big_bitonic(uint64_t* gk, uint32_t* gi, int P, uint64_t* lk, uint32_t* li, int C) {
    if (C > P) C = P;
    for (int base = 0; base < P; base += C) {
        for (int t = threadIdx.x; t < C; t += blockDim.x) { lk[t] = gk[base + t]; li[t] = gi[base + t]; }
        __syncthreads();
        for (int k = 2; k <= C; k <<= 1) lds_bitonic_steps(lk, li, C, base, k, k >> 1);
        for (int t = threadIdx.x; t < C; t += blockDim.x) { gk[base + t] = lk[t]; gi[base + t] = li[t]; }
        __syncthreads();
    }
    for (int k = 2 * C; k <= P && k > 0; k <<= 1) {
        for (int j = k >> 1; j >= C; j >>= 1) {
            for (int t = threadIdx.x; t < P; t += blockDim.x) {
                const int u = t ^ j;
                if (u > t) {
                    const bool up = ((t & k) == 0);
                    const uint64_t a = gk[t], b = gk[u];
                    if ((a > b) == up) {
                        gk[t] = b; gk[u] = a;
                        const uint32_t ia = gi[t]; gi[t] = gi[u]; gi[u] = ia;
                    }
                }
            }
            __syncthreads();
        }
        if (C > 1) {
            for (int base = 0; base < P; base += C) {
                for (int t = threadIdx.x; t < C; t += blockDim.x) { lk[t] = gk[base + t]; li[t] = gi[base + t]; }
                __syncthreads();
                lds_bitonic_steps(lk, li, C, base, k, C >> 1);
                for (int t = threadIdx.x; t < C; t += blockDim.x) { gk[base + t] = lk[t]; gi[base + t] = li[t]; }
                __syncthreads();
            }
        }
    }
}
// Greedy NMS of the first m entries of the sorted list (payload gi -> box through box_of).  kbox / karea / kid (global, m entries)
// receive the kept boxes, their areas and payloads in pick order.  S: LDS carve with room for C entries.  Returns the kept count.
//
// A chunk is first tested against the boxes kept from earlier chunks.  IoU mode (grid != null): through a uniform grid over the
// kept boxes' CENTRES (32-px cells, linked lists in global memory: head[cell], next[kept]).  A kept box i can only suppress a
// candidate j if they intersect AND inter > thr * area_i, hence w_i < w_j / thr and h_i < h_j / thr, hence
// |cx_i - cx_j| < w_j (1 + 1/thr) / 2 (same in y): the candidate walks the cells of that window only -- the pairs it skips could
// not have suppressed it, the pairs it tests are tested exactly as before, so every decision is the brute-force one.  Cell
// indices are clamped to the grid on both sides (boxes regressed past the frame land in the border cells).  'Min' mode has no such
// bound (a box of any size suppresses the boxes inside it): it tests against every kept box, staged through LDS in tiles.
struct KeptGrid { int* head; int* next; int gx, gy; };
constexpr int GRID_SHIFT = 5;
__device__ __forceinline__ int grid_clamp(float v, int n) {
    int c = (int)floorf(v * (1.0f / (1 << GRID_SHIFT)));
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}
template <bool MIN_MODE, class BoxOf>
__device__ int big_greedy(const Smem& S, int C, const uint32_t* gi, int m, float thr, BoxOf box_of, float4* kbox, float* karea,
                          uint32_t* kid, KeptGrid grid) {
    // 'Min' mode: kept boxes of earlier chunks are staged through LDS in tiles (the key area is idle during NMS: 8 C bytes = TK boxes + areas)
    const int TK = (C * 8) / 20;
    float4* tb = (float4*)S.key;
    float* ta = (float*)(tb + TK);
    constexpr int E = 2;                                  // entries of a chunk per thread: the spill tier runs with 1024 threads (C <= 2048)
    const bool use_grid = !MIN_MODE && grid.head != nullptr;
    if (use_grid) {
        for (int t = threadIdx.x; t < grid.gx * grid.gy; t += blockDim.x) grid.head[t] = -1;
        __syncthreads();
    }
    const float reach = 0.5f * (1.0f + 1.0f / thr);       // window half-size in units of the candidate's own extent (+ 1 px below)
    int K = 0;
    for (int base = 0; base < m; base += C) {
        const int nc = m - base < C ? m - base : C;
        float4 bt[E]; float at[E]; bool sp[E];
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int t = threadIdx.x + e * blockDim.x;
            sp[e] = true;                                 // (no entry)
            if (t < nc) {
                const uint32_t id = gi[base + t];
                const float4 b = box_of(id);
                bt[e] = b;
                at[e] = box_area<MIN_MODE>(b);
                S.box[t] = b; S.area[t] = at[e]; S.id[t] = id;
                sp[e] = false;
            }
        }
        if (use_grid) {
            if (K > 0) {
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if (sp[e]) continue;
                    const float4 b = bt[e];
                    const float w = b.z - b.x, h = b.w - b.y;
                    if (!(w > 0.f) || !(h > 0.f)) continue;                   // an empty box intersects nothing: never suppressed
                    const float cx = 0.5f * (b.x + b.z), cy = 0.5f * (b.y + b.w), rx = w * reach + 1.f, ry = h * reach + 1.f;
                    const int x0 = grid_clamp(cx - rx, grid.gx), x1 = grid_clamp(cx + rx, grid.gx);
                    const int y0 = grid_clamp(cy - ry, grid.gy), y1 = grid_clamp(cy + ry, grid.gy);
                    bool s = false;
                    for (int gy = y0; gy <= y1 && !s; gy++)
                        for (int gx = x0; gx <= x1 && !s; gx++)
                            for (int k = __hip_atomic_load(&grid.head[gy * grid.gx + gx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); k >= 0 && !s; k = grid.next[k])   // (head is updated by atomics at L2: read it there)
                                s = nms_suppresses<false>(kbox[k], karea[k], b, at[e], thr);
                    sp[e] = s;
                }
            }
        } else {
            // boxes kept from earlier chunks: every thread tests its own entries of the chunk against a tile of them at a time
            for (int k0 = 0; k0 < K; k0 += TK) {
                const int nt = K - k0 < TK ? K - k0 : TK;
                __syncthreads();
                for (int i = threadIdx.x; i < nt; i += blockDim.x) { tb[i] = kbox[k0 + i]; ta[i] = karea[k0 + i]; }
                __syncthreads();
#pragma unroll
                for (int e = 0; e < E; e++) {
                    if (sp[e]) continue;
                    bool s = false;
#pragma unroll 4
                    for (int k = 0; k < nt; k++) s |= nms_suppresses<MIN_MODE>(tb[k], ta[k], bt[e], at[e], thr);
                    sp[e] = s;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int t = threadIdx.x + e * blockDim.x;
            if (t < nc) S.sup[t] = sp[e] ? 1 : 0;
        }
        __syncthreads();
        const int nk = block_nms<MIN_MODE>(S.box, S.area, nc, thr, S.sup, S.keep, S.scal, true);
        for (int r = threadIdx.x; r < nk; r += blockDim.x) {
            const int t = S.keep[r];
            const float4 b = S.box[t];
            kbox[K + r] = b; karea[K + r] = S.area[t]; kid[K + r] = S.id[t];
            if (use_grid) {                               // register the kept box under its centre's cell
                const int cell = grid_clamp(0.5f * (b.y + b.w), grid.gy) * grid.gx + grid_clamp(0.5f * (b.x + b.z), grid.gx);
                grid.next[K + r] = atomicExch(&grid.head[cell], K + r);
            }
        }
        K += nk;
        __syncthreads();
    }
    return K;
}

// Workspace of one spilled list of n entries, P = next_pow2(n) sort slots:  gk | gi | kbox | karea | [kid] | [next | head].
// kid is part of it unless the kept payloads go straight to the caller's array (kid_out); next / head are the kept grid (IoU mode).
// bytes() is what the list asks of the pool -- the kernels and the host's up-front bound (spill_need) share it.
struct SpillWs {
    uint64_t* gk; uint32_t* gi; float4* kbox; float* karea; uint32_t* kid; KeptGrid grid;
    static __host__ __device__ size_t grid_cells(int W, int H) { return (size_t)((W >> GRID_SHIFT) + 1) * (size_t)((H >> GRID_SHIFT) + 1); }
    static __host__ __device__ size_t bytes(size_t P, size_t n, bool own_kid, bool grid, int W, int H) {
        return P * 12 + n * (20 + (own_kid ? 4 : 0) + (grid ? 4 : 0)) + (grid ? grid_cells(W, H) * 4 : 0);
    }
    __device__ SpillWs(char* w, int P, int n, uint32_t* kid_out, bool with_grid, int W, int H) {
        gk = (uint64_t*)w; gi = (uint32_t*)(gk + P);
        kbox = (float4*)(gi + P); karea = (float*)(kbox + n);
        int* rest = (int*)(karea + n);
        kid = kid_out ? kid_out : (uint32_t*)rest;
        if (!kid_out) rest += n;
        grid = with_grid ? KeptGrid{rest + n, rest, (W >> GRID_SHIFT) + 1, (H >> GRID_SHIFT) + 1} : KeptGrid{nullptr, nullptr, 0, 0};
    }
};

// What sort_and_suppress leaves: n kept entries in pick order, entry r = payload id(r), box(r).  keep != null: the list sits in LDS
// at the sorted positions keep[r] (S.id, S.box); otherwise in the spill workspace (kid, kbox).
struct Kept {
    int n; const int* keep; const uint32_t* ids; const float4* boxes;
    __device__ uint32_t id(int r) const { return ids[keep ? keep[r] : r]; }
    __device__ float4 box(int r) const { return boxes[keep ? keep[r] : r]; }
};

// Sort + greedy NMS of one list of n >= 1 entries by one workgroup (every thread calls it), in the LDS tier (n <= lds_cap) or the
// spill tier.  key_of(t, id) = entry t's sort_key, or NO_KEY when it is under the list's threshold (THRESHOLD lists only), and may
// replace its payload id (default t); box_of(id) = the box NMS sees.  kid_out (nullable) receives the kept payloads in pick order.
// A spilled list that finds no workspace is dropped (spill_alloc raises FLG_SPILL: the call is re-run): count 0, like an empty one.
template <bool MIN_MODE, bool THRESHOLD, class KeyOf, class BoxOf>
__device__ __forceinline__ Kept sort_and_suppress(const Smem& S, int lds_cap, int n, float nms_thr, const Spill& sp, uint32_t* kid_out, int W, int H,
                                                  KeyOf key_of, BoxOf box_of) {
    const int P = next_pow2(n);
    auto make_keys = [&](uint64_t* key, uint32_t* id) {   // P keys (NO_KEY behind the list) + payloads; returns the survivors
        if (THRESHOLD) {
            if (threadIdx.x == 0) S.scal[4] = 0;
            __syncthreads();
        }
        int mine = 0;
        for (int t = threadIdx.x; t < P; t += blockDim.x) {
            uint64_t k = NO_KEY;
            uint32_t i = t;
            if (t < n) k = key_of(t, i);
            mine += k != NO_KEY;
            key[t] = k; id[t] = i;
        }
        if (THRESHOLD && mine) atomicAdd(&S.scal[4], mine);
        __syncthreads();
        return THRESHOLD ? S.scal[4] : n;                 // (scal is reused by the NMS, behind the sort's barriers)
    };
    const Kept none{0, nullptr, nullptr, nullptr};
    if (n > lds_cap) {
        char* w = spill_alloc(sp, SpillWs::bytes(P, n, !kid_out, !MIN_MODE, W, H));
        if (!w) return none;
        const SpillWs ws(w, P, n, kid_out, !MIN_MODE, W, H);
        const int m = make_keys(ws.gk, ws.gi), C = pow2_floor(lds_cap);
        if (m == 0) return none;
        big_bitonic(ws.gk, ws.gi, P, S.key, S.id, C);
        return Kept{big_greedy<MIN_MODE>(S, C, ws.gi, m, nms_thr, box_of, ws.kbox, ws.karea, ws.kid, ws.grid), nullptr, ws.kid, ws.kbox};
    }
    const int m = make_keys(S.key, S.id);
    if (m == 0) return none;
    for (int k = 2; k <= P; k <<= 1) lds_bitonic_steps(S.key, S.id, P, 0, k, k >> 1);
    for (int t = threadIdx.x; t < m; t += blockDim.x) {
        const float4 b = box_of(S.id[t]);
        S.box[t] = b; S.area[t] = box_area<MIN_MODE>(b);
    }
    __syncthreads();
    const int nk = block_nms<MIN_MODE>(S.box, S.area, m, nms_thr, S.sup, S.keep, S.scal);
    if (kid_out) for (int r = threadIdx.x; r < nk; r += blockDim.x) kid_out[r] = S.id[S.keep[r]];
    return Kept{nk, S.keep, S.id, S.box};
}


// rerec() of one box
__device__ __forceinline__ void rerec1(float& x1, float& y1, float& x2, float& y2) {
    const float h = y2 - y1, w = x2 - x1;
    const float l = w > h ? w : h;
    x1 = x1 + w * 0.5f - l * 0.5f;
    y1 = y1 + h * 0.5f - l * 0.5f;
    x2 = x1 + l;
    y2 = y1 + l;
}
// pad(): trunc, clamp.  ok = the reference's `ey > y-1 and ex > x-1`
__device__ __forceinline__ bool pad1(float x1, float y1, float x2, float y2, int W, int H, int& y, int& ey, int& x, int& ex) {
    const int bx = (int)truncf(x1), by = (int)truncf(y1), bex = (int)truncf(x2), bey = (int)truncf(y2);
    x = bx < 1 ? 1 : bx;
    y = by < 1 ? 1 : by;
    ex = bex > W ? W : bex;
    ey = bey > H ? H : bey;
    return (ey > y - 1) && (ex > x - 1);
}

// Kept list -> rows (x1, y1, x2, y2, score) at fout, in pick order, without the rows whose clipped box is empty; returns the row
// count.  row_of(r, box, score) = row of kept entry r and whether it stays.  Chunks of `cap` rows staged in LDS (ordered
// compaction by block scan); a list of the LDS tier is one chunk.  row_of must not read S.box / S.aux / S.flg.
template <class RowOf>
__device__ __forceinline__ int write_rows(const Smem& S, int cap, int n, float* fout, RowOf row_of) {
    int out = 0;
    for (int base = 0; base < n; base += cap) {
        const int nc = n - base < cap ? n - base : cap;
        if (base) __syncthreads();                        // (the previous chunk's rows have left LDS)
        for (int r = threadIdx.x; r < nc; r += blockDim.x) {
            float4 b;
            float score;
            S.flg[r] = row_of(base + r, b, score) ? 1 : 0;
            S.box[r] = b; S.aux[r] = score;
        }
        __syncthreads();
        const int m = block_compact_positions(S.flg, nc, S.pos, S.part);
        for (int r = threadIdx.x; r < nc; r += blockDim.x) {
            if (!S.flg[r]) continue;
            float* o = fout + (size_t)(out + S.pos[r]) * 5;
            const float4 b = S.box[r];
            o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = S.aux[r];
        }
        out += m;
    }
    return out;
}

// ---- imresample (F.interpolate mode="area") of whole frames to one pyramid level --------------
__global__ void k_area_level(const uint8_t* __restrict__ frames, int nf, int H, int W, int h, int w, float* __restrict__ out) {
    const size_t total = (size_t)nf * h * w;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % w);
        const int oy = (int)((idx / w) % h);
        const int f = (int)(idx / ((size_t)w * h));
        const int ys = (int)(((long long)oy * H) / h), ye = (int)((((long long)oy + 1) * H + h - 1) / h);
        const int xs = (int)(((long long)ox * W) / w), xe = (int)((((long long)ox + 1) * W + w - 1) / w);
        unsigned s0 = 0, s1 = 0, s2 = 0;
        const uint8_t* fp = frames + (size_t)f * H * W * 3;
        for (int y = ys; y < ye; y++) {
            const uint8_t* p = fp + ((size_t)y * W + xs) * 3;
            for (int x = xs; x < xe; x++, p += 3) { s0 += p[0]; s1 += p[1]; s2 += p[2]; }
        }
        const float kh = (float)(ye - ys), kw = (float)(xe - xs);
        float* o = out + idx * 3;
        o[0] = ((float)s0 / kh / kw - 127.5f) * 0.0078125f;
        o[1] = ((float)s1 / kh / kw - 127.5f) * 0.0078125f;
        o[2] = ((float)s2 / kh / kw - 127.5f) * 0.0078125f;
    }
}

// generateBoundingBox on the generic path: heads [nf][oh][ow][6] -> candidate records
__global__ void k_pnet_collect(const float* __restrict__ heads, int nf, int f0, int oh, int ow, float scale, float thr,
                               int L, int l, int cap, int rec0, int S, int32_t* __restrict__ lvl_cnt, Cand* __restrict__ lvl_rec,
                               int32_t* __restrict__ flags) {
    const size_t total = (size_t)nf * oh * ow;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const float* hd = heads + idx * 6;
        const float p = trl_softmax2_p1(hd[0], hd[1]);
        if (!(p >= thr)) continue;
        const int cell = (int)(idx % ((size_t)oh * ow));
        const int f = f0 + (int)(idx / ((size_t)oh * ow));
        const int y = cell / ow, x = cell - y * ow;
        const int slot = atomicAdd(&lvl_cnt[f * L + l], 1);
        if (slot >= cap) { flags[FLG_LEVEL] = 1; continue; }
        Cand c;
        c.x1 = floorf((2.f * (float)x + 1.f) / scale);
        c.y1 = floorf((2.f * (float)y + 1.f) / scale);
        c.x2 = floorf((2.f * (float)x + 12.f) / scale);
        c.y2 = floorf((2.f * (float)y + 12.f) / scale);
        c.score = p;
        c.r0 = hd[2]; c.r1 = hd[3]; c.r2 = hd[4]; c.r3 = hd[5];
        c.cell = cell;
        lvl_rec[(size_t)f * S + rec0 + slot] = c;
    }
}

__global__ void k_heads_to_maps(const float* __restrict__ heads, int cells, float* __restrict__ prob, float* __restrict__ reg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const float* hd = heads + (size_t)i * 6;
    prob[i] = trl_softmax2_p1(hd[0], hd[1]);
    reg[4 * i + 0] = hd[2]; reg[4 * i + 1] = hd[3]; reg[4 * i + 2] = hd[4]; reg[4 * i + 3] = hd[5];
}

__device__ __forceinline__ float4 cand_box(const Cand& c) { return make_float4(c.x1, c.y1, c.x2, c.y2); }

// ---- stage 1a: per (frame, level) batched_nms(0.5) ------------------------------------------
// Two launches share the segments: the SMALL tier (LDS sized for `lds_cap` = 512 candidates: ~24 KB, six workgroups per CU) takes
// every segment with at most lds_cap candidates -- practically all of them: a level holds ~0.2 % of its cells -- and the FULL tier
// (LDS for 2048 candidates: 94 KB, one workgroup per CU) the crowded ones, through LDS up to its capacity and through the spill
// tier (global memory) beyond; a workgroup whose segment belongs to the other tier exits at once.  One tier for everything ran
// the 2,816 segments of a 256-frame batch in eleven rounds of 256.
__global__ __launch_bounds__(1024) void k_nms_level(LvLayout G, int lds_cap, int min_cnt, int spill_tier, int W, int H, const int32_t* __restrict__ lvl_cnt,
                                                   const Cand* __restrict__ lvl_rec,
                                                   int32_t* __restrict__ keep_cnt, int32_t* __restrict__ keep_idx,
                                                   int32_t* __restrict__ flags, Spill sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem S(smem_raw, lds_cap, blockDim.x);
    const int seg = blockIdx.x;
    const int f = seg / G.L, l = seg - f * G.L;
    const int cap = G.capl[l];
    int cnt = lvl_cnt[seg];
    // the small tier visits every segment: it reports the level's largest count (what the lists must hold: trl_cascade_check)
    if (min_cnt == 0 && threadIdx.x == 0 && cnt > 0) atomicMax(&flags[FLG_LEVEL_MAX + l], cnt);
    if (cnt > cap) { cnt = cap; if (threadIdx.x == 0) flags[FLG_LEVEL] = 1; }   // the call is re-run with longer lists
    if (cnt < min_cnt || (cnt > lds_cap && !spill_tier)) return;                  // the other tier's segment
    if (cnt == 0) { if (threadIdx.x == 0) keep_cnt[seg] = 0; return; }
    const Cand* recs = lvl_rec + (size_t)f * G.S + G.rec0[l];
    int32_t* kout = keep_idx + (size_t)f * G.S + G.rec0[l];
    const Kept K = sort_and_suppress<false, false>(S, lds_cap, cnt, 0.5f, sp, (uint32_t*)kout, W, H,
        [&](int t, uint32_t&) { return sort_key(recs[t].score, (uint32_t)recs[t].cell); },   // ties: raster (cell) order
        [&](uint32_t id) { return cand_box(recs[id]); });
    if (threadIdx.x == 0) keep_cnt[seg] = K.n;
}

// ---- stage 1b: per frame batched_nms(0.7) over all levels, regress, rerec ----------------------
// regress with the PNet offsets (w, h WITHOUT +1), rerec; ok = the clipped box is not empty
__device__ __forceinline__ bool stage1_row(const Cand& c, int W, int H, float4& box) {
    const float regw = c.x2 - c.x1, regh = c.y2 - c.y1;
    float x1 = c.x1 + c.r0 * regw, y1 = c.y1 + c.r1 * regh, x2 = c.x2 + c.r2 * regw, y2 = c.y2 + c.r3 * regh;
    rerec1(x1, y1, x2, y2);
    int y, ey, x, ex;
    box = make_float4(x1, y1, x2, y2);
    return pad1(x1, y1, x2, y2, W, H, y, ey, x, ex);
}
__global__ __launch_bounds__(1024) void k_nms_frame(LvLayout G, int lds_cap, int capF, int W, int H, const Cand* __restrict__ lvl_rec,
                                                   const int32_t* __restrict__ keep_cnt, const int32_t* __restrict__ keep_idx,
                                                   int32_t* __restrict__ n1, float* __restrict__ s1_box, int32_t* __restrict__ flags, Spill sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem S(smem_raw, lds_cap, blockDim.x);
    __shared__ int offs[33];
    const int f = blockIdx.x, L = G.L;
    if (threadIdx.x == 0) {
        int run = 0;
        for (int l = 0; l < L; l++) { offs[l] = run; run += keep_cnt[f * L + l]; }
        offs[L] = run;
        if (run > 0) atomicMax(&flags[FLG_FRAME_MAX], run);
        if (run > capF) flags[FLG_FRAME] = 1;                                    // the call is re-run with longer per-frame lists
    }
    __syncthreads();
    const int total = offs[L];
    if (total == 0 || total > capF) { if (threadIdx.x == 0) n1[f] = 0; return; }
    const Cand* frec = lvl_rec + (size_t)f * G.S;
    const int32_t* fkeep = keep_idx + (size_t)f * G.S;
    const Kept K = sort_and_suppress<false, false>(S, lds_cap, total, 0.7f, sp, nullptr, W, H,
        [&](int e, uint32_t& gid) {                          // entry e of the concatenated per-level pick lists
            int l = 0;
            while (e >= offs[l + 1]) l++;
            gid = (uint32_t)(G.rec0[l] + fkeep[G.rec0[l] + (e - offs[l])]);
            return sort_key(frec[gid].score, (uint32_t)e);   // ties: position in the concatenated list
        },
        [&](uint32_t id) { return cand_box(frec[id]); });
    const int out = write_rows(S, lds_cap, K.n, s1_box + (size_t)f * capF * 5, [&](int r, float4& b, float& score) {
        const Cand& c = frec[K.id(r)];
        score = c.score;
        return stage1_row(c, W, H, b);
    });
    if (threadIdx.x == 0) n1[f] = out;
}

// exclusive scan of per-frame counts; off[n] = total.  Also the candidate -> (frame, local) map.
__global__ __launch_bounds__(256) void k_scan_counts(const int32_t* __restrict__ cnt, int n, int32_t* __restrict__ off, int cap_total,
                                                     int32_t* __restrict__ flags, int slot) {
    // thread t owns the contiguous run [t per, (t+1) per) of frames: fixed LDS whatever n is (any batch check_call admits)
    __shared__ int part[257];
    const int t = threadIdx.x, per = (n + 255) / 256;
    const int b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    int s = 0;
    for (int i = b; i < e; i++) s += cnt[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 256; i++) { const int v = part[i]; part[i] = run; run += v; }
        part[256] = run;
    }
    __syncthreads();
    int run = part[t];
    for (int i = b; i < e; i++) { off[i] = run; run += cnt[i]; }
    // the batch the next stage processes was sized by an optimistic capacity: report the real total and whether it fits
    if (t == 0) { const int total = part[256]; off[n] = total; flags[FLG_T2N + slot] = total; if (total > cap_total) flags[FLG_T2 + slot] = 1; }
}
// Candidate list of a stage in launch order: candidate t = off[f] + i is box i of frame f.  The record holds what the front kernel
// needs to start its crop -- frame index and pad()'s clamped window (detect_face.py pad(): x = max(x1, 1), ex = min(x2, W), crop
// [y-1:ey, x-1:ex]) -- so that kernel reaches its first pixel load after ONE dependent read instead of three (map -> box -> pixels).
__global__ void k_build_map(const int32_t* __restrict__ cnt, const int32_t* __restrict__ off, const float* __restrict__ boxes, int capF,
                            int W, int H, int32_t* __restrict__ cbox) {
    const int f = blockIdx.x;
    const int c = cnt[f], o = off[f];
    for (int i = threadIdx.x; i < c; i += blockDim.x) {
        const float* b = boxes + ((size_t)f * capF + i) * 5;
        const int bx = (int)truncf(b[0]), by = (int)truncf(b[1]), bex = (int)truncf(b[2]), bey = (int)truncf(b[3]);
        const int x = bx < 1 ? 1 : bx, y = by < 1 ? 1 : by, ex = bex > W ? W : bex, ey = bey > H ? H : bey;
        int4* r = reinterpret_cast<int4*>(cbox + (size_t)(o + i) * 8);
        r[0] = make_int4(f, y - 1, x - 1, ey - (y - 1));
        r[1] = make_int4(ex - (x - 1), 0, 0, 0);
    }
}

// ---- stage 2 tail: thr1, batched_nms(0.7), bbreg, rerec ------------------------------------------
// bbreg (+1 widths) with the R-Net offsets g, rerec; ok = the clipped box is not empty
__device__ __forceinline__ bool stage2_row(const float4 b, const float* g, int W, int H, float4& out) {
    const float w = b.z - b.x + 1.f, h = b.w - b.y + 1.f;
    float x1 = b.x + g[0] * w, y1 = b.y + g[1] * h, x2 = b.z + g[2] * w, y2 = b.w + g[3] * h;
    rerec1(x1, y1, x2, y2);
    int y, ey, x, ex;
    out = make_float4(x1, y1, x2, y2);
    return pad1(x1, y1, x2, y2, W, H, y, ey, x, ex);
}
__global__ __launch_bounds__(1024) void k_stage2_post(int lds_cap, int capF, int cap_total, int W, int H, float thr, const int32_t* __restrict__ n1,
                                                     const float* __restrict__ s1_box, const int32_t* __restrict__ off2,
                                                     const float* __restrict__ out6, int32_t* __restrict__ n2,
                                                     float* __restrict__ s2_box, Spill sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem S(smem_raw, lds_cap, blockDim.x);
    const int f = blockIdx.x;
    const int cnt = n1[f];
    // total past the launch capacity: out6 is incomplete, the call is re-run with a larger capacity (flag set by k_scan_counts)
    if (cnt == 0 || off2[gridDim.x] > cap_total) { if (threadIdx.x == 0) n2[f] = 0; return; }
    const float* logits = out6 + (size_t)off2[f] * 6;
    const float* fb = s1_box + (size_t)f * capF * 5;
    auto prob = [&](int i) { return trl_softmax2_p1(logits[6 * i], logits[6 * i + 1]); };
    auto s1 = [&](uint32_t i) { const float* b = fb + 5 * i; return make_float4(b[0], b[1], b[2], b[3]); };
    const Kept K = sort_and_suppress<false, true>(S, lds_cap, cnt, 0.7f, sp, nullptr, W, H,
        [&](int i, uint32_t&) { const float p = prob(i); return p > thr ? sort_key(p, (uint32_t)i) : NO_KEY; },
        s1);
    const int out = write_rows(S, lds_cap, K.n, s2_box + (size_t)f * capF * 5, [&](int r, float4& b, float& score) {
        const int i = (int)K.id(r);
        score = prob(i);
        return stage2_row(s1(i), logits + 6 * i + 2, W, H, b);
    });
    if (threadIdx.x == 0) n2[f] = out;
}

// ---- stage 3 tail: thr2, landmarks, bbreg, nms 'Min' 0.7 --------------------------------------
__device__ __forceinline__ float4 stage3_box(const float* b, const float* g) {   // bbreg (+1 widths) with the O-Net offsets
    const float w = b[2] - b[0] + 1.f, h = b[3] - b[1] + 1.f;
    return make_float4(b[0] + g[0] * w, b[1] + g[1] * h, b[2] + g[2] * w, b[3] + g[3] * h);
}
__device__ __forceinline__ void stage3_points(const float* b, const float* pt, float* po) {
    const float w_i = b[2] - b[0] + 1.f, h_i = b[3] - b[1] + 1.f;
    for (int j = 0; j < 5; j++) {
        po[j] = w_i * pt[j] + b[0] - 1.f;
        po[5 + j] = h_i * pt[5 + j] + b[1] - 1.f;
    }
}
__global__ __launch_bounds__(1024) void k_stage3_post(int lds_cap, int capF, int cap_total, float thr, const int32_t* __restrict__ n2, const float* __restrict__ s2_box,
                                                     const int32_t* __restrict__ off3, const float* __restrict__ out16,
                                                     int32_t* __restrict__ n3, float* __restrict__ s3_box, float* __restrict__ s3_pts, Spill sp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Smem S(smem_raw, lds_cap, blockDim.x);
    const int f = blockIdx.x;
    const int cnt = n2[f];
    if (cnt == 0 || off3[gridDim.x] > cap_total) { if (threadIdx.x == 0) n3[f] = 0; return; }   // see k_stage2_post
    const float* logits = out16 + (size_t)off3[f] * 16;
    const float* fb = s2_box + (size_t)f * capF * 5;
    auto prob = [&](int i) { return trl_softmax2_p1(logits[16 * i], logits[16 * i + 1]); };
    // np.argsort ascending then take-from-the-end: descending score, ties -> higher index first
    const Kept K = sort_and_suppress<true, true>(S, lds_cap, cnt, 0.7f, sp, nullptr, 0, 0,
        [&](int i, uint32_t&) { const float p = prob(i); return p > thr ? sort_key(p, ~(uint32_t)i) : NO_KEY; },
        [&](uint32_t i) { return stage3_box(fb + 5 * i, logits + 16 * i + 2); });
    for (int r = threadIdx.x; r < K.n; r += blockDim.x) {
        const int i = (int)K.id(r);
        const float4 bb = K.box(r);
        float* o = s3_box + ((size_t)f * capF + r) * 5;
        o[0] = bb.x; o[1] = bb.y; o[2] = bb.z; o[3] = bb.w; o[4] = prob(i);
        stage3_points(fb + 5 * i, logits + 16 * i + 6, s3_pts + ((size_t)f * capF + r) * 10);
    }
    if (threadIdx.x == 0) n3[f] = K.n;
}

// MTCNN.detect ordering + model.py:49-54.  order 0: select_largest=True (area order); order 1: select_largest=False, the rows in
// detect_face's order (the pick order of the final NMS), i.e. rank = row.  box0 / rect / valid / pts0 always follow rank 0.
__global__ __launch_bounds__(64) void k_select(int capF, int max_faces, int W, int H, int order, const int32_t* __restrict__ n3,
                                               const float* __restrict__ s3_box, const float* __restrict__ s3_pts,
                                               float* __restrict__ boxes, float* __restrict__ probs, float* __restrict__ points,
                                               int32_t* __restrict__ counts, float* __restrict__ box0, float* __restrict__ prob0,
                                               int32_t* __restrict__ rect, uint8_t* __restrict__ valid, float* __restrict__ pts0) {
    const int f = blockIdx.x;
    const int n = n3[f];
    const float* b = s3_box + (size_t)f * capF * 5;
    // rank of r in np.argsort(area)[::-1] with stable-sort tie semantics: descending area, ties -> higher index first
    for (int r = threadIdx.x; r < n; r += blockDim.x) {
        int rank = r;
        if (order == 0) {
            const float ar = (b[5 * r + 2] - b[5 * r]) * (b[5 * r + 3] - b[5 * r + 1]);
            rank = 0;
            for (int q = 0; q < n; q++) {
                const float aq = (b[5 * q + 2] - b[5 * q]) * (b[5 * q + 3] - b[5 * q + 1]);
                rank += (aq > ar) || (aq == ar && q > r);
            }
        }
        if (boxes && rank < max_faces) {
            float* o = boxes + ((size_t)f * max_faces + rank) * 4;
            o[0] = b[5 * r]; o[1] = b[5 * r + 1]; o[2] = b[5 * r + 2]; o[3] = b[5 * r + 3];
            probs[(size_t)f * max_faces + rank] = b[5 * r + 4];
            if (points) {   // detect(landmarks=True): points[..., j] = (x_j, y_j), stored x0..x4,y0..y4 like the stage-3 rows
                const float* ps = s3_pts + ((size_t)f * capF + r) * 10;
                float* po = points + ((size_t)f * max_faces + rank) * 10;
                for (int q = 0; q < 10; q++) po[q] = ps[q];
            }
        }
        if (rank == 0 && box0) {
            box0[4 * f] = b[5 * r]; box0[4 * f + 1] = b[5 * r + 1]; box0[4 * f + 2] = b[5 * r + 2]; box0[4 * f + 3] = b[5 * r + 3];
            prob0[f] = b[5 * r + 4];
            // model.py:49-53: boxes[0].astype(int) (toward zero), clamp
            long long x0 = (long long)b[5 * r], y0 = (long long)b[5 * r + 1], x1 = (long long)b[5 * r + 2], y1 = (long long)b[5 * r + 3];
            if (x0 < 0) x0 = 0;
            if (y0 < 0) y0 = 0;
            if (x1 > W) x1 = W;
            if (y1 > H) y1 = H;
            rect[4 * f] = (int)x0; rect[4 * f + 1] = (int)y0; rect[4 * f + 2] = (int)x1; rect[4 * f + 3] = (int)y1;
            valid[f] = (x1 > x0 && y1 > y0) ? 1 : 0;   // model.py:54
            if (pts0) {                                 // embedding mode 3: the largest face's five landmarks
                const float* ps = s3_pts + ((size_t)f * capF + r) * 10;
                for (int q = 0; q < 10; q++) pts0[10 * f + q] = ps[q];
            }
        }
    }
    if (threadIdx.x == 0) {
        if (counts) counts[f] = n < max_faces ? n : max_faces;
        if (n == 0 && box0) {
            for (int q = 0; q < 4; q++) { box0[4 * f + q] = 0.f; rect[4 * f + q] = 0; }
            prob0[f] = 0.f; valid[f] = 0;
            if (pts0) for (int q = 0; q < 10; q++) pts0[10 * f + q] = 0.f;
        }
    }
}

template <typename K>
int set_dyn_smem(K kernel, size_t bytes) {
    TRL_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return TRL_OK;
}

}  // namespace

// ---- host helpers -------------------------------------------------------------------------------
int trl_compute_levels(trl_ctx* c, int H, int W) {
    // detect_face.py: m = 12/minsize; minl = min(h,w)*m; while minl >= 12: scales += [scale_i]; scale_i *= factor
    const double m = 12.0 / c->cfg.min_face_size;
    double minl = (H < W ? H : W) * m;
    double scale_i = m;
    int L = 0;
    while (minl >= 12 && L < 32) {
        LevelGeom& g = c->lv[L];
        g.scale = scale_i;
        g.h = (int)(H * scale_i + 1);
        g.w = (int)(W * scale_i + 1);
        const int ph = (g.h - 2 + 1) / 2, pw = (g.w - 2 + 1) / 2;
        g.oh = ph - 4; g.ow = pw - 4;
        L++;
        scale_i = scale_i * c->cfg.factor;
        minl = minl * c->cfg.factor;
    }
    return L;
}

int trl_launch_area_level(const uint8_t* d_frames, int nf, int H, int W, int h, int w, float* d_level, hipStream_t s) {
    const size_t total = (size_t)nf * h * w;
    size_t blocks = (total + 255) / 256;
    if (blocks > 32768) blocks = 32768;
    k_area_level<<<(unsigned)blocks, 256, 0, s>>>(d_frames, nf, H, W, h, w, d_level);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
int trl_launch_heads_to_maps(const float* d_heads, int cells, float* d_prob, float* d_reg, hipStream_t s) {
    k_heads_to_maps<<<(cells + 255) / 256, 256, 0, s>>>(d_heads, cells, d_prob, d_reg);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

// the fused launch carries 16 level descriptors; taller pyramids (a 16 K frame at min_face_size 12) take the per-level path
static bool pnet_is_fused(const trl_ctx* c, int L) { return c->cfg.pnet_mode == 0 && L <= 16; }
// The capacities of this attempt (trl_capacity.h): record slots per level, rows per frame, the R-/O-Net batches
static void plan_caps(trl_ctx* c, int L, int n) {
    // the fused PNet's confirm queue (0 slots: the exact chain runs inline)
    DeferCaps& d = c->caps.defer;
    d.mtiles = trl_pnet_mtiles(c, L, n);
    c->cb.pq_cap = d.cap = trl_defer_plan(d, d.mtiles, pnet_is_fused(c, L) && trl_pnet_can_defer(c));
    long long cells[32];
    for (int l = 0; l < L; l++) cells[l] = (long long)c->lv[l].oh * c->lv[l].ow;
    const CascadePlan p = trl_caps_plan(c->caps, c->cfg.cap_level, c->cfg.cap_frame, cells, L, n);
    c->cb.lay = p.lay;
    c->cb.capF = p.capF;
    c->caps.cap_t[0] = p.cap_t[0]; c->caps.cap_t[1] = p.cap_t[1];
}
static size_t spill_need(long long cnt, int W, int H) {   // upper bound of the workspace of one spilled list of cnt entries, whichever kernel spills it
    long long P = 2;
    while (P < cnt) P <<= 1;
    return SpillWs::bytes((size_t)P, (size_t)cnt, true, true, W, H) + 256;
}

// spill workspace of a call: lists that can outgrow the LDS tier get theirs up front (bounded; a pool that still runs out is grown
// by the re-run)
static size_t spill_pool(const trl_ctx* c, int n, int H, int W) {
    const LvLayout& G = c->cb.lay;
    const int lds_full = c->opt.nms_full;
    size_t spill = c->caps.spill_hint;
    size_t per_frame = 0;
    for (int l = 0; l < G.L; l++) if (G.capl[l] > lds_full) per_frame += spill_need(G.capl[l], W, H);
    if (c->cb.capF > lds_full) per_frame += 3 * spill_need(c->cb.capF, W, H);
    size_t up_front = per_frame * (size_t)n;
    if (up_front > (8ull << 30)) up_front = 8ull << 30;
    if (up_front > spill) spill = up_front;
    return spill;
}

// How the list kernels (k_nms_level, k_nms_frame, k_stage2_post, k_stage3_post) are launched for the layout in c->cb: LDS tiers,
// workgroup sizes, dynamic LDS.  One place for the cascade and the list test hook (trl_cascade_lists).
struct ListLaunch {
    int small_cap, full_l, full_f, max_capl, th_l, th_f;
    size_t sm_s, sm_l, sm_f;
};
static int list_launch(trl_ctx* c, ListLaunch& ll) {
    const LvLayout& G = c->cb.lay;
    const int capF = c->cb.capF;
    const int lds_full = c->opt.nms_full, lds_small = c->opt.nms_small < c->opt.nms_full ? c->opt.nms_small : c->opt.nms_full;
    // LDS tiers: no list is longer than its capacity, so the carve never exceeds what the call can produce
    int max_capl = 4;
    for (int l = 0; l < G.L; l++) if (G.capl[l] > max_capl) max_capl = G.capl[l];
    ll.max_capl = max_capl;
    ll.full_l = max_capl < lds_full ? max_capl : lds_full;
    ll.full_f = capF < lds_full ? capF : lds_full;
    // lists that can take the spill tier run with 1024 threads per workgroup: its cost is pair tests (candidates x boxes kept so far)
    ll.th_l = max_capl > lds_full ? 1024 : 256;
    ll.th_f = capF > lds_full ? 1024 : 256;
    ll.sm_l = Smem::bytes(ll.full_l, ll.th_l);
    ll.sm_f = Smem::bytes(ll.full_f, ll.th_f);
    ll.small_cap = ll.full_l < lds_small ? ll.full_l : lds_small;
    ll.sm_s = Smem::bytes(ll.small_cap);
    TRL_CHECK(set_dyn_smem(k_nms_level, ll.sm_l));
    TRL_CHECK(set_dyn_smem(k_nms_frame, ll.sm_f));
    TRL_CHECK(set_dyn_smem(k_stage2_post, ll.sm_f));
    TRL_CHECK(set_dyn_smem(k_stage3_post, ll.sm_f));
    return TRL_OK;
}
// stage 1 after PNet: per (frame, level) batched_nms(0.5) in the small and the full tier, then per frame NMS 0.7 + regression
static int launch_stage1_lists(trl_ctx* c, const ListLaunch& ll, int n, int H, int W, const Spill& sp, hipStream_t s) {
    CascadeBufs& B = c->cb;
    const LvLayout& G = B.lay;
    const int L = G.L;
    k_nms_level<<<n * L, 256, ll.sm_s, s>>>(G, ll.small_cap, 0, ll.small_cap == ll.max_capl ? 1 : 0, W, H, B.lvl_cnt, B.lvl_rec, B.lvl_keep_cnt, B.lvl_keep_idx, B.flags, sp);
    TRL_LAUNCH_CHECK();
    if (ll.small_cap < ll.max_capl) {
        k_nms_level<<<n * L, ll.th_l, ll.sm_l, s>>>(G, ll.full_l, ll.small_cap + 1, 1, W, H, B.lvl_cnt, B.lvl_rec, B.lvl_keep_cnt, B.lvl_keep_idx, B.flags, sp);
        TRL_LAUNCH_CHECK();
    }
    k_nms_frame<<<n, ll.th_f, ll.sm_f, s>>>(G, ll.full_f, B.capF, W, H, B.lvl_rec, B.lvl_keep_cnt, B.lvl_keep_idx, B.cnt[0], B.box[0], B.flags, sp);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
// Stages 2 and 3, described once: the net (trl_net_of), its threshold, and the launch of its tail kernel over the net's outputs
// out [cap][nout] (candidate off[st][f] + i = row i of frame f).  Stage st + 2 reads the lists of index st and writes those of
// st + 1; its flag slot is st (k_scan_counts) and its batch capacity c->caps.cap_t[st].
struct StageDesc {
    int net;
    float trl_config::*thr;
    void (*post)(const CascadeBufs& B, const ListLaunch& ll, int cap, float thr, const float* out, const Spill& sp, hipStream_t s);
};
static const StageDesc trl_stages[2] = {
    {24, &trl_config::thr1, [](const CascadeBufs& B, const ListLaunch& ll, int cap, float thr, const float* out, const Spill& sp, hipStream_t s) {
         k_stage2_post<<<B.n, ll.th_f, ll.sm_f, s>>>(ll.full_f, B.capF, cap, B.W, B.H, thr, B.cnt[0], B.box[0], B.off[0], out, B.cnt[1], B.box[1], sp);
     }},
    {48, &trl_config::thr2, [](const CascadeBufs& B, const ListLaunch& ll, int cap, float thr, const float* out, const Spill& sp, hipStream_t s) {
         k_stage3_post<<<B.n, ll.th_f, ll.sm_f, s>>>(ll.full_f, B.capF, cap, thr, B.cnt[1], B.box[1], B.off[1], out, B.cnt[2], B.box[2], B.pts3, sp);
     }},
};
// the batch of stage st + 2: the exclusive scan of its input counts, its total and whether it fits `cap` (flag slot st)
static int launch_stage_scan(const CascadeBufs& B, int st, int cap, hipStream_t s) {
    k_scan_counts<<<1, 256, 0, s>>>(B.cnt[st], B.n, B.off[st], cap, B.flags, st);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}
static int launch_stage_post(trl_ctx* c, const ListLaunch& ll, int st, int cap, const float* out, const Spill& sp, hipStream_t s) {
    trl_stages[st].post(c->cb, ll, cap, c->cfg.*trl_stages[st].thr, out, sp, s);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

// The cascade's blocks for B's geometry (n, L, lay, capF) and a spill pool of `spill` bytes: the lists, then k_select's per-frame
// outputs.  One layout for the cascade and the list hook (trl_cascade_lists)
static void layout_lists(CascadeBufs& B, Arena& A, size_t spill) {
    const LvLayout& G = B.lay;
    const int n = B.n, L = B.L, capF = B.capF;
    A.reset("lists");
    B.lvl_cnt = (int32_t*)A.alloc((size_t)n * L * 4);
    B.lvl_keep_cnt = (int32_t*)A.alloc((size_t)n * L * 4);
    B.lvl_rec = (Cand*)A.alloc((size_t)n * G.S * sizeof(Cand));
    B.lvl_keep_idx = (int32_t*)A.alloc((size_t)n * G.S * 4);
    for (int k = 0; k < 3; k++) B.cnt[k] = (int32_t*)A.alloc((size_t)n * 4);
    for (int k = 0; k < 3; k++) B.box[k] = (float*)A.alloc((size_t)n * capF * 20);
    B.pts3 = (float*)A.alloc((size_t)n * capF * 40);
    for (int k = 0; k < 2; k++) B.off[k] = (int32_t*)A.alloc((size_t)(n + 1) * 4);
    B.cbox = (int32_t*)A.alloc((size_t)n * capF * 32);
    B.flags = (int32_t*)A.alloc(TRL_NFLAGS * 4);
    B.pq = (char*)trl_defer_carve(A, B.pq_cap);
    B.spill = spill ? (char*)A.alloc(spill) : nullptr;
    B.spill_cap = B.spill ? spill : 0;
    B.box0 = (float*)A.alloc((size_t)n * 16); B.prob0 = (float*)A.alloc((size_t)n * 4);
    B.rect = (int32_t*)A.alloc((size_t)n * 16); B.valid = (uint8_t*)A.alloc((size_t)n);
    B.pts0 = (float*)A.alloc((size_t)n * 40);
}
// ... carved from c->arena (live for the whole call, and for the debug hooks after it) for the layout in c->cb, flags zeroed
static int carve_lists(trl_ctx* c, size_t spill, hipStream_t s) {
    CascadeBufs& B = c->cb;
    Arena count = Arena::counter(c->arena.guard);
    layout_lists(B, count, spill);
    TRL_CHECK(trl_ensure(c, c->arena, c->arena_need = count.off));
    layout_lists(B, c->arena, spill);
    if (c->arena.off != c->arena_need) { trl_set_error("cascade workspace allocation failed"); return TRL_ERR_STATE; }
    TRL_HIP(hipMemsetAsync(B.flags, 0, TRL_NFLAGS * 4, s));
    return TRL_OK;
}

int trl_pnet_generic_level(trl_ctx* c, Arena& X, const uint8_t* d_frames, int nf, int H, int W, const LevelGeom& g, float** d_heads, hipStream_t s) {
    X.reset("pnet_level");
    float* lvl = (float*)X.alloc((size_t)nf * g.h * g.w * 12);
    float* heads = (float*)X.alloc((size_t)nf * g.oh * g.ow * 24);
    if (!lvl || !heads) { trl_set_error("pnet generic workspace"); return TRL_ERR_STATE; }
    if (!X.counting) TRL_CHECK(trl_launch_area_level(d_frames, nf, H, W, g.h, g.w, lvl, s));
    TRL_CHECK(trl_run_net(c, X, trl_nets[TRL_PNET], 0, Act::dense(lvl, nf, g.h, g.w, 3), heads, s));   // heads [nf][oh][ow][6]
    *d_heads = heads;
    return TRL_OK;
}

// the next (start, end) event pair of the call's PNet launches (pointers into c->pnet_ev: the fused path reserves it first)
static int next_pnet_events(trl_ctx* c, std::pair<hipEvent_t, hipEvent_t>*& out) {
    if ((int)c->pnet_ev.size() <= c->pnet_ev_used) {
        hipEvent_t e0, e1;
        TRL_HIP(hipEventCreate(&e0)); TRL_HIP(hipEventCreate(&e1));
        c->pnet_ev.push_back({e0, e1});
    }
    out = &c->pnet_ev[c->pnet_ev_used++];
    return TRL_OK;
}

// stage 2 / 3 carves X from its start (stream order: the stage in front is done with it): *d_out = [cap][nout], then trl_stage_net's
static int stage_carve(trl_ctx* c, Arena& X, int net, const uint8_t* d_frames, int H, int W, const int32_t* d_total, int cap, float** d_out, hipStream_t s) {
    const NetDesc& d = trl_net_of(net);
    X.reset("stage_carve");
    *d_out = (float*)X.alloc((size_t)cap * d.nout * 4);
    if (!*d_out) { trl_set_error("%s workspace", d.name); return TRL_ERR_STATE; }
    return trl_stage_net(c, X, net, d_frames, H, W, d_total, cap, *d_out, s);
}

// ONE scratch workspace big enough for every stage at this attempt's batch capacities: it is only ever grown here, before
// anything of the call is queued (growing frees the old block)
static int size_scratch(trl_ctx* c, int n, int H, int W, bool fused) {
    // one counting arena under all that carves the scratch in turn (each from a reset): its high-water mark is the call's need
    Arena X = Arena::counter(c->scratch.guard);
    X.high = std::max(c->scratch_after_cascade, fused ? trl_pnet_fused_bytes(c, n, H, W) + (1u << 20) : 0);
    float* o;
    for (int l = 0; l < c->cb.L && !fused; l++) {
        LevelGeom& g = c->lv[l];
        if (g.oh < 1 || g.ow < 1) continue;
        TRL_CHECK(trl_pnet_generic_level(c, X, nullptr, 1, 0, 0, g, &o, nullptr));
        g.chunk = (int)std::min<size_t>(n, std::max<size_t>(1, (size_t)(2048ull << 20) / X.off));
        TRL_CHECK(trl_pnet_generic_level(c, X, nullptr, g.chunk, 0, 0, g, &o, nullptr));
    }
    for (int st = 0; st < 2; st++) TRL_CHECK(stage_carve(c, X, trl_stages[st].net, nullptr, 0, 0, nullptr, c->caps.cap_t[st], &o, nullptr));
    return trl_scratch_begin(c, X.high);
}

// stage 1, fused path: pyramid kernel + ONE persistent PNet launch over every (frame, level, tile)
static int stage1_fused(trl_ctx* c, const uint8_t* d_frames, hipStream_t s) {
    const CascadeBufs& B = c->cb;
    std::pair<hipEvent_t, hipEvent_t>*pa, *pb;
    c->pnet_ev.reserve(64);   // next_pnet_events hands out pointers into the vector: no reallocation below
    TRL_CHECK(next_pnet_events(c, pa)); TRL_CHECK(next_pnet_events(c, pb));
    hipEvent_t ev[4] = {pa->first, pa->second, pb->first, pb->second};
    return trl_pnet_fused_all(c, d_frames, B.n, B.H, B.W, ev, s);
}

// stage 1, generic layer path: per level, the level materialised for a chunk of frames, PNet's layers, candidate records
static int stage1_generic(trl_ctx* c, const uint8_t* d_frames, hipStream_t s) {
    const CascadeBufs& B = c->cb;
    const LvLayout& G = B.lay;
    const int n = B.n, H = B.H, W = B.W, L = B.L;
    for (int l = 0; l < L; l++) {
        const LevelGeom& g = c->lv[l];
        if (g.oh < 1 || g.ow < 1) continue;
        std::pair<hipEvent_t, hipEvent_t>* pe;
        TRL_CHECK(next_pnet_events(c, pe));
        TRL_HIP(hipEventRecord(pe->first, s));
        const int chunk = g.chunk;
        for (int f0 = 0; f0 < n; f0 += chunk) {
            const int nf = (n - f0 < chunk) ? n - f0 : chunk;
            float* heads;
            TRL_CHECK(trl_pnet_generic_level(c, c->scratch, d_frames + (size_t)f0 * H * W * 3, nf, H, W, g, &heads, s));
            const size_t total = (size_t)nf * g.oh * g.ow;
            size_t blocks = (total + 255) / 256;
            if (blocks > 16384) blocks = 16384;
            k_pnet_collect<<<(unsigned)blocks, 256, 0, s>>>(heads, nf, f0, g.oh, g.ow, (float)g.scale, c->cfg.thr0, L, l, G.capl[l],
                                                             G.rec0[l], G.S, B.lvl_cnt, B.lvl_rec, B.flags);
            TRL_LAUNCH_CHECK();
        }
        TRL_HIP(hipEventRecord(pe->second, s));
    }
    return TRL_OK;
}

// Stage st + 2: R-Net over the stage-1 boxes / O-Net over the stage-2 boxes, then its tail.  No host round trip: the candidate
// total stays on the device (off[st][n]).  Launches are sized by an optimistic capacity (c->caps.cap_t[st], from earlier calls) and
// workgroups past the real total exit at once; if the total exceeds the capacity a flag is raised and the call is re-run with a
// larger one (trl_cascade_check).
static int stage_net_and_post(trl_ctx* c, int st, const ListLaunch& ll, const uint8_t* d_frames, const Spill& sp, hipStream_t s) {
    const CascadeBufs& B = c->cb;
    const int n = B.n, H = B.H, W = B.W, cap = c->caps.cap_t[st];
    TRL_CHECK(launch_stage_scan(B, st, cap, s));
    k_build_map<<<n, 64, 0, s>>>(B.cnt[st], B.off[st], B.box[st], B.capF, W, H, B.cbox);
    TRL_LAUNCH_CHECK();
    float* out;
    TRL_CHECK(stage_carve(c, c->scratch, trl_stages[st].net, d_frames, H, W, B.off[st] + n, cap, &out, s));
    return launch_stage_post(c, ll, st, cap, out, sp, s);
}

// detect_face() stages 1-3 for n frames; results stay in c->cb
// `resume` = 2 / 3: re-run of a call whose R-Net / O-Net batch capacity was too small -- everything up to that stage is intact in
// the cascade arena (the lists, the stage boxes, the counts), so the attempt starts at stage 2 / 3 instead of at the pyramid.
int trl_cascade_detect(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, hipStream_t s, int resume) {
    const int L = trl_compute_levels(c, H, W);
    CascadeBufs& B = c->cb;
    if (resume >= 2 && !(B.flags && B.n == n && B.L == L && B.H == H && B.W == W && L > 0)) resume = 0;   // nothing to resume from
    B.n = n; B.L = L; B.H = H; B.W = W;
    plan_caps(c, L, n);   // (a resumed attempt plans the lists it has: the check behind the last one raised a batch hint only)
    const size_t spill = spill_pool(c, n, H, W);
    if (resume) {
        // the stages that run again report afresh (the stage-2 total of a resume at stage 3 stays: it is complete)
        for (int st = resume - 2; st < 2; st++) {
            TRL_HIP(hipMemsetAsync(B.flags + FLG_T2 + st, 0, 4, s));
            TRL_HIP(hipMemsetAsync(B.flags + FLG_T2N + st, 0, 4, s));
        }
    } else {
        TRL_CHECK(carve_lists(c, spill, s));
    }
    const Spill sp{B.spill, (unsigned long long)B.spill_cap, B.flags};
    if (L == 0) {
        // min(H, W) * 12 / min_face_size < 12: detect_face() builds no scale at all and returns no boxes (the frame is smaller
        // than the smallest face looked for).  Every stage count is zero; k_select then reports "no face" for every frame.
        for (int k = 0; k < 3; k++) TRL_HIP(hipMemsetAsync(B.cnt[k], 0, (size_t)n * 4, s));
        for (int k = 0; k < 2; k++) TRL_HIP(hipMemsetAsync(B.off[k], 0, (size_t)(n + 1) * 4, s));
        TRL_CHECK(trl_scratch_begin(c, c->scratch_after_cascade));   // the crops + embedder of the same call
        return TRL_OK;
    }
    if (!resume) {
        TRL_HIP(hipMemsetAsync(B.lvl_cnt, 0, (size_t)n * L * 4, s));
        c->pnet_ev_used = 0;
    }
    const bool fused = pnet_is_fused(c, L);
    TRL_CHECK(size_scratch(c, n, H, W, fused));
    if (!resume) TRL_CHECK(fused ? stage1_fused(c, d_frames, s) : stage1_generic(c, d_frames, s));
    ListLaunch ll;
    TRL_CHECK(list_launch(c, ll));
    if (!resume) TRL_CHECK(launch_stage1_lists(c, ll, n, H, W, sp, s));
    for (int st = resume ? resume - 2 : 0; st < 2; st++) TRL_CHECK(stage_net_and_post(c, st, ll, d_frames, sp, s));
    return TRL_OK;
}

// One R-Net (net = 24) or O-Net (net = 48) stage over `cap` candidate slots: chunks of c->opt.rnet_chunk / c->opt.onet_chunk candidates,
// each the fused front kernel (crop of record t0 + i of c->cb.cbox, conv1, pool1 in LDS) then the layer tail.  Launches are sized
// by the capacity; the candidates that exist are the first *d_total, and every kernel skips the rest on the device.  The pooled
// maps come from X behind its current offset (the caller's blocks below it stay intact).  d_out: [cap][6] / [cap][16].  Over a
// counting X one chunk is walked: the first is the largest.
int trl_stage_net(trl_ctx* c, Arena& X, int net, const uint8_t* d_frames, int H, int W, const int32_t* d_total, int cap, float* d_out, hipStream_t s) {
    const NetDesc& d = trl_net_of(net);
    const int CH = c->opt.*d.chunk;
    const size_t mk = X.off;
    for (int t0 = 0; t0 < cap; t0 += CH) {
        const int nc = (cap - t0 < CH) ? cap - t0 : CH;
        X.rewind(mk, "chunk");
        float* pool1 = (float*)X.alloc((size_t)nc * d.P * d.P * d.C1 * 4);
        if (!pool1) { trl_set_error("%s workspace", d.name); return TRL_ERR_STATE; }
        if (!X.counting) TRL_CHECK(trl_launch_front(c, d, d_frames, H, W, d_total, t0, nc, pool1, s));   // crop + conv1 + pool1 in LDS
        TRL_CHECK(trl_run_net(c, X, d, d.tail, Act::dense(pool1, nc, d.P, d.P, d.C1), d_out + (size_t)t0 * d.nout, s, d_total, t0));
        if (X.counting) break;
    }
    return TRL_OK;
}

int trl_cascade_finish(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_boxes, float* d_probs, float* d_points,
                       int32_t* d_counts, float* d_box0, float* d_prob0, int32_t* d_rect, uint8_t* d_valid, float* d_pts0, hipStream_t s,
                       int order) {
    (void)d_frames;
    CascadeBufs& B = c->cb;
    k_select<<<n, 64, 0, s>>>(B.capF, c->cfg.max_faces, W, H, order, B.cnt[2], B.box[2], B.pts3, d_boxes, d_probs, d_points, d_counts, d_box0, d_prob0,
                              d_rect, d_valid, d_pts0);
    TRL_LAUNCH_CHECK();
    // overflow flags + stage totals travel to pinned host memory behind the kernels; trl_cascade_check reads them after the
    // call's ONE stream synchronisation (no host round trip inside the call)
    TRL_HIP(hipMemcpyAsync(trl_host_flags(c), B.flags, TRL_NFLAGS * 4, hipMemcpyDeviceToHost, s));
    return TRL_OK;
}

// After the stream has been synchronised.  *retry = 1 when a capacity of this attempt was too small -- a level's record list, a
// frame's box list, the spill workspace, or the optimistic R-/O-Net batch -- : the capacities have been raised to what the
// attempt measured and the caller runs the call again (results of the attempt are incomplete, not wrong-but-plausible, and are
// never delivered).  No input can make this fail: detect_face() (server/model.py:47) has no candidate limit.
int trl_cascade_check(trl_ctx* c, int n, int* retry) {
    *retry = trl_caps_check(c->caps, trl_host_flags(c), n, c->cb.lay).retry;
    return TRL_OK;
}

// test hook behind trl_debug_lists: the list kernels on lists the caller provides, in the cascade's own layout (carve_lists),
// launched by its own code (list_launch, launch_stage1_lists / launch_stage_scan / launch_stage_post, trl_cascade_finish) with
// its spill pool and overflow flags.  kind 1: h_rows = Cand records of every (frame, level), frame-major, h_counts [n][L]; kind 2: stage-1 rows
// (x1, y1, x2, y2, score) of every frame, h_counts [n], h_logits the R-Net outputs [total][6]; kind 3: stage-2 rows, h_logits the
// O-Net outputs [total][16], then k_select into the d_* outputs and the stage-3 landmarks into h_pts [n][capF][10] (nullable).
// h_caps = the L level capacities, then capF.  Every slot the inputs do not fill holds the poison byte of trl_debug_poison (0xA5
// without one).  The lists stay in c->cb for the inspection hooks (trl_debug_level_keep, trl_debug_stage_boxes).
int trl_cascade_lists(trl_ctx* c, int kind, int n, int H, int W, const int32_t* h_caps, int L, const int32_t* h_counts, const void* h_rows,
                      const float* h_logits, float* h_pts, float* d_boxes, float* d_probs, float* d_points, int32_t* d_counts, float* d_box0,
                      float* d_prob0, int32_t* d_rect, uint8_t* d_valid, hipStream_t s) {
    CascadeBufs& B = c->cb;
    B = CascadeBufs();
    c->caps.defer.cap = 0;                                // (no PNet launch, no confirm queue)
    LvLayout& G = B.lay;
    G.L = L;
    for (int l = 0; l < L; l++) { G.capl[l] = h_caps[l]; G.rec0[l] = G.S; G.S += h_caps[l]; }
    B.capF = h_caps[L];
    B.n = n; B.L = L; B.H = H; B.W = W;
    const int capF = B.capF, nc = kind == 1 ? n * L : n;
    long long total = 0;
    for (int i = 0; i < nc; i++) total += h_counts[i];
    const int carved = carve_lists(c, spill_pool(c, n, H, W), s);
    if (carved != TRL_OK) { B = CascadeBufs(); return carved; }
    const int poison = c->hook.dbg_poison >= 0 ? c->hook.dbg_poison : 0xA5;
    TRL_HIP(hipMemsetAsync(c->arena.base, poison, (size_t)((char*)B.flags - c->arena.base), s));   // every list (the flags stay zero)
    // the caller's lists, packed, into the capacity layout; the poison stays in the slots behind the counts
    std::vector<int32_t> cnt(h_counts, h_counts + nc);
    std::vector<float> logits;
    const int st = kind - 2;                              // kinds 2 / 3: the stage's index (trl_stages)
    const int NO = kind == 1 ? 0 : trl_net_of(trl_stages[st].net).nout;
    if (kind == 1) {
        const Cand* src = (const Cand*)h_rows;
        TRL_HIP(hipMemcpyAsync(B.lvl_cnt, cnt.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s));
        for (int f = 0; f < n; f++)
            for (int l = 0; l < L; l++) {
                const int k = cnt[f * L + l];
                if (k) TRL_HIP(hipMemcpyAsync(B.lvl_rec + (size_t)f * G.S + G.rec0[l], src, (size_t)k * sizeof(Cand), hipMemcpyHostToDevice, s));
                src += k;
            }
    } else {
        const float* src = (const float*)h_rows;
        float* rows = B.box[st];
        TRL_HIP(hipMemcpyAsync(B.cnt[st], cnt.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
        for (int f = 0; f < n; f++) {
            if (cnt[f]) TRL_HIP(hipMemcpyAsync(rows + (size_t)f * capF * 5, src, (size_t)cnt[f] * 20, hipMemcpyHostToDevice, s));
            src += 5 * (size_t)cnt[f];
        }
        logits.assign(h_logits, h_logits + (size_t)total * NO);
    }
    TRL_HIP(hipStreamSynchronize(s));                     // (host vectors)
    const Spill sp{B.spill, (unsigned long long)B.spill_cap, B.flags};
    ListLaunch ll;
    TRL_CHECK(list_launch(c, ll));
    if (kind == 1) {
        TRL_CHECK(launch_stage1_lists(c, ll, n, H, W, sp, s));
    } else {
        // the net outputs: [cap][NO] in the scratch arena, cap = the candidate total (+ 64 poisoned rows behind it)
        const int cap = (int)total + 64;
        Arena& X = c->scratch;
        TRL_CHECK(trl_scratch_begin(c, (size_t)cap * NO * 4 + (1u << 20)));
        float* out = (float*)X.alloc((size_t)cap * NO * 4);
        if (!out) { trl_set_error("list hook net outputs"); return TRL_ERR_STATE; }
        TRL_HIP(hipMemsetAsync(out, poison, (size_t)cap * NO * 4, s));
        if (total) TRL_HIP(hipMemcpyAsync(out, logits.data(), logits.size() * 4, hipMemcpyHostToDevice, s));
        TRL_CHECK(launch_stage_scan(B, st, cap, s));
        TRL_CHECK(launch_stage_post(c, ll, st, cap, out, sp, s));
        if (kind == 3) {
            TRL_CHECK(trl_cascade_finish(c, nullptr, n, H, W, d_boxes, d_probs, d_points, d_counts, d_box0, d_prob0, d_rect, d_valid, nullptr, s));
        }
        TRL_HIP(hipStreamSynchronize(s));                 // (the logits vector)
    }
    if (kind != 3) TRL_HIP(hipMemcpyAsync(trl_host_flags(c), B.flags, TRL_NFLAGS * 4, hipMemcpyDeviceToHost, s));
    if (kind == 3 && h_pts) TRL_HIP(hipMemcpyAsync(h_pts, B.pts3, (size_t)n * capF * 40, hipMemcpyDeviceToHost, s));
    TRL_HIP(hipStreamSynchronize(s));
    c->caps.last_attempts = 1;
    const int32_t* fl = trl_host_flags(c);
    if (fl[FLG_LEVEL] || fl[FLG_FRAME] || fl[FLG_SPILL]) {
        trl_set_error("list hook: a capacity was too small (level %d, frame %d, spill %d)", fl[FLG_LEVEL], fl[FLG_FRAME], fl[FLG_SPILL]);
        return TRL_ERR_CAPACITY;
    }
    return TRL_OK;
}

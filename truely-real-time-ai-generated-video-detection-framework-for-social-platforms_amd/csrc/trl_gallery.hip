// trl_gallery.hip -- embedding match (DESIGN section 7, f-7 .. f-11): a gallery of enrolled 512-float embeddings on the device and
// every kernel that scores query rows against it on the matrix cores.
//
// The gallery is k-major, [512][ld] f32 with ld a multiple of 32 and zero padding, plus n2[ld] -- the loader's layout of
// facenet.logits.w, and for the reason trl_logits.hip gives: lane l's B operand of v_mfma_f32_32x32x2_f32 is one dword of a whole
// 128-byte line, so the gallery goes from memory into the matrix core without touching LDS.  The main loop is k_logits' with a
// zero bias: a workgroup holds a row tile of 32 queries in LDS ([32][514] words), a wave takes a SLAB of 32 gallery columns at a
// time, the columns stream through a three-deep register ring, and every output is ONE accumulator over ascending k:
//     dot(q, g) = chain(0; k = 0..511: acc = fmaf(q[k], g[k], acc))                         
// n2(x) = dot(x, x) is the same chain, taken once per gallery row at enrolment (k_gallery_pack) and once per query row per
// workgroup (gl_fill_tile).  A slab's 16 accumulators per lane become scores (gl_score):
//     cosine      dot / (sqrtf(n2 q) * sqrtf(n2 g))
//     euclidean   s = n2 q + n2 g;  d2 = fmaf(-2, dot, s);  d2 < 0 ? 0 : d2;  sqrtf(d2)
// Scores do not depend on n, tile, strip or launch geometry (one chain per output), so neither does any result below.
//
// THE WALK: workgroup x = strip * tiles + tile (the row tile is the fast index: workgroups in flight share a few column groups in L2)
// fills its tile and walks a STRIP of gps column groups of 128; of each group wave w takes slab w.  Nothing crosses waves inside a
// strip, so the loop over slabs holds no barrier.  GlFrame (LDS carve, grid decode), gl_slab / GlSlab::rows (chain, column info, the
// C/D row decode, the score) and gl_walk carry it for the kernels that measured no slower on them than on their own text
// (profiles/gallery_refactor_timing.txt); the kernel hands the walk its ENDING, a functor that receives one slab:
//   k_gallery_scores        no strip: one slab per wave, stored (rows < n, columns < m)
//   k_gallery_search        the k best matches per row: the scores go through a wave-private LDS stage, lane l walks row l & 31 over
//     [_groups]             16 of the 32 columns against a list of its own (trl_gallery_order.h), the workgroup merges its eight lists
//                           per row and k_gallery_merge[_groups] the strips; with group ids (f-11) a list holds distinct groups
// k_gallery_links, k_gallery_hist and the range search's rg_walk measured 0.6 - 0.8 % slower on the shared pieces and keep the same
// walk in their own text (the decode and the h barrier are those of gl_slab -- change them together):
//   k_gallery_links  (f-8)  the ballot of the link predicate is two finished words of the n x n bitmap; trl_cluster.hip labels it
//   k_gallery_hist   (f-9)  every score is put into its bin and counted in LDS, genuine and impostor apart; k_gallery_hist_sum adds
//                           the workgroups' counters
//   k_gallery_range_count / _fill (f-10)  the ballot ends in popcounts per row, then in ranked stores of CSR lists; here wave w walks a
//                           contiguous quarter of the strip (rg_walk), and k_range_rows / k_range_scan turn counts into offsets
// The entry points refuse, find their device, check their workspace and launch the tile kernels through trl_host.h.
#include <algorithm>
#include <utility>

#include "trl_cluster.h"
#include "trl_host.h"
#include "trl_gallery_bins.h"
#include "trl_gallery_groups.h"
#include "trl_gallery_order.h"
#include "trl_scan.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GL_K = 512;             // floats per embedding
constexpr int GL_LDF = GL_K + 2;      // LDS row pitch in words (trl_logits.hip: 64 lanes of an A read on 64 banks)
constexpr int GL_ROWS = 32;           // query rows of a tile
constexpr int GL_CHUNK = 32;          // k-steps (of 2) per ring slot
constexpr int GL_NCHUNK = GL_K / 2 / GL_CHUNK;
constexpr int GL_GROUP = 128;         // gallery columns of a workgroup's step: 32 per wave
constexpr int GL_TILE_WORDS = GL_ROWS * GL_LDF;
constexpr int GL_INFO_WORDS = 3 * GL_ROWS;   // per row: n2, sqrtf(n2), and whether the row exists and is valid
constexpr int GL_TARGET_WGS = 512;    // workgroups wanted: two rounds of one per CU on 256 CUs
constexpr int GL_MAX_STRIPS = 512;    // of the default plan
constexpr int GL_STAGE_WORDS = GL_ROWS * 33;   // a wave's 32 x 32 scores, rows 33 words apart
constexpr int GG_STAGE_WORDS = GL_STAGE_WORDS + GL_ROWS;   // the same, then the slab's 32 group ids
constexpr int GL_LISTS = 8;           // lists per query row in a workgroup: two per wave

template <int... I, typename F>
__device__ __forceinline__ void gl_static_for(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}

// rows row0 .. row0 + 31 of q -> tile (rows past n as zeros), and their n2 / sqrtf(n2) / live flag -> info.  Ends on a barrier.
__device__ __forceinline__ int gl_fill_tile(float* tile, float* info, const float* __restrict__ q, const uint8_t* __restrict__ valid,
                                            int n, long long row0, int tid) {
    const int live = n - row0 < GL_ROWS ? (int)(n - row0) : GL_ROWS;
    const float* src = q + (size_t)row0 * GL_K;
    if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {
#pragma unroll 4
        for (int t = tid; t < GL_ROWS * GL_K / 4; t += 256) {
            const int r = t >> 7, c = t & 127;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < live) v = *reinterpret_cast<const float4*>(src + (size_t)r * GL_K + 4 * c);
            float2* d = reinterpret_cast<float2*>(tile + r * GL_LDF + 4 * c);      // (rows are 8-byte aligned: 514 words)
            d[0] = make_float2(v.x, v.y);
            d[1] = make_float2(v.z, v.w);
        }
    } else {
#pragma unroll 4
        for (int t = tid; t < GL_ROWS * GL_K; t += 256) {
            const int r = t >> 9, k = t & 511;
            tile[r * GL_LDF + k] = r < live ? src[(size_t)r * GL_K + k] : 0.f;
        }
    }
    __syncthreads();
    if (tid < GL_ROWS) {
        const float* x = tile + tid * GL_LDF;
        float acc = 0.f;
#pragma unroll 16
        for (int k = 0; k < GL_K; k++) acc = __builtin_fmaf(x[k], x[k], acc);
        info[tid] = acc;
        info[GL_ROWS + tid] = __builtin_sqrtf(acc);
        reinterpret_cast<int*>(info)[2 * GL_ROWS + tid] = tid < live && (!valid || valid[row0 + tid] != 0);
    }
    __syncthreads();
    return live;
}

// One wave: the 32 x 32 dots of the tile's rows against gallery columns c0 .. c0 + 31 (c0 + 31 < ld).  C/D map of the 32x32
// forms: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5).
__device__ __forceinline__ f32x16 gl_chain(const float* tile, const float* __restrict__ mat, size_t ld, long long c0, int lane) {
    const int j = lane & 31, h = lane >> 5;
    const float* wp = mat + (size_t)h * ld + c0 + j;
    const float* xp = tile + j * GL_LDF + h;
    const size_t step = 2 * ld;
    float wb[3][GL_CHUNK], xa[2][GL_CHUNK];
    // a ring slot's 32 k-rows are addressed from the slot's own base, which the compiler is kept from folding back into
    // 256 multiples of ld: inside a loop over column groups those would be hoisted into more registers than there are
    auto load_w = [&](int ch, float* o) __attribute__((always_inline)) {
        const float* base = wp + (size_t)(ch * GL_CHUNK) * step;
        asm volatile("" : "+v"(base));
#pragma unroll
        for (int u = 0; u < GL_CHUNK; u++) o[u] = base[(size_t)u * step];
    };
    auto load_x = [&](int ch, float* o) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < GL_CHUNK; u++) o[u] = xp[2 * (ch * GL_CHUNK + u)];
    };
    load_w(0, wb[0]);
    load_w(1, wb[1]);
    load_x(0, xa[0]);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    gl_static_for(std::make_integer_sequence<int, GL_NCHUNK>{}, [&](auto CH) __attribute__((always_inline)) {
        constexpr int ch = decltype(CH)::value;
        if constexpr (ch + 2 < GL_NCHUNK) load_w(ch + 2, wb[(ch + 2) % 3]);
        if constexpr (ch + 1 < GL_NCHUNK) load_x(ch + 1, xa[(ch + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < GL_CHUNK; u++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[ch & 1][u], wb[ch % 3][u], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    });
    return acc;
}

__device__ __forceinline__ float gl_score(int metric, float dot, float qn2, float qsq, float gn2, float gsq) {
    if (metric == TRL_GL_COSINE) return dot / (qsq * gsq);
    const float s = qn2 + gn2;
    float d2 = __builtin_fmaf(-2.0f, dot, s);
    d2 = d2 < 0.f ? 0.f : d2;                           // (NaN stays NaN)
    return __builtin_sqrtf(d2);
}

// whether tile row r exists and is valid
__device__ __forceinline__ bool gl_rowok(const float* info, int r) { return reinterpret_cast<const int*>(info)[2 * GL_ROWS + r] != 0; }

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
// A tile kernel's workgroup: its dynamic LDS -- `front` words the kernel wants in front, the tile, the row info (gl_fill_tile),
// then `rest`, the kernel's own -- and its place in the grid, x = strip * tiles + tile.  gl_lds_bytes is the size the host passes for
// every tile kernel, also for those that carve by hand.
struct GlFrame {
    float *front, *tile, *info;
    float* rest;
    int tid, lane, wave;
    long long row0, strip;
    __device__ __forceinline__ explicit GlFrame(int tiles, int front_words = 0) {
        extern __shared__ float gl_lds[];
        front = gl_lds;
        tile = gl_lds + front_words;
        info = tile + GL_TILE_WORDS;
        rest = info + GL_INFO_WORDS;
        tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)tiles;
    }
};

constexpr size_t gl_lds_bytes(size_t rest_bytes = 0, int front_words = 0) {
    return (size_t)(front_words + GL_TILE_WORDS + GL_INFO_WORDS) * 4 + rest_bytes;
}

// One slab: a wave's chain against columns c0 .. c0 + 31 and what its lane needs to turn accumulators into scores.  Lane l holds
// column c0 + j, j = l & 31, and in accumulator i row r = (i & 3) + 8 (i >> 2) + 4 h, h = l >> 5.  h is made here, behind the chain:
// the 16 rows' LDS addresses are computed per slab, not kept in registers across the chain.
struct GlSlab {
    f32x16 acc;
    long long c0, col;
    float g2, gs;
    int j, h;
    // f(i, r, score) for the lane's 16 accumulators, i a constant after unrolling; `metric` an int or a std::integral_constant
    template <typename Metric, typename F>
    __device__ __forceinline__ void rows(Metric metric, const float* info, F&& f) const {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
            f(i, r, gl_score(metric, acc[i], info[r], info[GL_ROWS + r], g2, gs));
        }
    }
};

__device__ __forceinline__ GlSlab gl_slab(const float* tile, const float* __restrict__ mat, size_t ld, const float* __restrict__ gn2,
                                          long long c0, int lane) {
    GlSlab s;
    s.acc = gl_chain(tile, mat, ld, c0, lane);
    s.c0 = c0;
    s.j = lane & 31;
    s.col = c0 + s.j;
    s.g2 = gn2[s.col];                                   // (col < ld: n2 has ld entries)
    s.gs = __builtin_sqrtf(s.g2);
    int h = lane >> 5;
    asm volatile("" : "+v"(h));
    s.h = h;
    return s;
}

// The loop over a wave's slabs: end(slab) for the slabs at first, first + step, ... in front of `last`.  first + 31 < ld wherever a
// slab is walked: `last` is at most the gallery's rows, and those at most ld, a multiple of 32.
template <typename End>
__device__ __forceinline__ void gl_walk(const GlFrame& w, const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                        long long first, long long last, int step, End&& end) {
    for (long long c0 = first; c0 < last; c0 += step) end(gl_slab(w.tile, mat, (size_t)ld, gn2, c0, w.lane));
}

// the last column group of a strip, + 1
__device__ __forceinline__ long long gl_strip_end(long long strip, long long gps, long long groups) {
    return (strip + 1) * gps < groups ? (strip + 1) * gps : groups;
}

// the walk of the group-interleaved kernels: slab `wave` of each of the column groups g_begin .. g_end - 1, as far as `cols` columns
template <typename End>
__device__ __forceinline__ void gl_walk_groups(const GlFrame& w, const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                               long long cols, long long g_begin, long long g_end, End&& end) {
    gl_walk(w, mat, ld, gn2, g_begin * GL_GROUP + w.wave * 32, g_end * GL_GROUP < cols ? g_end * GL_GROUP : cols, GL_GROUP, end);
}

__global__ __launch_bounds__(256) void k_gallery_scores(const float* __restrict__ q, int n, const float* __restrict__ mat, long long ld,
                                                        const float* __restrict__ gn2, long long m, int metric, float* __restrict__ out,
                                                        long long ldo, int tiles) {
    const GlFrame w(tiles);                              // (its strip is one column group)
    const int live = gl_fill_tile(w.tile, w.info, q, nullptr, n, w.row0, w.tid);
    const long long c0 = w.strip * GL_GROUP + w.wave * 32;
    if (c0 >= m) return;                                 // (behind the last barrier)
    const GlSlab s = gl_slab(w.tile, mat, (size_t)ld, gn2, c0, w.lane);
    if (s.col >= m) return;
    s.rows(metric, w.info, [&](int, int r, float sc) __attribute__((always_inline)) {
        if (r < live) out[(size_t)(w.row0 + r) * (size_t)ldo + s.col] = sc;
    });
}

// ---- search (f-7) and grouped search (f-11) --------------------------------------------------------------------------------------------
// Each wave keeps its own lists (two per row) and its own score stage.  A wave's 32 x 32 scores go through LDS so that each lane can
// walk ONE row's scores against its own list: a score is compared with the list's k-th entry, kept in a register, and only survivors
// are inserted -- after a strip's first groups almost none -- and the 64 lists of a wave are updated side by side.  A workgroup merges
// its eight lists per row and writes n x k entries per strip (or the result itself when there is one strip); the merge kernel merges
// the strips per row by the same order, which is total, so the result does not depend on the strips.
// GROUPS: every gallery row carries a group id (gid < 0: the row is excluded), and a list holds the best row of each of the k best
// groups seen so far (trl_gallery_groups.h: 8-byte entries as before, their groups in a parallel int32 array).  The slab's 32 ids are
// loaded like gn2 -- lane j loads gid[c0 + j], one line -- and staged behind the wave's scores.  The comparison with the list's k-th
// entry is still a valid rejection: a full list holds better rows of k distinct groups, so the newcomer is either beaten inside its
// own group or by k others.  A strip's list of its k best distinct groups is enough for the merge.  Suppose group L's globally best
// row lies in strip s and is not in strip s's list: then k other groups each have a row in strip s alone that comes before it, their
// globally best rows come before it too, and L is not among the k best groups.  So every group of the answer reaches the merge with
// its globally best row, and rows of it from other strips lose to that row in trl_gl_insert_group.  The same holds one level down for
// the eight lists of a row inside a workgroup, and one level up for the 64 lanes of the merge kernel.
// LDS: the tile, the row info, 4 stages, 8 x 32 x k entries [and groups] -- 93 KB at k = 5 plain; with groups at k = 16,
// 65,792 (tile) + 384 (info) + 17,408 (stages with ids) + 32,768 (entries) + 16,384 (groups) = 132,736 bytes.
template <bool GROUPS>
__device__ __forceinline__ void gl_search(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n, const float* __restrict__ mat,
                                          long long ld, const float* __restrict__ gn2, const int32_t* __restrict__ gid, long long m, int metric,
                                          int k, int tiles, long long gps, long long groups, TrlGlEntry* __restrict__ part,
                                          int32_t* __restrict__ part_ids, float* __restrict__ d_score, int32_t* __restrict__ d_index,
                                          int32_t* __restrict__ d_group) {
    constexpr int STAGE = GROUPS ? GG_STAGE_WORDS : GL_STAGE_WORDS;
    const GlFrame w(tiles);
    float* stage = w.rest + w.wave * STAGE;
    int32_t* ids = reinterpret_cast<int32_t*>(stage + GL_STAGE_WORDS);                          // (GROUPS)
    TrlGlEntry* lists = reinterpret_cast<TrlGlEntry*>(w.rest + 4 * STAGE);                     // (8-byte aligned: even word offset)
    int32_t* lids = reinterpret_cast<int32_t*>(lists + GL_LISTS * GL_ROWS * k);                // (GROUPS)
    // lane l keeps the list of row l & 31 over columns 16 (l >> 5) .. + 15 of each of the wave's 32-column slabs
    const int at = ((w.wave * 2 + (w.lane >> 5)) * GL_ROWS + (w.lane & 31)) * k;
    TrlGlEntry* mine = lists + at;
    int32_t* mine_ids = lids + at;
    for (int e = 0; e < k; e++) {
        mine[e] = trl_gl_empty();
        if constexpr (GROUPS) mine_ids[e] = -1;
    }
    const int live = gl_fill_tile(w.tile, w.info, q, valid, n, w.row0, w.tid);
    gl_walk_groups(w, mat, ld, gn2, m, w.strip * gps, gl_strip_end(w.strip, gps, groups), [&](const GlSlab& s) __attribute__((always_inline)) {
        [[maybe_unused]] int32_t id = -1;
        if constexpr (GROUPS) id = s.col < m ? gid[s.col] : -1;       // (gid has m entries)
        s.rows(metric, w.info, [&](int, int r, float sc) __attribute__((always_inline)) { stage[r * 33 + s.j] = sc; });
        if constexpr (GROUPS) {
            if (s.h == 0) ids[s.j] = id;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // (wave-private data: the fence orders the wave's own LDS traffic)
        __builtin_amdgcn_wave_barrier();
        if (gl_rowok(w.info, s.j)) {
            const float* sr = stage + s.j * 33 + 16 * s.h;
            const long long cb = s.c0 + 16 * s.h;
            TrlGlEntry last = mine[k - 1];
            if constexpr (!GROUPS) {
                for (int c = 0; c < 16 && cb + c < m; c++) {
                    const float sc = sr[c];
                    if (trl_gl_before(metric, sc, (int32_t)(cb + c), last.score, last.index)) {
                        trl_gl_insert(mine, k, metric, sc, (int32_t)(cb + c));
                        last = mine[k - 1];
                    }
                }
            } else {
                // four columns at a time: their scores and ids are read together (eight LDS reads in flight; all 32 columns of the
                // stage exist, whatever m is), so a quarter that holds no survivor costs one LDS round trip, not four
                const int32_t* si = ids + 16 * s.h;
                for (int c4 = 0; c4 < 16 && cb + c4 < m; c4 += 4) {
                    float s4[4];
                    int32_t g4[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        s4[u] = sr[c4 + u];
                        g4[u] = si[c4 + u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const long long c = cb + c4 + u;
                        if (c < m && g4[u] >= 0 && trl_gl_before(metric, s4[u], (int32_t)c, last.score, last.index) &&
                            trl_gl_insert_group(mine, mine_ids, k, metric, s4[u], (int32_t)c, g4[u]))
                            last = mine[k - 1];
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // the next group's scores and ids follow these reads
        __builtin_amdgcn_wave_barrier();
    });
    __syncthreads();
    if (w.tid < live) {
        TrlGlEntry* L = lists + w.tid * k;               // the row's first list takes the other seven
        int32_t* I = lids + w.tid * k;
        if constexpr (GROUPS) trl_gl_merge_groups(L, I, k, metric, L + GL_ROWS * k, I + GL_ROWS * k, GL_LISTS - 1, (long long)GL_ROWS * k);
        else trl_gl_merge(L, k, metric, L + GL_ROWS * k, GL_LISTS - 1, (long long)GL_ROWS * k);
        const size_t row = (size_t)(w.row0 + w.tid);
        if (part) {
            const size_t o = ((size_t)w.strip * (size_t)n + row) * (size_t)k;
            for (int e = 0; e < k; e++) {
                part[o + e] = L[e];
                if constexpr (GROUPS) part_ids[o + e] = I[e];
            }
        } else {
            for (int e = 0; e < k; e++) {
                d_score[row * k + e] = L[e].score;
                d_index[row * k + e] = L[e].index == TRL_GL_EMPTY ? -1 : L[e].index;
                if constexpr (GROUPS) d_group[row * k + e] = I[e];
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void k_gallery_search(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n,
                                                        const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                                        long long m, int metric, int k, int tiles, long long gps, long long groups,
                                                        TrlGlEntry* __restrict__ part, float* __restrict__ d_score,
                                                        int32_t* __restrict__ d_index) {
    gl_search<false>(q, valid, n, mat, ld, gn2, nullptr, m, metric, k, tiles, gps, groups, part, nullptr, d_score, d_index, nullptr);
}

__global__ __launch_bounds__(256, 2) void k_gallery_search_groups(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n,
                                                               const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                                               const int32_t* __restrict__ gid, long long m, int metric, int k, int tiles,
                                                               long long gps, long long groups, TrlGlEntry* __restrict__ part,
                                                               int32_t* __restrict__ part_ids, float* __restrict__ d_score,
                                                               int32_t* __restrict__ d_index, int32_t* __restrict__ d_group) {
    gl_search<true>(q, valid, n, mat, ld, gn2, gid, m, metric, k, tiles, gps, groups, part, part_ids, d_score, d_index, d_group);
}

// one wave per query row: lane l merges strips l, l + 64, ... into a list of its own (a strip's k entries are loaded before they
// are looked at: independent loads), then lane 0 merges the 64 lists -- all with the code the search kernel uses; with GROUPS the
// grouped operations, so a group that reaches the merge from several strips keeps its best row
template <bool GROUPS>
__device__ __forceinline__ void gl_merge_strips(const TrlGlEntry* __restrict__ part, const int32_t* __restrict__ part_ids, int n, long long strips,
                                                int k, int metric, float* __restrict__ d_score, int32_t* __restrict__ d_index,
                                                int32_t* __restrict__ d_group) {
    __shared__ TrlGlEntry best[64 * TRL_GL_MAX_K];
    __shared__ int32_t best_ids[GROUPS ? 64 * TRL_GL_MAX_K : 1];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    TrlGlEntry* mine = best + lane * k;
    int32_t* mine_ids = best_ids + lane * k;                                                  // (GROUPS)
    for (int e = 0; e < k; e++) {
        mine[e] = trl_gl_empty();
        if constexpr (GROUPS) mine_ids[e] = -1;
    }
    for (long long s = lane; s < strips; s += 64) {
        const size_t o = ((size_t)s * (size_t)n + row) * (size_t)k;
        TrlGlEntry v[TRL_GL_MAX_K];
        [[maybe_unused]] int32_t vi[TRL_GL_MAX_K];
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++) {
            v[e] = e < k ? part[o + e] : trl_gl_empty();
            if constexpr (GROUPS) vi[e] = e < k ? part_ids[o + e] : -1;
        }
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++) {
            if constexpr (GROUPS) {
                if (e < k && v[e].index != TRL_GL_EMPTY) trl_gl_insert_group(mine, mine_ids, k, metric, v[e].score, v[e].index, vi[e]);
            } else {
                if (e < k) trl_gl_insert(mine, k, metric, v[e].score, v[e].index);
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        if constexpr (GROUPS) trl_gl_merge_groups(best, best_ids, k, metric, best + k, best_ids + k, 63, k);
        else trl_gl_merge(best, k, metric, best + k, 63, k);
    }
    __syncthreads();
    if (lane < k) {
        d_score[row * k + lane] = best[lane].score;
        d_index[row * k + lane] = best[lane].index == TRL_GL_EMPTY ? -1 : best[lane].index;
        if constexpr (GROUPS) d_group[row * k + lane] = best_ids[lane];
    }
}

__global__ __launch_bounds__(64) void k_gallery_merge(const TrlGlEntry* __restrict__ part, int n, long long strips, int k, int metric,
                                                      float* __restrict__ d_score, int32_t* __restrict__ d_index) {
    gl_merge_strips<false>(part, nullptr, n, strips, k, metric, d_score, d_index, nullptr);
}

__global__ __launch_bounds__(64) void k_gallery_merge_groups(const TrlGlEntry* __restrict__ part, const int32_t* __restrict__ part_ids, int n,
                                                             long long strips, int k, int metric, float* __restrict__ d_score,
                                                             int32_t* __restrict__ d_index, int32_t* __restrict__ d_group) {
    gl_merge_strips<true>(part, part_ids, n, strips, k, metric, d_score, d_index, d_group);
}

__global__ void k_gallery_fill(float* __restrict__ d_score, int32_t* __restrict__ d_index, long long count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < count) {
        d_score[t] = __builtin_nanf("");
        d_index[t] = -1;
    }
}

// rows [m][512] -> columns c0 .. c0 + m - 1 of mat [512][ld] and n2[c0 ..]: a workgroup takes 32 rows through a [32][64] LDS tile
// eight times (reads: 256 bytes of a row per 64 lanes; writes: 128 bytes of a k-row per 32 lanes), thread r < 32 carrying row r's
// n2 chain across the eight tiles in ascending k.
__global__ __launch_bounds__(256) void k_gallery_pack(const float* __restrict__ rows, long long m, float* __restrict__ mat, long long ld,
                                                      float* __restrict__ n2, long long c0) {
    __shared__ float t[GL_ROWS][65];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * GL_ROWS;
    const int live = m - row0 < GL_ROWS ? (int)(m - row0) : GL_ROWS;
    float acc = 0.f;
    for (int k0 = 0; k0 < GL_K; k0 += 64) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int e = tid + 256 * i, r = e >> 6, kk = e & 63;
            t[r][kk] = r < live ? rows[(size_t)(row0 + r) * GL_K + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int e = tid + 256 * i, kk = e >> 5, r = e & 31;
            if (r < live) mat[(size_t)(k0 + kk) * (size_t)ld + (size_t)(c0 + row0 + r)] = t[r][kk];
        }
        if (tid < GL_ROWS) {
#pragma unroll 16
            for (int kk = 0; kk < 64; kk++) acc = __builtin_fmaf(t[tid][kk], t[tid][kk], acc);
        }
        __syncthreads();
    }
    if (tid < live) n2[c0 + row0 + tid] = acc;
}

// ---- clustering: the link bitmap of n rows against themselves; trl_cluster.hip turns it into labels ------
// Accumulator i of the 32 x 32 C/D map holds row (i & 3) + 8 (i >> 2) + 4 (lane >> 5) at column lane & 31, so the ballot of its link
// predicate IS two finished words of the bitmap: the low half row r's word c0 / 32, the high half row r + 4's.
// No LDS stage and no atomic: every word (rows < n, words < ceil(n / 32)) is written exactly once, by one wave, with a vector store.
// Masked before the ballot: the diagonal, columns >= n, invalid columns, invalid or absent rows.  A NaN score fails both comparisons.
__global__ __launch_bounds__(256, 2) void k_gallery_links(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n,
                                                       const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                                       int metric, float thr, int tiles, long long gps, long long groups,
                                                       uint32_t* __restrict__ adj, long long pitch) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int* rowok = reinterpret_cast<const int*>(info) + 2 * GL_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)tiles;
    const int live = gl_fill_tile(tile, info, q, valid, n, row0, tid);
    const int j = lane & 31, h = lane >> 5;
    const long long g_end = (strip + 1) * gps < groups ? (strip + 1) * gps : groups;
    for (long long g = strip * gps; g < g_end; g++) {
        const long long c0 = g * GL_GROUP + wave * 32;
        if (c0 >= n) break;
        const f32x16 acc = gl_chain(tile, mat, (size_t)ld, c0, lane);
        const long long col = c0 + j;
        const float g2 = gn2[col], gs = __builtin_sqrtf(g2);          // (col < ld: n2 has ld entries)
        const bool colok = col < n && (!valid || valid[col] != 0);
        int h_here = h;                                               // (as in gl_slab: the 16 rows' LDS addresses are made
        asm volatile("" : "+v"(h_here));                              // here, not kept in registers across the chain)
        uint32_t* dst = adj + (size_t)row0 * (size_t)pitch + (size_t)(c0 >> 5);
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h_here;
            const float sc = gl_score(metric, acc[i], info[r], info[GL_ROWS + r], g2, gs);
            const bool hit = (metric == TRL_GL_COSINE ? sc >= thr : sc <= thr) && colok && rowok[r] != 0 && row0 + r != col;
            const unsigned long long b = __ballot(hit);
            if (j == 0 && r < live) dst[(size_t)r * (size_t)pitch] = h_here ? (uint32_t)(b >> 32) : (uint32_t)b;
        }
    }
}

// one wave per row: the row's popcount, + 1 for the row itself; 0 for an invalid row.  Not an atomic counter.
__global__ __launch_bounds__(256) void k_cluster_degree(const uint32_t* __restrict__ adj, long long pitch, const uint8_t* __restrict__ valid,
                                                        int n, int words, int32_t* __restrict__ degree) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint32_t* a = adj + (size_t)row * (size_t)pitch;
    int c = 0;
    for (int w = lane; w < words; w += 64) c += __popc(a[w]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) degree[row] = (!valid || valid[row] != 0) ? c + 1 : 0;
}

// ---- score histograms: pair counts per score bin, genuine and impostor ------------------------------------
// Every accumulator's score is put into its bin (trl_gallery_bins.h, the edges in LDS, padded with +inf to 1,023) and counted by an
// LDS atomic in the workgroup's own counters, [2][E + 2] uint32: class 0 impostor (qid != gid), 1 genuine; slot E + 1 the NaN scores.
// Counted: rows < n, columns < m, both valid and, with `upper`, column > row.  A workgroup sees 32 rows x gps x 128 columns < 2^32
// pairs (HI_MAX_GPS).  It stores its counters as they stand -- zeros included -- in its own slab of `part`, and k_gallery_hist_sum
// adds the slabs into the int64 output: integer sums, so the counts do not depend on strips, launch geometry or arrival order, and
// nothing has to be zeroed in front of the call.
// With `upper` the pairs below the diagonal are not computed: a workgroup starts at the column group that holds its first row, a wave
// whose 32 columns all lie at or below that row skips its chain, and a strip wholly below the diagonal skips the tile too.
// LDS: 4 KB of edges, the tile, the row info and ids, 2 (E + 2) counters -- 78.6 KB at E = 1023, two workgroups per CU as k_gallery_links.
constexpr long long HI_MAX_GPS = 1 << 19;   // column groups of a strip: 32 x 2^19 x 128 = 2^31 pairs
constexpr int HI_SQUARE_WGS = 2048;         // workgroups wanted when n == m: strips short enough that `upper` drops half of them
constexpr int HI_EDGE_WORDS = TRL_GL_PADDED_EDGES + 1;
constexpr int HI_SUM_SLOTS = 64;            // output slots of one k_gallery_hist_sum workgroup

__global__ __launch_bounds__(256, 2) void k_gallery_hist(const float* __restrict__ q, const uint8_t* __restrict__ qvalid,
                                                      const int32_t* __restrict__ qid, int n, const float* __restrict__ mat, long long ld,
                                                      const float* __restrict__ gn2, const uint8_t* __restrict__ gvalid,
                                                      const int32_t* __restrict__ gid, long long m, int metric, int upper,
                                                      const float* __restrict__ d_edges, int E, int tiles, long long gps,
                                                      long long groups, uint32_t* __restrict__ part) {
    extern __shared__ float gl_lds[];
    float* edges = gl_lds;                                 // (in front: a search trip's read is the count plus a constant offset)
    float* tile = gl_lds + HI_EDGE_WORDS;
    float* info = tile + GL_TILE_WORDS;
    const int* rowok = reinterpret_cast<const int*>(info) + 2 * GL_ROWS;
    int* rowid = reinterpret_cast<int*>(info) + GL_INFO_WORDS;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(info) + GL_INFO_WORDS + GL_ROWS;
    const int slots = 2 * (E + 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)tiles;
    for (int t = tid; t < TRL_GL_PADDED_EDGES; t += 256) edges[t] = t < E ? d_edges[t] : __builtin_inff();
    for (int t = tid; t < slots; t += 256) cnt[t] = 0u;
    if (tid < GL_ROWS) rowid[tid] = row0 + tid < n ? qid[row0 + tid] : 0;
    const long long g_end = (strip + 1) * gps < groups ? (strip + 1) * gps : groups;
    long long g_begin = strip * gps;
    if (upper && g_begin < row0 / GL_GROUP) g_begin = row0 / GL_GROUP;       // (groups in front of it end at or below row0)
    if (g_begin < g_end) {                                                    // (the same for every thread: the barriers are met by all)
        gl_fill_tile(tile, info, q, qvalid, n, row0, tid);
        const int j = lane & 31, h = lane >> 5;
        for (long long g = g_begin; g < g_end; g++) {
            const long long c0 = g * GL_GROUP + wave * 32;
            if (c0 >= m) break;
            if (upper && c0 + 31 <= row0) continue;
            const f32x16 acc = gl_chain(tile, mat, (size_t)ld, c0, lane);
            const long long col = c0 + j;
            const float g2 = gn2[col], gs = __builtin_sqrtf(g2);          // (col < ld: n2 has ld entries)
            const bool colok = col < m && (!gvalid || gvalid[col] != 0);
            const int cid = col < m ? gid[col] : 0;                       // (gid has m entries)
            int h_here = h;                                               // (as in gl_slab: the 16 rows' LDS addresses are made
            asm volatile("" : "+v"(h_here));                              // here, not kept in registers across the chain)
            auto tally = [&](auto METRIC) __attribute__((always_inline)) {
                constexpr int mt = decltype(METRIC)::value;
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int r = (i & 3) + 8 * (i >> 2) + 4 * h_here;
                    const float sc = gl_score(mt, acc[i], info[r], info[GL_ROWS + r], g2, gs);
                    const bool counted = colok && rowok[r] != 0 && (!upper || col > row0 + r);
                    const int bin = trl_gl_bin_padded(mt, sc, edges, E, TRL_GL_MAX_STEPS);
                    if (counted) atomicAdd(cnt + (rowid[r] == cid ? E + 2 : 0) + bin, 1u);
                }
            };
            if (metric == TRL_GL_COSINE) tally(std::integral_constant<int, TRL_GL_COSINE>{});
            else tally(std::integral_constant<int, TRL_GL_EUCLIDEAN>{});
        }
    }
    __syncthreads();
    uint32_t* out = part + (size_t)blockIdx.x * (size_t)slots;
    for (int t = tid; t < slots; t += 256) out[t] = cnt[t];
}

// counts[s] = the sum over the workgroups' slabs of slot s.  A workgroup takes HI_SUM_SLOTS slots: lane l of each of its 16 waves
// reads slot l of every 16th slab (256 contiguous bytes per wave), then wave 0 adds the 16 partial sums.
__global__ __launch_bounds__(1024) void k_gallery_hist_sum(const uint32_t* __restrict__ part, long long wgs, int slots,
                                                           long long* __restrict__ counts) {
    __shared__ unsigned long long sum[16][HI_SUM_SLOTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.x * HI_SUM_SLOTS + lane;
    unsigned long long acc = 0;
    if (s < slots) {
#pragma unroll 8
        for (long long w = wave; w < wgs; w += 16) acc += part[(size_t)w * (size_t)slots + s];
    }
    sum[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && s < slots) {
        for (int k = 1; k < 16; k++) acc += sum[k][lane];
        counts[s] = (long long)acc;
    }
}

// ---- range search: every match within a threshold, as CSR lists ----------------------------------------
// Two passes over the gallery, both through rg_walk: the first ends the ballot of the match predicate in popcounts per row, the second
// in ranked stores.  A workgroup takes a strip of gps column groups = 4 gps slabs of 32 columns, and wave w walks slabs w gps ..
// (w + 1) gps - 1 of them -- a contiguous quarter, not every fourth slab as in the kernels above -- so (strip, wave, column) ascending
// is the gallery index ascending and a row's place in its list is wave-private.  Pass 1 leaves one uint32 count per (strip, wave,
// row); k_range_rows turns each row's counts into exclusive bases in place and writes the row's total, k_range_scan turns the totals
// into the int64 offsets; pass 2 starts row r of (strip, wave) at offsets[r] + base and stores hit number p of the whole result iff
// p < capacity.  No atomics: every count, offset and entry is written once, by one lane, with a vector store.  Both passes recompute
// the scores -- one chain per output, so the same bits -- and share the predicate, the masks and the C/D decode: all of it is rg_walk.
constexpr int RG_WAVES = 4;

// match(r, c) of the header, but for the masks: plain f32 comparisons, false for a NaN score
__device__ __forceinline__ bool rg_match(int metric, float sc, float thr) { return metric == TRL_GL_COSINE ? sc >= thr : sc <= thr; }

struct RgArgs {
    const float* q;
    const uint8_t* qvalid;
    int n;
    const float* mat;
    long long ld;
    const float* gn2;
    const uint8_t* gvalid;
    long long m;
    int metric;
    float thr;
    int self;
    int tiles;
    long long gps;
};

// lane l's value of a position (l the same for the whole wave)
__device__ __forceinline__ long long rg_lane_value(long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave's walk over its quarter of a strip.  `run` is per lane: lanes j and j + 32 both carry row j's position -- the matches of
// row row0 + j in front of the slab at hand, counted from the caller's start value.  The ballot of the predicate over accumulator i
// is two rows' hit masks, the low half row r_lo's, the high half row r_lo + 4's.  With EMIT a hitting lane calls emit(position,
// column, score), position = its row's run + the hits of its half below its own lane; then (in both passes) the two rows' runs
// advance by the halves' popcounts.  Returns the final run.  (It takes the parts of the workgroup's GlFrame by value: handed the frame
// by reference, k_gallery_range_count compiles to one VGPR more than it had.)
template <bool EMIT, typename Pos, typename Emit>
__device__ __forceinline__ Pos rg_walk(const RgArgs& a, const float* tile, const float* info, long long row0, long long strip, int wave,
                                       int lane, Pos run, Emit&& emit) {
    const int* rowok = reinterpret_cast<const int*>(info) + 2 * GL_ROWS;
    const int j = lane & 31, h = lane >> 5;
    long long c0 = (strip * RG_WAVES + wave) * a.gps * 32;                  // the quarter's first column
    const long long ahead = a.m - c0 + 31;                                  // (slabs that begin in front of m: ahead / 32 of them)
    const int slabs = ahead < 32 ? 0 : ahead / 32 < a.gps ? (int)(ahead / 32) : (int)a.gps;
    for (int s = 0; s < slabs; s++, c0 += 32) {
        const f32x16 acc = gl_chain(tile, a.mat, (size_t)a.ld, c0, lane);   // (c0 + 31 < ld: c0 < m <= ld, both multiples of 32)
        const long long col = c0 + j;
        const float g2 = a.gn2[col], gs = __builtin_sqrtf(g2);              // (col < ld: n2 has ld entries)
        const bool colok = col < a.m && (!a.gvalid || a.gvalid[col] != 0);
        const int own = a.self ? (int)(col - row0) : -1;                    // the tile row that IS this column, if it is one of the 32
        int h_here = h;                                                     // (as in gl_slab: the 16 rows' LDS addresses are made
        asm volatile("" : "+v"(h_here));                                    // here, not kept in registers across the chain)
        const uint32_t below = (1u << j) - 1u;
        // lane j (row j) takes accumulator mine's ballot, the high half when bit 2 of j is set.  Both are made here, per slab: as
        // loop invariants the 32 lane masks "j == r_lo", "j == r_lo + 4" would be hoisted into 64 SGPRs, spilled to VGPR lanes
        // and read back for every accumulator of every slab
        int mine = (j & 3) | ((j >> 3) << 2), upper = j & 4;
        asm volatile("" : "+v"(mine), "+v"(upper));
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r_lo = (i & 3) + 8 * (i >> 2), r = r_lo + 4 * h_here;
            const float sc = gl_score(a.metric, acc[i], info[r], info[GL_ROWS + r], g2, gs);
            const bool hit = rg_match(a.metric, sc, a.thr) && colok && rowok[r] != 0 && r != own;
            const unsigned long long b = __ballot(hit);
            const uint32_t lo = (uint32_t)b, hi = (uint32_t)(b >> 32);
            if (b != 0) {                                                   // (the same for the whole wave; rarely true at a useful threshold)
                if constexpr (EMIT) {
                    const Pos at_lo = rg_lane_value(run, r_lo), at_hi = rg_lane_value(run, r_lo + 4);
                    if (hit) emit((h_here ? at_hi : at_lo) + (Pos)__popc((h_here ? hi : lo) & below), col, sc);
                }
                run += (Pos)(mine == i ? __popc(upper ? hi : lo) : 0);
            }
        }
    }
    return run;
}

// grid: x = strip * tiles + tile.  cnt [strips][4][n] uint32: every entry with row < n is written, a wave without slabs writes 0.
__global__ __launch_bounds__(256, 2) void k_gallery_range_count(RgArgs a, uint32_t* __restrict__ cnt) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)a.tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)a.tiles;
    const int live = gl_fill_tile(tile, info, a.q, a.qvalid, a.n, row0, tid);
    const uint32_t run = rg_walk<false, uint32_t>(a, tile, info, row0, strip, wave, lane, 0u, [](uint32_t, long long, float) {});
    if (lane < live) cnt[(size_t)(strip * RG_WAVES + wave) * (size_t)a.n + (size_t)(row0 + lane)] = run;
}

// one thread per row: the row's counts over (strip, wave) ascending -> exclusive bases, in place; its total -> offsets[row + 1]
__global__ __launch_bounds__(256) void k_range_rows(uint32_t* __restrict__ cnt, int n, long long parts, long long* __restrict__ offsets) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    uint32_t run = 0;
    for (long long p = 0; p < parts; p++) {
        uint32_t* c = cnt + (size_t)p * (size_t)n + (size_t)row;
        const uint32_t v = *c;
        *c = run;
        run += v;
    }
    offsets[row + 1] = run;
}

// one workgroup: offsets[1 .. n] hold the rows' totals -> offsets[0 .. n], their exclusive sums (offsets[n] the grand total).  Thread t
// owns rows t * per .. + per - 1.
__global__ __launch_bounds__(1024) void k_range_scan(long long* __restrict__ offsets, int n, long long per) {
    const int t = threadIdx.x;
    const long long lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    long long c = 0;
    for (long long i = lo; i < hi; i++) c += offsets[i + 1];
    long long run = trl_scan_1024(c);
    for (long long i = lo; i < hi; i++) {
        run += offsets[i + 1];
        offsets[i + 1] = run;
    }
    if (t == 0) offsets[0] = 0;
}

// grid as pass 1.  base = pass 1's counts after k_range_rows.  Entry p of the result is written iff 0 <= p < capacity.
__global__ __launch_bounds__(256, 2) void k_gallery_range_fill(RgArgs a, const long long* __restrict__ offsets, const uint32_t* __restrict__ base,
                                                            long long capacity, int32_t* __restrict__ d_index, float* __restrict__ d_score) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)a.tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)a.tiles;
    const int live = gl_fill_tile(tile, info, a.q, a.qvalid, a.n, row0, tid);
    const int j = lane & 31;
    long long start = 0;
    if (j < live) start = offsets[row0 + j] + (long long)base[(size_t)(strip * RG_WAVES + wave) * (size_t)a.n + (size_t)(row0 + j)];
    rg_walk<true, long long>(a, tile, info, row0, strip, wave, lane, start, [&](long long p, long long col, float sc) {
        if ((unsigned long long)p < (unsigned long long)capacity) {
            d_index[p] = (int32_t)col;
            d_score[p] = sc;
        }
    });
}

// ---- plans, workspaces and checks, each written once: a *_workspace function is a dry run of its carve ----------------------------
struct GlPlan {
    long long tiles = 0, groups = 0, gps = 0, strips = 0;
};

const char* gl_plan(int n, long long m, int k, int max_strip_cols, GlPlan* p, int target_wgs = GL_TARGET_WGS) {
    if (n < 0 || m < 0 || m > 0x7fffffffLL) return "n or m out of range (n >= 0, 0 <= m <= 2^31 - 1)";
    if (k < 1 || k > TRL_GL_MAX_K) return "k outside 1..16";
    if (max_strip_cols < 0 || max_strip_cols % GL_GROUP) return "max_strip_cols is not a multiple of 128";
    *p = GlPlan();
    if (n == 0 || m == 0) return nullptr;
    p->tiles = (n + GL_ROWS - 1) / GL_ROWS;
    p->groups = (m + GL_GROUP - 1) / GL_GROUP;
    long long want = std::max<long long>(1, target_wgs / p->tiles);
    want = std::min<long long>(want, std::min<long long>(GL_MAX_STRIPS, p->groups));
    p->gps = (p->groups + want - 1) / want;
    if (max_strip_cols > 0) p->gps = std::min<long long>(p->gps, max_strip_cols / GL_GROUP);
    p->strips = (p->groups + p->gps - 1) / p->gps;
    if (p->strips * p->tiles > 0x7fffffffLL) return "too many workgroups: raise max_strip_cols";
    return nullptr;
}

// the strips' lists [strips][n][k] and, for the grouped search, their group ids in a block of their own; none when one strip writes
// the result itself
bool gl_carve(Arena& a, const GlPlan& p, int n, int k, bool grouped, TrlGlEntry** part, int32_t** part_ids) {
    *part = nullptr;
    *part_ids = nullptr;
    if (p.strips <= 1) return true;
    const size_t entries = (size_t)p.strips * (size_t)n * (size_t)k;
    *part = (TrlGlEntry*)a.alloc(entries * sizeof(TrlGlEntry));
    if (*part && grouped) *part_ids = (int32_t*)a.alloc(entries * sizeof(int32_t));
    return *part && (*part_ids || !grouped);
}

const char* gl_check_gallery(const float* d_mat, long long ld, const float* d_n2, long long m) {
    if (!d_mat || !d_n2) return "null gallery";
    if (ld <= 0 || ld % 32) return "ld is not a positive multiple of 32";
    if (m > ld) return "m > ld";
    return nullptr;
}

int gl_check_metric(const char* who, int metric) {
    if (metric == TRL_GL_COSINE || metric == TRL_GL_EUCLIDEAN) return TRL_OK;
    trl_set_error("%s: metric %d (0 cosine, 1 euclidean)", who, metric);
    return TRL_ERR_INVALID;
}

const char* gl_check_threshold(float threshold) { return threshold - threshold == 0.f ? nullptr : "the threshold is not finite"; }

// the histogram's plan: the search's, with strips short enough for 32-bit counters; n == m (the shape of `upper`, whose workgroups
// below the diagonal do nothing) asks for four times the workgroups, so that those left still fill the device evenly
const char* hi_plan(int n, long long m, int nedges, int max_strip_cols, GlPlan* p) {
    if (nedges < 1 || nedges > TRL_GL_MAX_EDGES) return "nedges outside 1..1023";
    if (const char* why = gl_plan(n, m, 1, max_strip_cols, p, n == m ? HI_SQUARE_WGS : GL_TARGET_WGS)) return why;
    if (p->gps > HI_MAX_GPS) {
        p->gps = HI_MAX_GPS;
        p->strips = (p->groups + p->gps - 1) / p->gps;
        if (p->strips * p->tiles > 0x7fffffffLL) return "too many workgroups";
    }
    return nullptr;
}

// the workgroups' counters [strips * tiles][2 (nedges + 2)] uint32; none for an empty problem
bool hi_carve(Arena& a, const GlPlan& p, int nedges, uint32_t** part) {
    *part = nullptr;
    if (p.strips * p.tiles > 0) {
        *part = (uint32_t*)a.alloc((size_t)(p.strips * p.tiles) * (size_t)(2 * (nedges + 2)) * sizeof(uint32_t));
        if (!*part) return false;
    }
    return true;
}

// the range search's counts [strips][4][n] uint32 (pass 1's counts, then pass 2's bases); none for an empty problem.  The plan is the
// search's, so at the default plan strips x n stays near GL_TARGET_WGS x 32 whatever m is.
bool rg_carve(Arena& a, const GlPlan& p, int n, uint32_t** cnt) {
    *cnt = nullptr;
    if (p.strips * p.tiles > 0) {
        *cnt = (uint32_t*)a.alloc((size_t)p.strips * RG_WAVES * (size_t)n * sizeof(uint32_t));
        if (!*cnt) return false;
    }
    return true;
}

// what both passes refuse, in one place; null when the arguments are fine
const char* rg_check(int n, const float* d_mat, long long ld, const float* d_n2, long long m, int metric, float threshold, int self,
                     int max_strip_cols, GlPlan* p) {
    if (const char* why = gl_plan(n, m, 1, max_strip_cols, p)) return why;
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) return "the metric is neither 0 (cosine) nor 1 (euclidean)";
    if (self != 0 && self != 1) return "self is neither 0 nor 1";
    if (self && n != m) return "self = 1 needs n == m";
    if (const char* why = gl_check_threshold(threshold)) return why;
    return gl_check_gallery(d_mat, ld, d_n2, m);
}

RgArgs rg_args(const float* d_q, const uint8_t* d_qvalid, int n, const float* d_mat, long long ld, const float* d_n2, const uint8_t* d_gvalid,
               long long m, int metric, float threshold, int self, const GlPlan& p) {
    RgArgs a;
    a.q = d_q; a.qvalid = d_qvalid; a.n = n;
    a.mat = d_mat; a.ld = ld; a.gn2 = d_n2; a.gvalid = d_gvalid; a.m = m;
    a.metric = metric; a.thr = threshold; a.self = self;
    a.tiles = (int)p.tiles; a.gps = p.gps;
    return a;
}

size_t gl_search_workspace(int n, long long m, int k, int max_strip_cols, bool grouped) {
    GlPlan p;
    if (gl_plan(n, m, k, max_strip_cols, &p)) return 0;
    Arena a = Arena::counter(0);
    TrlGlEntry* part;
    int32_t* part_ids;
    gl_carve(a, p, n, k, grouped, &part, &part_ids);
    return a.high;
}

// trl_gallery_search, and with `grouped` (d_gid, d_group) trl_gallery_search_groups
int gl_search_entry(const char* who, bool grouped, const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld,
                    const float* d_n2, const int32_t* d_gid, long long m, int metric, int k, float* d_score, int32_t* d_index, int32_t* d_group,
                    void* d_ws, size_t ws_bytes, int max_strip_cols, hipStream_t s) {
    GlPlan p;
    if (const char* why = gl_plan(n, m, k, max_strip_cols, &p)) return trl_refuse(who, why);
    TRL_CHECK(gl_check_metric(who, metric));
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) return trl_refuse(who, why);
    if (grouped && m > 0 && !d_gid) return trl_refuse(who, "null group ids");
    if (n == 0) return TRL_OK;
    if (!d_q || !d_score || !d_index || (grouped && !d_group)) return trl_refuse(who, "null argument");
    Arena a = Arena::over(d_ws, ws_bytes);
    TrlGlEntry* part;
    int32_t* part_ids;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, gl_carve(a, p, n, k, grouped, &part, &part_ids),
                          [&] { return gl_search_workspace(n, m, k, max_strip_cols, grouped); }))
        return TRL_ERR_INVALID;
    TRL_CHECK(trl_device_of(d_mat));
    if (m == 0) {
        const long long count = (long long)n * k;
        k_gallery_fill<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(d_score, d_index, count);
        TRL_LAUNCH_CHECK();
        if (grouped) TRL_HIP(hipMemsetAsync(d_group, 0xff, (size_t)count * sizeof(int32_t), s));             // (-1)
        return TRL_OK;
    }
    const size_t lds = gl_lds_bytes(4 * (grouped ? GG_STAGE_WORDS : GL_STAGE_WORDS) * sizeof(float) +
                                    (size_t)GL_LISTS * GL_ROWS * k * (sizeof(TrlGlEntry) + (grouped ? sizeof(int32_t) : 0)));
    const long long wgs = p.strips * p.tiles;
    if (grouped) {
        TRL_CHECK(trl_launch_lds(k_gallery_search_groups, wgs, lds, s, d_q, d_valid, n, d_mat, ld, d_n2, d_gid, m, metric, k, (int)p.tiles, p.gps,
                            p.groups, part, part_ids, d_score, d_index, d_group));
        if (part) k_gallery_merge_groups<<<(unsigned)n, 64, 0, s>>>(part, part_ids, n, p.strips, k, metric, d_score, d_index, d_group);
    } else {
        TRL_CHECK(trl_launch_lds(k_gallery_search, wgs, lds, s, d_q, d_valid, n, d_mat, ld, d_n2, m, metric, k, (int)p.tiles, p.gps, p.groups, part,
                            d_score, d_index));
        if (part) k_gallery_merge<<<(unsigned)n, 64, 0, s>>>(part, n, p.strips, k, metric, d_score, d_index);
    }
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

}  // namespace

extern "C" size_t trl_gallery_range_workspace(int n, long long m, int max_strip_cols) {
    GlPlan p;
    if (gl_plan(n, m, 1, max_strip_cols, &p)) return 0;
    Arena a = Arena::counter(0);
    uint32_t* cnt;
    rg_carve(a, p, n, &cnt);
    return a.high;
}

extern "C" int trl_gallery_range_count(const float* d_q, const uint8_t* d_qvalid, int n, const float* d_mat, long long ld, const float* d_n2,
                                       const uint8_t* d_gvalid, long long m, int metric, float threshold, int self, long long* d_offsets,
                                       void* d_ws, size_t ws_bytes, int max_strip_cols, void* stream) {
    const char* who = "trl_gallery_range_count";
    GlPlan p;
    if (const char* why = rg_check(n, d_mat, ld, d_n2, m, metric, threshold, self, max_strip_cols, &p)) return trl_refuse(who, why);
    if (n == 0) return TRL_OK;
    if (!d_offsets || (m > 0 && !d_q)) return trl_refuse(who, "null argument");
    Arena a = Arena::over(d_ws, ws_bytes);
    uint32_t* cnt;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, rg_carve(a, p, n, &cnt), [&] { return trl_gallery_range_workspace(n, m, max_strip_cols); }))
        return TRL_ERR_INVALID;
    TRL_CHECK(trl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        TRL_HIP(hipMemsetAsync(d_offsets, 0, ((size_t)n + 1) * sizeof(long long), s));
        return TRL_OK;
    }
    TRL_CHECK(trl_launch_lds(k_gallery_range_count, p.strips * p.tiles, gl_lds_bytes(), s,
                        rg_args(d_q, d_qvalid, n, d_mat, ld, d_n2, d_gvalid, m, metric, threshold, self, p), cnt));
    k_range_rows<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(cnt, n, p.strips * RG_WAVES, d_offsets);
    TRL_LAUNCH_CHECK();
    k_range_scan<<<1, 1024, 0, s>>>(d_offsets, n, ((long long)n + 1023) / 1024);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_gallery_range_fill(const float* d_q, const uint8_t* d_qvalid, int n, const float* d_mat, long long ld, const float* d_n2,
                                      const uint8_t* d_gvalid, long long m, int metric, float threshold, int self, const long long* d_offsets,
                                      const void* d_ws, size_t ws_bytes, long long capacity, int32_t* d_index, float* d_score,
                                      int max_strip_cols, void* stream) {
    const char* who = "trl_gallery_range_fill";
    GlPlan p;
    if (const char* why = rg_check(n, d_mat, ld, d_n2, m, metric, threshold, self, max_strip_cols, &p)) return trl_refuse(who, why);
    if (capacity < 0) { trl_set_error("%s: capacity = %lld < 0", who, capacity); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_offsets || (m > 0 && !d_q) || (capacity > 0 && (!d_index || !d_score))) return trl_refuse(who, "null argument");
    Arena a = Arena::over(d_ws, ws_bytes);
    uint32_t* cnt;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, rg_carve(a, p, n, &cnt), [&] { return trl_gallery_range_workspace(n, m, max_strip_cols); }))
        return TRL_ERR_INVALID;
    if (m == 0 || capacity == 0) return TRL_OK;
    TRL_CHECK(trl_device_of(d_mat));
    return trl_launch_lds(k_gallery_range_fill, p.strips * p.tiles, gl_lds_bytes(), (hipStream_t)stream,
                     rg_args(d_q, d_qvalid, n, d_mat, ld, d_n2, d_gvalid, m, metric, threshold, self, p), d_offsets, (const uint32_t*)cnt, capacity,
                     d_index, d_score);
}

extern "C" int trl_gallery_pack(const float* d_rows, long long m, float* d_mat, long long ld, float* d_n2, long long c0, void* stream) {
    if (m < 0 || c0 < 0 || m > 0x7fffffffLL) { trl_set_error("trl_gallery_pack: m = %lld rows at column %lld", m, c0); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, 0)) return trl_refuse("trl_gallery_pack", why);
    if (c0 + m > ld) { trl_set_error("trl_gallery_pack: columns %lld..%lld of %lld", c0, c0 + m, ld); return TRL_ERR_INVALID; }
    if (m == 0) return TRL_OK;
    if (!d_rows) return trl_refuse("trl_gallery_pack", "null rows");
    TRL_CHECK(trl_device_of(d_mat));
    k_gallery_pack<<<(unsigned)((m + GL_ROWS - 1) / GL_ROWS), 256, 0, (hipStream_t)stream>>>(d_rows, m, d_mat, ld, d_n2, c0);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_gallery_scores(const float* d_q, int n, const float* d_mat, long long ld, const float* d_n2, long long m, int metric,
                                  float* d_out, long long ldo, void* stream) {
    const char* who = "trl_gallery_scores";
    if (n < 0 || m < 0 || m > 0x7fffffffLL) { trl_set_error("%s: n = %d, m = %lld", who, n, m); return TRL_ERR_INVALID; }
    TRL_CHECK(gl_check_metric(who, metric));
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) return trl_refuse(who, why);
    if (ldo < m) { trl_set_error("%s: ldo = %lld < m = %lld", who, ldo, m); return TRL_ERR_INVALID; }
    if (n == 0 || m == 0) return TRL_OK;
    if (!d_q || !d_out) return trl_refuse(who, "null argument");
    const long long tiles = (n + GL_ROWS - 1) / GL_ROWS, groups = (m + GL_GROUP - 1) / GL_GROUP;
    if (tiles * groups > 0x7fffffffLL) { trl_set_error("%s: %lld x %lld workgroups", who, tiles, groups); return TRL_ERR_INVALID; }
    TRL_CHECK(trl_device_of(d_mat));
    return trl_launch_lds(k_gallery_scores, tiles * groups, gl_lds_bytes(), (hipStream_t)stream, d_q, n, d_mat, ld, d_n2, m, metric, d_out, ldo, (int)tiles);
}

extern "C" size_t trl_gallery_search_workspace(int n, long long m, int k, int max_strip_cols) {
    return gl_search_workspace(n, m, k, max_strip_cols, false);
}

extern "C" int trl_gallery_search(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                  long long m, int metric, int k, float* d_score, int32_t* d_index, void* d_ws, size_t ws_bytes,
                                  int max_strip_cols, void* stream) {
    return gl_search_entry("trl_gallery_search", false, d_q, d_valid, n, d_mat, ld, d_n2, nullptr, m, metric, k, d_score, d_index, nullptr, d_ws,
                           ws_bytes, max_strip_cols, (hipStream_t)stream);
}

extern "C" size_t trl_gallery_search_groups_workspace(int n, long long m, int k, int max_strip_cols) {
    return gl_search_workspace(n, m, k, max_strip_cols, true);
}

extern "C" int trl_gallery_search_groups(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                         const int32_t* d_gid, long long m, int metric, int k, float* d_score, int32_t* d_index,
                                         int32_t* d_group, void* d_ws, size_t ws_bytes, int max_strip_cols, void* stream) {
    return gl_search_entry("trl_gallery_search_groups", true, d_q, d_valid, n, d_mat, ld, d_n2, d_gid, m, metric, k, d_score, d_index, d_group,
                           d_ws, ws_bytes, max_strip_cols, (hipStream_t)stream);
}

extern "C" int trl_cluster_links(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                 int metric, float threshold, uint32_t* d_adj, long long pitch_words, int32_t* d_degree,
                                 int max_strip_cols, void* stream) {
    const char* who = "trl_cluster_links";
    if (n < 0 || n > CL_MAX_N) { trl_set_error("%s: n = %d outside 0..%d", who, n, CL_MAX_N); return TRL_ERR_INVALID; }
    GlPlan p;
    if (const char* why = gl_plan(n, n, 1, max_strip_cols, &p)) return trl_refuse(who, why);
    TRL_CHECK(gl_check_metric(who, metric));
    if (const char* why = gl_check_threshold(threshold)) return trl_refuse(who, why);
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, n)) return trl_refuse(who, why);
    const int words = (n + 31) / 32;
    if (pitch_words < words) { trl_set_error("%s: pitch_words = %lld < %d", who, pitch_words, words); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_q || !d_adj || !d_degree) return trl_refuse(who, "null argument");
    TRL_CHECK(trl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_launch_lds(k_gallery_links, p.strips * p.tiles, gl_lds_bytes(), s, d_q, d_valid, n, d_mat, ld, d_n2, metric, threshold, (int)p.tiles,
                        p.gps, p.groups, d_adj, pitch_words));
    k_cluster_degree<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(d_adj, pitch_words, d_valid, n, words, d_degree);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" size_t trl_gallery_hist_workspace(int n, long long m, int nedges, int max_strip_cols) {
    GlPlan p;
    if (hi_plan(n, m, nedges, max_strip_cols, &p)) return 0;
    Arena a = Arena::counter(0);
    uint32_t* part;
    hi_carve(a, p, nedges, &part);
    return a.high;
}

extern "C" int trl_gallery_hist(const float* d_q, const uint8_t* d_qvalid, const int32_t* d_qid, int n, const float* d_mat, long long ld,
                                const float* d_n2, const uint8_t* d_gvalid, const int32_t* d_gid, long long m, int metric, int pairs,
                                const float* d_edges, int nedges, long long* d_counts, void* d_ws, size_t ws_bytes, int max_strip_cols,
                                void* stream) {
    const char* who = "trl_gallery_hist";
    GlPlan p;
    if (const char* why = hi_plan(n, m, nedges, max_strip_cols, &p)) return trl_refuse(who, why);
    TRL_CHECK(gl_check_metric(who, metric));
    if (pairs != TRL_GL_PAIRS_ALL && pairs != TRL_GL_PAIRS_UPPER) { trl_set_error("%s: pairs %d (0 all, 1 upper)", who, pairs); return TRL_ERR_INVALID; }
    if (pairs == TRL_GL_PAIRS_UPPER && n != m) { trl_set_error("%s: upper pairs need n == m, not %d and %lld", who, n, m); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) return trl_refuse(who, why);
    if (!d_edges || !d_counts || (n > 0 && (!d_q || !d_qid)) || (m > 0 && !d_gid)) return trl_refuse(who, "null argument");
    Arena a = Arena::over(d_ws, ws_bytes);
    uint32_t* part;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, hi_carve(a, p, nedges, &part), [&] { return trl_gallery_hist_workspace(n, m, nedges, max_strip_cols); }))
        return TRL_ERR_INVALID;
    TRL_CHECK(trl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    const int slots = 2 * (nedges + 2);
    if (n == 0 || m == 0) {
        TRL_HIP(hipMemsetAsync(d_counts, 0, (size_t)slots * sizeof(long long), s));
        return TRL_OK;
    }
    const long long wgs = p.strips * p.tiles;
    TRL_CHECK(trl_launch_lds(k_gallery_hist, wgs, gl_lds_bytes((size_t)(GL_ROWS + slots) * 4, HI_EDGE_WORDS), s, d_q, d_qvalid, d_qid, n, d_mat, ld, d_n2,
                        d_gvalid, d_gid, m, metric, pairs, d_edges, nedges, (int)p.tiles, p.gps, p.groups, part));
    k_gallery_hist_sum<<<(unsigned)((slots + HI_SUM_SLOTS - 1) / HI_SUM_SLOTS), 1024, 0, s>>>(part, wgs, slots, d_counts);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

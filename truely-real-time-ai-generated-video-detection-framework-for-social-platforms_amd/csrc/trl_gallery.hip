// trl_gallery.hip -- embedding match: a gallery of enrolled 512-float embeddings on the device, the full
// score matrix of n queries against it, and the fused top-k search that never writes that matrix.
//
// The gallery is k-major, [512][ld] f32 with ld a multiple of 32 and zero padding, plus n2[ld] -- the loader's layout of
// facenet.logits.w, and for the reason trl_logits.hip gives: lane l's B operand of v_mfma_f32_32x32x2_f32 is one dword of a whole
// 128-byte line, so the gallery goes from memory into the matrix core without touching LDS.  The main loop is k_logits' with a
// zero bias: a workgroup holds a row tile of 32 queries in LDS ([32][514] words), each of its 4 waves owns 32 gallery columns of a
// 128-column group, the columns stream through a three-deep register ring, and every output is ONE accumulator over ascending k:
//     dot(q, g) = chain(0; k = 0..511: acc = fmaf(q[k], g[k], acc))                         
// n2(x) = dot(x, x) is the same chain, taken once per gallery row at enrolment (k_gallery_pack) and once per query row per
// workgroup (gl_fill_tile).  The epilogue turns accumulators into scores:
//     cosine      dot / (sqrtf(n2 q) * sqrtf(n2 g))
//     euclidean   s = n2 q + n2 g;  d2 = fmaf(-2, dot, s);  d2 < 0 ? 0 : d2;  sqrtf(d2)
// k_gallery_scores stores them (rows < n, columns < m).  k_gallery_search keeps running lists of the k best matches in LDS
// (trl_gallery_order.h): a wave puts its 32 x 32 scores through an LDS stage, then lane l walks row l & 31 over 16 of the 32
// columns against a list of its own -- a score is compared with the list's k-th entry, kept in a register, and only survivors
// are inserted: after a strip's first groups almost none, and the 64 lists of a wave are updated side by side.  A workgroup walks
// a STRIP of column groups, merges its eight lists per row and writes n x k entries per strip; k_gallery_merge merges the strips
// per row by the same order.  Scores do not depend on n, tile, strip or launch geometry (one chain per output), and the order is
// total, so neither does the result.
//
// Clustering (f-8) is the same main loop ended in a ballot: k_gallery_links writes the packed link bitmap of n rows against
// themselves, and the k_cluster_* kernels turn it into DBSCAN labels by rounds of hooking and pointer jumping, a launch each.
// Past the bitmap's 65,536 rows the k_cluster_list_* kernels hook and assign over the range search's neighbour lists instead.
//
// Score histograms (f-9) end it in counters: k_gallery_hist counts the pairs per score bin (trl_gallery_bins.h), genuine and
// impostor apart, in LDS, and k_gallery_hist_sum adds the workgroups' counters into the int64 result.
//
// The range search (f-10) ends it in popcounts and ranked stores: k_gallery_range_count counts each row's matches per (strip, wave),
// k_range_rows / k_range_scan turn the counts into bases and int64 offsets, k_gallery_range_fill stores the CSR lists.
//
// The grouped search (f-11) ends it in lists of distinct groups: k_gallery_search_groups is k_gallery_search with a group id per gallery
// row and lists that hold each group's best row only (trl_gallery_groups.h), k_gallery_merge_groups merges the strips by the same rule.
#include <algorithm>
#include <utility>

#include "trl_common.h"
#include "trl_gallery_bins.h"
#include "trl_gallery_groups.h"
#include "trl_gallery_order.h"

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

// grid: x = group * tiles + tile (the row tile is the fast index: workgroups in flight share a few column groups in L2)
__global__ __launch_bounds__(256) void k_gallery_scores(const float* __restrict__ q, int n, const float* __restrict__ mat, long long ld,
                                                        const float* __restrict__ gn2, long long m, int metric, float* __restrict__ out,
                                                        long long ldo, int tiles) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, group = blockIdx.x / (unsigned)tiles;
    const int live = gl_fill_tile(tile, info, q, nullptr, n, row0, tid);
    const long long c0 = group * GL_GROUP + wave * 32;
    if (c0 >= m) return;                                 // (behind the last barrier)
    const f32x16 acc = gl_chain(tile, mat, (size_t)ld, c0, lane);
    const int j = lane & 31, h = lane >> 5;
    const long long col = c0 + j;
    if (col >= m) return;
    const float g2 = gn2[col], gs = __builtin_sqrtf(g2);
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = (i & 3) + 8 * (i >> 2) + 4 * h;
        if (r < live) out[(size_t)(row0 + r) * (size_t)ldo + col] = gl_score(metric, acc[i], info[r], info[GL_ROWS + r], g2, gs);
    }
}

// grid: x = strip * tiles + tile.  A workgroup walks column groups strip * gps .. (strip + 1) * gps - 1.  Each wave keeps its own
// lists (two per row) and its own score stage: nothing crosses waves until the strip is done, so the group loop holds no barrier.
// LDS: the tile, the row info, 4 stages of 32 x 33 words, 8 x 32 x k entries (93 KB at k = 5: one workgroup per CU).
__global__ __launch_bounds__(256, 2) void k_gallery_search(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n,
                                                        const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                                        long long m, int metric, int k, int tiles, long long gps, long long groups,
                                                        TrlGlEntry* __restrict__ part, float* __restrict__ d_score,
                                                        int32_t* __restrict__ d_index) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int* rowok = reinterpret_cast<const int*>(info) + 2 * GL_ROWS;
    float* stages = gl_lds + GL_TILE_WORDS + GL_INFO_WORDS;
    TrlGlEntry* lists = reinterpret_cast<TrlGlEntry*>(stages + 4 * GL_STAGE_WORDS);              // (8-byte aligned: even word offset)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)tiles;
    float* stage = stages + wave * GL_STAGE_WORDS;
    // lane l keeps the list of row l & 31 over columns 16 (l >> 5) .. + 15 of each of the wave's 32-column slabs
    TrlGlEntry* mine = lists + ((wave * 2 + (lane >> 5)) * GL_ROWS + (lane & 31)) * k;
    for (int e = 0; e < k; e++) mine[e] = trl_gl_empty();
    const int live = gl_fill_tile(tile, info, q, valid, n, row0, tid);
    const int j = lane & 31, h = lane >> 5;
    const long long g_end = (strip + 1) * gps < groups ? (strip + 1) * gps : groups;
    for (long long g = strip * gps; g < g_end; g++) {
        const long long c0 = g * GL_GROUP + wave * 32;
        if (c0 >= m) break;
        const f32x16 acc = gl_chain(tile, mat, (size_t)ld, c0, lane);
        const long long col = c0 + j;
        const float g2 = gn2[col], gs = __builtin_sqrtf(g2);          // (col < ld: n2 has ld entries)
        int h_here = h;                                               // (the 16 rows' LDS addresses are made here, not kept in
        asm volatile("" : "+v"(h_here));                              // registers across the chain)
        // the wave's 32 x 32 scores go through LDS, so that each lane can walk ONE row's scores against its own list: 64 lists
        // are updated side by side, and after a strip's first groups a score is one LDS read and one comparison
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h_here;
            stage[r * 33 + j] = gl_score(metric, acc[i], info[r], info[GL_ROWS + r], g2, gs);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // (wave-private data: the fence orders the wave's own LDS traffic)
        __builtin_amdgcn_wave_barrier();
        if (rowok[j]) {
            const float* sr = stage + j * 33 + 16 * h_here;
            const long long cb = c0 + 16 * h_here;
            TrlGlEntry last = mine[k - 1];
            for (int c = 0; c < 16 && cb + c < m; c++) {
                const float sc = sr[c];
                if (trl_gl_before(metric, sc, (int32_t)(cb + c), last.score, last.index)) {
                    trl_gl_insert(mine, k, metric, sc, (int32_t)(cb + c));
                    last = mine[k - 1];
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // the next group's scores follow these reads
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (tid < live) {
        TrlGlEntry* L = lists + tid * k;                 // the row's first list takes the other seven
        trl_gl_merge(L, k, metric, L + GL_ROWS * k, GL_LISTS - 1, (long long)GL_ROWS * k);
        const size_t row = (size_t)(row0 + tid);
        if (part) {
            TrlGlEntry* o = part + ((size_t)strip * (size_t)n + row) * (size_t)k;
            for (int e = 0; e < k; e++) o[e] = L[e];
        } else {
            for (int e = 0; e < k; e++) {
                d_score[row * k + e] = L[e].score;
                d_index[row * k + e] = L[e].index == TRL_GL_EMPTY ? -1 : L[e].index;
            }
        }
    }
}

// one wave per query row: lane l merges strips l, l + 64, ... into a list of its own (a strip's k entries are loaded before they
// are looked at: independent loads), then lane 0 merges the 64 lists -- all with the code the search kernel uses
__global__ __launch_bounds__(64) void k_gallery_merge(const TrlGlEntry* __restrict__ part, int n, long long strips, int k, int metric,
                                                      float* __restrict__ d_score, int32_t* __restrict__ d_index) {
    __shared__ TrlGlEntry best[64 * TRL_GL_MAX_K];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    TrlGlEntry* mine = best + lane * k;
    for (int e = 0; e < k; e++) mine[e] = trl_gl_empty();
    for (long long s = lane; s < strips; s += 64) {
        const TrlGlEntry* src = part + ((size_t)s * (size_t)n + row) * (size_t)k;
        TrlGlEntry v[TRL_GL_MAX_K];
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++) v[e] = e < k ? src[e] : trl_gl_empty();
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++)
            if (e < k) trl_gl_insert(mine, k, metric, v[e].score, v[e].index);
    }
    __syncthreads();
    if (lane == 0) trl_gl_merge(best, k, metric, best + k, 63, k);
    __syncthreads();
    if (lane < k) {
        d_score[row * k + lane] = best[lane].score;
        d_index[row * k + lane] = best[lane].index == TRL_GL_EMPTY ? -1 : best[lane].index;
    }
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

// ---- clustering: the link bitmap of n rows against themselves, then DBSCAN labels over it ----------------
// k_gallery_links is k_gallery_search's frame -- gl_fill_tile, a strip of column groups per workgroup, gl_chain, gl_score -- with
// another end: accumulator i of the 32 x 32 C/D map holds row (i & 3) + 8 (i >> 2) + 4 (lane >> 5) at column lane & 31, so the
// ballot of its link predicate IS two finished words of the bitmap: the low half row r's word c0 / 32, the high half row r + 4's.
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
        int h_here = h;                                               // (as in k_gallery_search: the 16 rows' LDS addresses are
        asm volatile("" : "+v"(h_here));                              // made here, not kept in registers across the chain)
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

// Labels.  Every kernel below reads buffers that no workgroup writes in the same launch, so nothing depends on one workgroup seeing
// another's stores; a round is a copy and two launches (b = a; hook: a -> b; jump: b -> a) and the host decides between small
// batches of rounds.
constexpr int CL_NONE = 0x7fffffff;   // the label of a row that is not core
constexpr int CL_JUMPS = 32;          // pointer chases of one jump launch (over a buffer the launch does not write)
constexpr int CL_BATCH = 4;           // rounds queued between two looks at the change flags
constexpr int CL_MAX_N = 65536;

__global__ void k_cluster_init(const int32_t* __restrict__ degree, int n, int min_samples, uint8_t* __restrict__ core, int32_t* __restrict__ lab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int d = degree[i];
    const bool c = d > 0 && d >= min_samples;
    core[i] = c;
    lab[i] = c ? i : CL_NONE;
}

// the smallest of f(label of j) over the set bits j < n of bitmap row `a`, by one wave (every lane returns it); rows that are not
// core carry CL_NONE and drop out of the minimum by themselves
template <typename F>
__device__ __forceinline__ int cl_row_min(const uint32_t* __restrict__ a, int n, int words, const int32_t* __restrict__ lab, int lane, F&& f) {
    int m = CL_NONE;
    for (int w = lane; w < words; w += 64) {
        uint32_t bits = a[w];
        if (w == words - 1 && (n & 31)) bits &= (1u << (n & 31)) - 1u;      // (a caller's bitmap is never followed past n)
        while (bits) {
            const int b = __ffs(bits) - 1;
            bits &= bits - 1;
            const int v = f(lab[32 * w + b]);
            m = v < m ? v : m;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
    }
    return m;
}

// one wave per core row: m = the smallest label among the row's core neighbours; where m is below the row's own label, both the row
// and the row its label names (its tree's root, after a jump) take it: out[row] = min(out[row], m), out[own] = min(out[own], m).
// `out` is a copy of `in` made in front of the launch and this launch touches it with atomicMin only -- never a plain store beside
// an atomic on one line -- and min commutes, so `out` does not depend on the order the waves run in.  *changed likewise is only
// ever touched by atomics, the memset in front of the batch and the copy behind it, and lies in an allocation of its own.
__global__ __launch_bounds__(256) void k_cluster_hook(const uint32_t* __restrict__ adj, long long pitch, int n, int words,
                                                      const int32_t* __restrict__ in, int32_t* out, int* changed) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int own = in[row];
    if (own == CL_NONE) return;
    const int m = cl_row_min(adj + (size_t)row * (size_t)pitch, n, words, in, lane, [](int l) { return l; });
    if (lane == 0 && m < own) {
        atomicMin(out + row, m);
        atomicMin(out + own, m);
        atomicOr(changed, 1);
    }
}

// out = the label CL_JUMPS steps up the chain of `in` (labels only point downwards and a root points at itself, so the walk ends)
__global__ void k_cluster_jump(const int32_t* __restrict__ in, int n, int32_t* __restrict__ out, int* changed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int own = in[i];
    int l = own;
    if (own != CL_NONE) {
        for (int s = 0; s < CL_JUMPS; s++) {
            const int up = in[l];
            if (up == l) break;
            l = up;
        }
    }
    out[i] = l;
    if (l != own) atomicOr(changed, 1);
}

// one workgroup: cid[i] = the number of roots (core rows whose label is their own index) below i, for every root i; *count = roots.
// Thread t owns rows t * per .. + per - 1; the 1,024 partial counts are scanned in LDS.
__global__ __launch_bounds__(1024) void k_cluster_number(const int32_t* __restrict__ lab, int n, int per, int32_t* __restrict__ cid,
                                                         int32_t* __restrict__ count) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int c = 0;
    for (int i = lo; i < hi; i++) c += lab[i] == i;
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int base = part[t] - c;
    for (int i = lo; i < hi; i++) cid[i] = lab[i] == i ? base++ : -1;
    if (t == 1023) *count = part[1023];
}

// one wave per row: a core row takes its root's number; a valid row that is not core the smallest number among its core
// neighbours' clusters (a border row), -1 without one (noise); an invalid row -1
__global__ __launch_bounds__(256) void k_cluster_assign(const uint32_t* __restrict__ adj, long long pitch, const int32_t* __restrict__ degree,
                                                        int n, int words, const int32_t* __restrict__ lab, const int32_t* __restrict__ cid,
                                                        int32_t* __restrict__ labels) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int own = lab[row];
    int out = -1;
    if (own != CL_NONE) {
        out = cid[own];
    } else if (degree[row] > 0) {
        const int m = cl_row_min(adj + (size_t)row * (size_t)pitch, n, words, lab, lane, [&](int l) { return l == CL_NONE ? CL_NONE : cid[l]; });
        out = m == CL_NONE ? -1 : m;
    }
    if (lane == 0) labels[row] = out;
}

// the label stage's workspace, carved once: trl_cluster_workspace is a dry run of this
struct ClWs {
    int32_t *a = nullptr, *b = nullptr, *cid = nullptr;
    int* changed = nullptr;           // CL_BATCH flags, in an allocation of their own
};

bool cl_carve(Arena& a, int n, ClWs* w) {
    const size_t bytes = (size_t)n * sizeof(int32_t);
    w->a = (int32_t*)a.alloc(bytes);
    w->b = (int32_t*)a.alloc(bytes);
    w->cid = (int32_t*)a.alloc(bytes);
    w->changed = (int*)a.alloc(CL_BATCH * sizeof(int));
    return w->a && w->b && w->cid && w->changed;
}

// The rounds of either label stage: copy, hook (a -> b, launched by `hook` with the round's change flag) and jump (b -> a) until a
// round changes nothing, CL_BATCH rounds queued between two looks at the flags.  Every round before the last lowers at least one
// label, and a label is at least 0 and at most its row's index -- whatever the links hold -- so the loop ends; the bound of n rounds
// is a second line of defence.  *rounds_out (may be null): the rounds up to and including the first that changed nothing.
template <typename Hook>
int cl_rounds(const char* who, const ClWs& w, int n, hipStream_t s, int* rounds_out, Hook&& hook) {
    int rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= n + CL_BATCH) { trl_set_error("%s: no fixed point after %d rounds", who, rounds); return TRL_ERR_STATE; }
        TRL_HIP(hipMemsetAsync(w.changed, 0, CL_BATCH * sizeof(int), s));
        for (int r = 0; r < CL_BATCH; r++) {
            TRL_HIP(hipMemcpyAsync(w.b, w.a, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            hook(w.changed + r);
            TRL_LAUNCH_CHECK();
            k_cluster_jump<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(w.b, n, w.a, w.changed + r);
            TRL_LAUNCH_CHECK();
        }
        int changed[CL_BATCH];
        TRL_HIP(hipMemcpyAsync(changed, w.changed, sizeof(changed), hipMemcpyDeviceToHost, s));
        TRL_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < CL_BATCH && !done; r++) {
            rounds++;
            done = changed[r] == 0;
        }
    }
    if (rounds_out) *rounds_out = rounds;
    return TRL_OK;
}

// ---- the label stage over neighbour lists: past the bitmap's 65,536 rows ---------------------------------
// The links are CSR lists -- row i's neighbours are index[offsets[i] .. offsets[i + 1]), what the range search writes with self = 1 --
// and k_cluster_init / jump / number run as they are: they never see the links.  Lists of face clusters hold tens of entries, so a
// row is walked by L = 4 / 16 / 64 lanes of a wave, the 256 / L rows of a workgroup side by side.  The L lanes of a row are an
// aligned group of their wave and leave a kernel together, so the xor shuffles below stay among lanes that are there.
constexpr int CL_LIST_MAX_N = 1 << 24;

// a thread per row: the row's list length, + 1 for the row itself; 0 for an invalid row
__global__ void k_cluster_list_degree(const long long* __restrict__ offsets, const uint8_t* __restrict__ valid, int n, int32_t* __restrict__ degree) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    degree[i] = (!valid || valid[i] != 0) ? (int)(offsets[i + 1] - offsets[i]) + 1 : 0;
}

// the smallest of f(label of j) over the entries j of the list index[beg .. end), by the L lanes that share the row (each of them
// returns it).  An entry outside 0 .. n - 1 is skipped, never followed; rows that are not core carry CL_NONE and drop out.
template <int L, typename F>
__device__ __forceinline__ int cl_list_min(const int32_t* __restrict__ index, long long beg, long long end, int n, const int32_t* __restrict__ lab,
                                           int sub, F&& f) {
    int m = CL_NONE;
    for (long long p = beg + sub; p < end; p += L) {
        const uint32_t j = (uint32_t)index[p];
        if (j < (uint32_t)n) {
            const int v = f(lab[j]);
            m = v < m ? v : m;
        }
    }
#pragma unroll
    for (int off = L / 2; off >= 1; off >>= 1) {
        const int o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
    }
    return m;
}

// k_cluster_hook over a list: L lanes per core row, and the same stores -- `out` is a copy of `in` made in front of the launch and
// is touched by atomicMin only, *changed by atomicOr only; nothing here reads what another workgroup writes in this launch.
template <int L>
__global__ __launch_bounds__(256) void k_cluster_list_hook(const long long* __restrict__ offsets, const int32_t* __restrict__ index, int n,
                                                           const int32_t* __restrict__ in, int32_t* out, int* changed) {
    const int sub = threadIdx.x & (L - 1);
    const long long row = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    if (row >= n) return;
    const int own = in[row];
    if (own == CL_NONE) return;
    const int m = cl_list_min<L>(index, offsets[row], offsets[row + 1], n, in, sub, [](int l) { return l; });
    if (sub == 0 && m < own) {
        atomicMin(out + row, m);
        atomicMin(out + own, m);
        atomicOr(changed, 1);
    }
}

// k_cluster_assign over a list: L lanes per row
template <int L>
__global__ __launch_bounds__(256) void k_cluster_list_assign(const long long* __restrict__ offsets, const int32_t* __restrict__ index,
                                                             const int32_t* __restrict__ degree, int n, const int32_t* __restrict__ lab,
                                                             const int32_t* __restrict__ cid, int32_t* __restrict__ labels) {
    const int sub = threadIdx.x & (L - 1);
    const long long row = (long long)blockIdx.x * (256 / L) + threadIdx.x / L;
    if (row >= n) return;
    const int own = lab[row];
    int out = -1;
    if (own != CL_NONE) {
        out = cid[own];
    } else if (degree[row] > 0) {
        const int m = cl_list_min<L>(index, offsets[row], offsets[row + 1], n, lab, sub, [&](int l) { return l == CL_NONE ? CL_NONE : cid[l]; });
        out = m == CL_NONE ? -1 : m;
    }
    if (sub == 0) labels[row] = out;
}

template <int L>
void cl_list_hook(const long long* offsets, const int32_t* index, int n, const int32_t* in, int32_t* out, int* changed, hipStream_t s) {
    k_cluster_list_hook<L><<<(unsigned)((n + 256 / L - 1) / (256 / L)), 256, 0, s>>>(offsets, index, n, in, out, changed);
}

template <int L>
void cl_list_assign(const long long* offsets, const int32_t* index, const int32_t* degree, int n, const int32_t* lab, const int32_t* cid,
                    int32_t* labels, hipStream_t s) {
    k_cluster_list_assign<L><<<(unsigned)((n + 256 / L - 1) / (256 / L)), 256, 0, s>>>(offsets, index, degree, n, lab, cid, labels);
}

// the lanes per row for lists of `mean` entries on average, from profiles/cluster_lists_kernel_stats.csv: at
// the sizes this stage is for, 4 lanes win up to lists of 127 and 16 lanes at 1,023; 64 lanes won nowhere past 1,024 rows
int cl_list_lanes(long long mean) { return mean < 384 ? 4 : 16; }

// ---- score histograms: pair counts per score bin, genuine and impostor ------------------------------------
// k_gallery_hist is k_gallery_links' frame with a fourth end: every accumulator's score is put into its bin (trl_gallery_bins.h, the
// edges in LDS, padded with +inf to 1,023) and counted by an LDS atomic in the workgroup's own counters, [2][E + 2] uint32: class 0
// impostor (qid != gid), 1 genuine; slot E + 1 the NaN scores.  Counted: rows < n, columns < m, both valid and, with `upper`, column >
// row.  A workgroup sees 32 rows x gps x 128 columns < 2^32 pairs (HI_MAX_GPS).  It stores its counters as they stand -- zeros
// included -- in its own slab of `part`, and k_gallery_hist_sum adds the slabs into the int64 output: integer sums, so the counts do
// not depend on strips, launch geometry or arrival order, and nothing has to be zeroed in front of the call.
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
            int h_here = h;                                               // (as in k_gallery_search: the 16 rows' LDS addresses are
            asm volatile("" : "+v"(h_here));                              // made here, not kept in registers across the chain)
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
// Two passes over the gallery in k_gallery_links' frame, both through rg_walk: the first ends the ballot of the match predicate in
// popcounts per row, the second in ranked stores.  A workgroup takes a strip of gps column groups = 4 gps slabs of 32 columns, and
// wave w walks slabs w gps .. (w + 1) gps - 1 of them -- a contiguous quarter, not every fourth slab as in the kernels above -- so
// (strip, wave, column) ascending is the gallery index ascending and a row's place in its list is wave-private: the loop over slabs
// holds no barrier, as k_gallery_search's.  Pass 1 leaves one uint32 count per (strip, wave, row); k_range_rows turns each row's
// counts into exclusive bases in place and writes the row's total, k_range_scan turns the totals into the int64 offsets; pass 2
// starts row r of (strip, wave) at offsets[r] + base and stores hit number p of the whole result iff p < capacity.  No atomics: every
// count, offset and entry is written once, by one lane, with a vector store.  Both passes recompute the scores -- one chain per
// output, so the same bits -- and share the predicate, the masks and the C/D decode: all of it is rg_walk.
constexpr int RG_WAVES = 4;

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

// match(r, c) of the header, but for the masks: plain f32 comparisons, false for a NaN score
__device__ __forceinline__ bool rg_match(int metric, float sc, float thr) { return metric == TRL_GL_COSINE ? sc >= thr : sc <= thr; }

// lane l's value of a position (l the same for the whole wave)
__device__ __forceinline__ long long rg_lane_value(long long v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// One wave's walk over its quarter of a strip.  `run` is per lane: lanes j and j + 32 both carry row j's position -- the matches of
// row row0 + j in front of the slab at hand, counted from the caller's start value.  Accumulator i holds row r = (i & 3) + 8 (i >> 2)
// + 4 (lane >> 5) at column lane & 31, so the ballot of the predicate is two rows' hit masks, the low half row r_lo's, the high
// half row r_lo + 4's.  With EMIT a hitting lane calls emit(position, column, score), position = its row's run + the hits of its
// half below its own lane; then (in both passes) the two rows' runs advance by the halves' popcounts.  Returns the final run.
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
        int h_here = h;                                                     // (as in k_gallery_search: the 16 rows' LDS addresses are
        asm volatile("" : "+v"(h_here));                                    // made here, not kept in registers across the chain)
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
// owns rows t * per .. + per - 1, as k_cluster_number; the 1,024 partial sums are scanned in LDS.
__global__ __launch_bounds__(1024) void k_range_scan(long long* __restrict__ offsets, int n, long long per) {
    __shared__ long long part[1024];
    const int t = threadIdx.x;
    const long long lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    long long c = 0;
    for (long long i = lo; i < hi; i++) c += offsets[i + 1];
    part[t] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    long long run = part[t] - c;
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

// ---- grouped search: per query the k best DISTINCT groups, each with its best row ------------------------
// k_gallery_search's frame with another list: every gallery row carries a group id (gid < 0: the row is excluded), and a list holds
// the best row of each of the k best groups seen so far (trl_gallery_groups.h: 8-byte entries as before, their groups in a parallel
// int32 array).  The slab's 32 ids are loaded like gn2 -- lane j loads gid[c0 + j], one line -- and staged behind the wave's scores.
// The comparison with the list's k-th entry, kept in a register, is still a valid rejection: a full list holds better rows of k
// distinct groups, so the newcomer is either beaten inside its own group or by k others.  A lane reads the scores and ids of four
// columns together (one LDS round trip per quarter of its 16 columns); the list itself is touched for survivors only.
// A strip's list of its k best distinct groups is enough for the merge.  Suppose group L's globally best row lies in strip s and is
// not in strip s's list: then k other groups each have a row in strip s alone that comes before it, their globally best rows come
// before it too, and L is not among the k best groups.  So every group of the answer reaches the merge with its globally best row,
// and rows of it from other strips lose to that row in trl_gl_insert_group.  The same holds one level down for the eight lists of a
// row inside a workgroup, and one level up for the 64 lanes of the merge kernel.
// LDS at k = 16: 65,792 (tile) + 384 (info) + 17,408 (stages with ids) + 32,768 (entries) + 16,384 (groups) = 132,736 bytes.
constexpr int GG_STAGE_WORDS = GL_STAGE_WORDS + GL_ROWS;   // a wave's 32 x 32 scores, then its slab's 32 group ids

__global__ __launch_bounds__(256, 2) void k_gallery_search_groups(const float* __restrict__ q, const uint8_t* __restrict__ valid, int n,
                                                               const float* __restrict__ mat, long long ld, const float* __restrict__ gn2,
                                                               const int32_t* __restrict__ gid, long long m, int metric, int k, int tiles,
                                                               long long gps, long long groups, TrlGlEntry* __restrict__ part,
                                                               int32_t* __restrict__ part_ids, float* __restrict__ d_score,
                                                               int32_t* __restrict__ d_index, int32_t* __restrict__ d_group) {
    extern __shared__ float gl_lds[];
    float* tile = gl_lds;
    float* info = gl_lds + GL_TILE_WORDS;
    const int* rowok = reinterpret_cast<const int*>(info) + 2 * GL_ROWS;
    float* stages = gl_lds + GL_TILE_WORDS + GL_INFO_WORDS;
    TrlGlEntry* lists = reinterpret_cast<TrlGlEntry*>(stages + 4 * GG_STAGE_WORDS);              // (8-byte aligned: even word offset)
    int32_t* lids = reinterpret_cast<int32_t*>(lists + GL_LISTS * GL_ROWS * k);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)(blockIdx.x % (unsigned)tiles) * GL_ROWS, strip = blockIdx.x / (unsigned)tiles;
    float* stage = stages + wave * GG_STAGE_WORDS;
    int32_t* ids = reinterpret_cast<int32_t*>(stage + GL_STAGE_WORDS);
    // lane l keeps the list of row l & 31 over columns 16 (l >> 5) .. + 15 of each of the wave's 32-column slabs
    const int at = ((wave * 2 + (lane >> 5)) * GL_ROWS + (lane & 31)) * k;
    TrlGlEntry* mine = lists + at;
    int32_t* mine_ids = lids + at;
    for (int e = 0; e < k; e++) {
        mine[e] = trl_gl_empty();
        mine_ids[e] = -1;
    }
    const int live = gl_fill_tile(tile, info, q, valid, n, row0, tid);
    const int j = lane & 31, h = lane >> 5;
    const long long g_end = (strip + 1) * gps < groups ? (strip + 1) * gps : groups;
    for (long long g = strip * gps; g < g_end; g++) {
        const long long c0 = g * GL_GROUP + wave * 32;
        if (c0 >= m) break;
        const f32x16 acc = gl_chain(tile, mat, (size_t)ld, c0, lane);
        const long long col = c0 + j;
        const float g2 = gn2[col], gs = __builtin_sqrtf(g2);          // (col < ld: n2 has ld entries)
        const int32_t id = col < m ? gid[col] : -1;                   // (gid has m entries)
        int h_here = h;                                               // (as in k_gallery_search: the 16 rows' LDS addresses are
        asm volatile("" : "+v"(h_here));                              // made here, not kept in registers across the chain)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * h_here;
            stage[r * 33 + j] = gl_score(metric, acc[i], info[r], info[GL_ROWS + r], g2, gs);
        }
        if (h_here == 0) ids[j] = id;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // (wave-private data: the fence orders the wave's own LDS traffic)
        __builtin_amdgcn_wave_barrier();
        if (rowok[j]) {
            const float* sr = stage + j * 33 + 16 * h_here;
            const int32_t* si = ids + 16 * h_here;
            const long long cb = c0 + 16 * h_here;
            TrlGlEntry last = mine[k - 1];
            // four columns at a time: their scores and ids are read together (eight LDS reads in flight; all 32 columns of the
            // stage exist, whatever m is), so a quarter that holds no survivor costs one LDS round trip, not four
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
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");        // the next group's scores and ids follow these reads
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    if (tid < live) {
        TrlGlEntry* L = lists + tid * k;                 // the row's first list takes the other seven
        int32_t* I = lids + tid * k;
        trl_gl_merge_groups(L, I, k, metric, L + GL_ROWS * k, I + GL_ROWS * k, GL_LISTS - 1, (long long)GL_ROWS * k);
        const size_t row = (size_t)(row0 + tid);
        if (part) {
            const size_t o = ((size_t)strip * (size_t)n + row) * (size_t)k;
            for (int e = 0; e < k; e++) {
                part[o + e] = L[e];
                part_ids[o + e] = I[e];
            }
        } else {
            for (int e = 0; e < k; e++) {
                d_score[row * k + e] = L[e].score;
                d_index[row * k + e] = L[e].index == TRL_GL_EMPTY ? -1 : L[e].index;
                d_group[row * k + e] = I[e];
            }
        }
    }
}

// one wave per query row, as k_gallery_merge: lane l puts strips l, l + 64, ... into a list of its own, then lane 0 merges the 64
// lists -- with the grouped operations, so a group that reaches the merge from several strips keeps its best row
__global__ __launch_bounds__(64) void k_gallery_merge_groups(const TrlGlEntry* __restrict__ part, const int32_t* __restrict__ part_ids, int n,
                                                             long long strips, int k, int metric, float* __restrict__ d_score,
                                                             int32_t* __restrict__ d_index, int32_t* __restrict__ d_group) {
    __shared__ TrlGlEntry best[64 * TRL_GL_MAX_K];
    __shared__ int32_t best_ids[64 * TRL_GL_MAX_K];
    const int lane = threadIdx.x;
    const size_t row = blockIdx.x;
    TrlGlEntry* mine = best + lane * k;
    int32_t* mine_ids = best_ids + lane * k;
    for (int e = 0; e < k; e++) {
        mine[e] = trl_gl_empty();
        mine_ids[e] = -1;
    }
    for (long long s = lane; s < strips; s += 64) {
        const size_t o = ((size_t)s * (size_t)n + row) * (size_t)k;
        TrlGlEntry v[TRL_GL_MAX_K];
        int32_t vi[TRL_GL_MAX_K];
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++) {
            v[e] = e < k ? part[o + e] : trl_gl_empty();
            vi[e] = e < k ? part_ids[o + e] : -1;
        }
#pragma unroll
        for (int e = 0; e < TRL_GL_MAX_K; e++)
            if (e < k && v[e].index != TRL_GL_EMPTY) trl_gl_insert_group(mine, mine_ids, k, metric, v[e].score, v[e].index, vi[e]);
    }
    __syncthreads();
    if (lane == 0) trl_gl_merge_groups(best, best_ids, k, metric, best + k, best_ids + k, 63, k);
    __syncthreads();
    if (lane < k) {
        d_score[row * k + lane] = best[lane].score;
        d_index[row * k + lane] = best[lane].index == TRL_GL_EMPTY ? -1 : best[lane].index;
        d_group[row * k + lane] = best_ids[lane];
    }
}

// ---- the search's plan and workspace, written once: trl_gallery_search_workspace is a dry run of gl_carve -------------------------
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

// the strips' lists [strips][n][k]; none when one strip writes the result itself
bool gl_carve(Arena& a, const GlPlan& p, int n, int k, TrlGlEntry** part) {
    *part = nullptr;
    if (p.strips > 1) {
        *part = (TrlGlEntry*)a.alloc((size_t)p.strips * (size_t)n * (size_t)k * sizeof(TrlGlEntry));
        if (!*part) return false;
    }
    return true;
}

// the grouped search's strip lists: gl_carve's entries [strips][n][k] and, in a block of their own, their group ids
bool gg_carve(Arena& a, const GlPlan& p, int n, int k, TrlGlEntry** part, int32_t** part_ids) {
    *part_ids = nullptr;
    if (!gl_carve(a, p, n, k, part)) return false;
    if (*part) {
        *part_ids = (int32_t*)a.alloc((size_t)p.strips * (size_t)n * (size_t)k * sizeof(int32_t));
        if (!*part_ids) return false;
    }
    return true;
}

int gl_device_of(const void* p) {
    hipPointerAttribute_t attr;
    TRL_HIP(hipPointerGetAttributes(&attr, p));
    TRL_HIP(hipSetDevice(attr.device));
    return TRL_OK;
}

const char* gl_check_gallery(const float* d_mat, long long ld, const float* d_n2, long long m) {
    if (!d_mat || !d_n2) return "null gallery";
    if (ld <= 0 || ld % 32) return "ld is not a positive multiple of 32";
    if (m > ld) return "m > ld";
    return nullptr;
}

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
    if (!(threshold - threshold == 0.f)) return "the threshold is not finite";
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
    GlPlan p;
    if (const char* why = rg_check(n, d_mat, ld, d_n2, m, metric, threshold, self, max_strip_cols, &p)) {
        trl_set_error("trl_gallery_range_count: %s", why);
        return TRL_ERR_INVALID;
    }
    if (n == 0) return TRL_OK;
    if (!d_offsets || (m > 0 && !d_q)) { trl_set_error("trl_gallery_range_count: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    uint32_t* cnt;
    if (((uintptr_t)d_ws & 7) || !rg_carve(a, p, n, &cnt)) {
        trl_set_error("trl_gallery_range_count: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_gallery_range_workspace(n, m, max_strip_cols));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        TRL_HIP(hipMemsetAsync(d_offsets, 0, ((size_t)n + 1) * sizeof(long long), s));
        return TRL_OK;
    }
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS) * 4;
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_range_count, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    k_gallery_range_count<<<(unsigned)(p.strips * p.tiles), 256, lds, s>>>(
        rg_args(d_q, d_qvalid, n, d_mat, ld, d_n2, d_gvalid, m, metric, threshold, self, p), cnt);
    TRL_LAUNCH_CHECK();
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
    GlPlan p;
    if (const char* why = rg_check(n, d_mat, ld, d_n2, m, metric, threshold, self, max_strip_cols, &p)) {
        trl_set_error("trl_gallery_range_fill: %s", why);
        return TRL_ERR_INVALID;
    }
    if (capacity < 0) { trl_set_error("trl_gallery_range_fill: capacity = %lld < 0", capacity); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_offsets || (m > 0 && !d_q) || (capacity > 0 && (!d_index || !d_score))) {
        trl_set_error("trl_gallery_range_fill: null argument");
        return TRL_ERR_INVALID;
    }
    Arena a;
    a.base = (char*)const_cast<void*>(d_ws);
    a.cap = d_ws ? ws_bytes : 0;
    uint32_t* cnt;
    if (((uintptr_t)d_ws & 7) || !rg_carve(a, p, n, &cnt)) {
        trl_set_error("trl_gallery_range_fill: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_gallery_range_workspace(n, m, max_strip_cols));
        return TRL_ERR_INVALID;
    }
    if (m == 0 || capacity == 0) return TRL_OK;
    TRL_CHECK(gl_device_of(d_mat));
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS) * 4;
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_range_fill, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    k_gallery_range_fill<<<(unsigned)(p.strips * p.tiles), 256, lds, (hipStream_t)stream>>>(
        rg_args(d_q, d_qvalid, n, d_mat, ld, d_n2, d_gvalid, m, metric, threshold, self, p), d_offsets, cnt, capacity, d_index, d_score);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_gallery_pack(const float* d_rows, long long m, float* d_mat, long long ld, float* d_n2, long long c0, void* stream) {
    if (m < 0 || c0 < 0 || m > 0x7fffffffLL) { trl_set_error("trl_gallery_pack: m = %lld rows at column %lld", m, c0); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, 0)) { trl_set_error("trl_gallery_pack: %s", why); return TRL_ERR_INVALID; }
    if (c0 + m > ld) { trl_set_error("trl_gallery_pack: columns %lld..%lld of %lld", c0, c0 + m, ld); return TRL_ERR_INVALID; }
    if (m == 0) return TRL_OK;
    if (!d_rows) { trl_set_error("trl_gallery_pack: null rows"); return TRL_ERR_INVALID; }
    TRL_CHECK(gl_device_of(d_mat));
    k_gallery_pack<<<(unsigned)((m + GL_ROWS - 1) / GL_ROWS), 256, 0, (hipStream_t)stream>>>(d_rows, m, d_mat, ld, d_n2, c0);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_gallery_scores(const float* d_q, int n, const float* d_mat, long long ld, const float* d_n2, long long m, int metric,
                                  float* d_out, long long ldo, void* stream) {
    if (n < 0 || m < 0 || m > 0x7fffffffLL) { trl_set_error("trl_gallery_scores: n = %d, m = %lld", n, m); return TRL_ERR_INVALID; }
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) { trl_set_error("trl_gallery_scores: metric %d (0 cosine, 1 euclidean)", metric); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) { trl_set_error("trl_gallery_scores: %s", why); return TRL_ERR_INVALID; }
    if (ldo < m) { trl_set_error("trl_gallery_scores: ldo = %lld < m = %lld", ldo, m); return TRL_ERR_INVALID; }
    if (n == 0 || m == 0) return TRL_OK;
    if (!d_q || !d_out) { trl_set_error("trl_gallery_scores: null argument"); return TRL_ERR_INVALID; }
    const long long tiles = (n + GL_ROWS - 1) / GL_ROWS, groups = (m + GL_GROUP - 1) / GL_GROUP;
    if (tiles * groups > 0x7fffffffLL) { trl_set_error("trl_gallery_scores: %lld x %lld workgroups", tiles, groups); return TRL_ERR_INVALID; }
    TRL_CHECK(gl_device_of(d_mat));
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS) * 4;
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_scores, hipFuncAttributeMaxDynamicSharedMemorySize, lds));   // above the default 64 KB
    k_gallery_scores<<<(unsigned)(tiles * groups), 256, lds, (hipStream_t)stream>>>(d_q, n, d_mat, ld, d_n2, m, metric, d_out, ldo, (int)tiles);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" size_t trl_gallery_search_workspace(int n, long long m, int k, int max_strip_cols) {
    GlPlan p;
    if (gl_plan(n, m, k, max_strip_cols, &p)) return 0;
    Arena a = Arena::counter(0);
    TrlGlEntry* part;
    gl_carve(a, p, n, k, &part);
    return a.high;
}

extern "C" int trl_gallery_search(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                  long long m, int metric, int k, float* d_score, int32_t* d_index, void* d_ws, size_t ws_bytes,
                                  int max_strip_cols, void* stream) {
    GlPlan p;
    if (const char* why = gl_plan(n, m, k, max_strip_cols, &p)) { trl_set_error("trl_gallery_search: %s", why); return TRL_ERR_INVALID; }
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) { trl_set_error("trl_gallery_search: metric %d (0 cosine, 1 euclidean)", metric); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) { trl_set_error("trl_gallery_search: %s", why); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_q || !d_score || !d_index) { trl_set_error("trl_gallery_search: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    TrlGlEntry* part;
    if (((uintptr_t)d_ws & 7) || !gl_carve(a, p, n, k, &part)) {
        trl_set_error("trl_gallery_search: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_gallery_search_workspace(n, m, k, max_strip_cols));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        const long long count = (long long)n * k;
        k_gallery_fill<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(d_score, d_index, count);
        TRL_LAUNCH_CHECK();
        return TRL_OK;
    }
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS + 4 * GL_STAGE_WORDS) * 4 + GL_LISTS * GL_ROWS * k * (int)sizeof(TrlGlEntry);
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_search, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    k_gallery_search<<<(unsigned)(p.strips * p.tiles), 256, lds, s>>>(d_q, d_valid, n, d_mat, ld, d_n2, m, metric, k, (int)p.tiles, p.gps,
                                                                     p.groups, part, d_score, d_index);
    TRL_LAUNCH_CHECK();
    if (part) {
        k_gallery_merge<<<(unsigned)n, 64, 0, s>>>(part, n, p.strips, k, metric, d_score, d_index);
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

extern "C" size_t trl_gallery_search_groups_workspace(int n, long long m, int k, int max_strip_cols) {
    GlPlan p;
    if (gl_plan(n, m, k, max_strip_cols, &p)) return 0;
    Arena a = Arena::counter(0);
    TrlGlEntry* part;
    int32_t* part_ids;
    gg_carve(a, p, n, k, &part, &part_ids);
    return a.high;
}

extern "C" int trl_gallery_search_groups(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                         const int32_t* d_gid, long long m, int metric, int k, float* d_score, int32_t* d_index,
                                         int32_t* d_group, void* d_ws, size_t ws_bytes, int max_strip_cols, void* stream) {
    GlPlan p;
    if (const char* why = gl_plan(n, m, k, max_strip_cols, &p)) { trl_set_error("trl_gallery_search_groups: %s", why); return TRL_ERR_INVALID; }
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) { trl_set_error("trl_gallery_search_groups: metric %d (0 cosine, 1 euclidean)", metric); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) { trl_set_error("trl_gallery_search_groups: %s", why); return TRL_ERR_INVALID; }
    if (m > 0 && !d_gid) { trl_set_error("trl_gallery_search_groups: null group ids"); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_q || !d_score || !d_index || !d_group) { trl_set_error("trl_gallery_search_groups: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    TrlGlEntry* part;
    int32_t* part_ids;
    if (((uintptr_t)d_ws & 7) || !gg_carve(a, p, n, k, &part, &part_ids)) {
        trl_set_error("trl_gallery_search_groups: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes,
                      trl_gallery_search_groups_workspace(n, m, k, max_strip_cols));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    if (m == 0) {
        const long long count = (long long)n * k;
        k_gallery_fill<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(d_score, d_index, count);
        TRL_LAUNCH_CHECK();
        TRL_HIP(hipMemsetAsync(d_group, 0xff, (size_t)count * sizeof(int32_t), s));             // (-1)
        return TRL_OK;
    }
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS + 4 * GG_STAGE_WORDS) * 4 + GL_LISTS * GL_ROWS * k * (int)(sizeof(TrlGlEntry) + sizeof(int32_t));
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_search_groups, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    k_gallery_search_groups<<<(unsigned)(p.strips * p.tiles), 256, lds, s>>>(d_q, d_valid, n, d_mat, ld, d_n2, d_gid, m, metric, k, (int)p.tiles,
                                                                            p.gps, p.groups, part, part_ids, d_score, d_index, d_group);
    TRL_LAUNCH_CHECK();
    if (part) {
        k_gallery_merge_groups<<<(unsigned)n, 64, 0, s>>>(part, part_ids, n, p.strips, k, metric, d_score, d_index, d_group);
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

extern "C" int trl_cluster_links(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                 int metric, float threshold, uint32_t* d_adj, long long pitch_words, int32_t* d_degree,
                                 int max_strip_cols, void* stream) {
    if (n < 0 || n > CL_MAX_N) { trl_set_error("trl_cluster_links: n = %d outside 0..%d", n, CL_MAX_N); return TRL_ERR_INVALID; }
    GlPlan p;
    if (const char* why = gl_plan(n, n, 1, max_strip_cols, &p)) { trl_set_error("trl_cluster_links: %s", why); return TRL_ERR_INVALID; }
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) { trl_set_error("trl_cluster_links: metric %d (0 cosine, 1 euclidean)", metric); return TRL_ERR_INVALID; }
    if (!(threshold - threshold == 0.f)) { trl_set_error("trl_cluster_links: the threshold is not finite"); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, n)) { trl_set_error("trl_cluster_links: %s", why); return TRL_ERR_INVALID; }
    const int words = (n + 31) / 32;
    if (pitch_words < words) { trl_set_error("trl_cluster_links: pitch_words = %lld < %d", pitch_words, words); return TRL_ERR_INVALID; }
    if (n == 0) return TRL_OK;
    if (!d_q || !d_adj || !d_degree) { trl_set_error("trl_cluster_links: null argument"); return TRL_ERR_INVALID; }
    TRL_CHECK(gl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    const int lds = (GL_TILE_WORDS + GL_INFO_WORDS) * 4;
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_links, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    k_gallery_links<<<(unsigned)(p.strips * p.tiles), 256, lds, s>>>(d_q, d_valid, n, d_mat, ld, d_n2, metric, threshold, (int)p.tiles, p.gps,
                                                                    p.groups, d_adj, pitch_words);
    TRL_LAUNCH_CHECK();
    k_cluster_degree<<<(unsigned)((n + 3) / 4), 256, 0, s>>>(d_adj, pitch_words, d_valid, n, words, d_degree);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" size_t trl_cluster_workspace(int n) {
    if (n < 0 || n > CL_MAX_N) return 0;
    Arena a = Arena::counter(0);
    ClWs w;
    cl_carve(a, n, &w);
    return a.high;
}

extern "C" int trl_cluster_labels(const uint32_t* d_adj, long long pitch_words, const int32_t* d_degree, int n, int min_samples,
                                  int32_t* d_labels, uint8_t* d_core, int32_t* d_count, void* d_ws, size_t ws_bytes, int* rounds_out,
                                  void* stream) {
    if (n < 0 || n > CL_MAX_N) { trl_set_error("trl_cluster_labels: n = %d outside 0..%d", n, CL_MAX_N); return TRL_ERR_INVALID; }
    if (min_samples < 1) { trl_set_error("trl_cluster_labels: min_samples = %d < 1", min_samples); return TRL_ERR_INVALID; }
    const int words = (n + 31) / 32;
    if (pitch_words < words) { trl_set_error("trl_cluster_labels: pitch_words = %lld < %d", pitch_words, words); return TRL_ERR_INVALID; }
    if (!d_count) { trl_set_error("trl_cluster_labels: null count"); return TRL_ERR_INVALID; }
    if (n > 0 && (!d_adj || !d_degree || !d_labels || !d_core)) { trl_set_error("trl_cluster_labels: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    ClWs w;
    if (n > 0 && (((uintptr_t)d_ws & 7) || !cl_carve(a, n, &w))) {
        trl_set_error("trl_cluster_labels: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_cluster_workspace(n));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_count));
    hipStream_t s = (hipStream_t)stream;
    if (rounds_out) *rounds_out = 0;
    if (n == 0) {
        TRL_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
        return TRL_OK;
    }
    const unsigned per_thread = (unsigned)((n + 255) / 256), per_wave = (unsigned)((n + 3) / 4);
    k_cluster_init<<<per_thread, 256, 0, s>>>(d_degree, n, min_samples, d_core, w.a);
    TRL_LAUNCH_CHECK();
    TRL_CHECK(cl_rounds("trl_cluster_labels", w, n, s, rounds_out, [&](int* changed) {
        k_cluster_hook<<<per_wave, 256, 0, s>>>(d_adj, pitch_words, n, words, w.a, w.b, changed);
    }));
    k_cluster_number<<<1, 1024, 0, s>>>(w.a, n, (n + 1023) / 1024, w.cid, d_count);
    TRL_LAUNCH_CHECK();
    k_cluster_assign<<<per_wave, 256, 0, s>>>(d_adj, pitch_words, d_degree, n, words, w.a, w.cid, d_labels);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" size_t trl_cluster_lists_workspace(int n) {
    if (n < 0 || n > CL_LIST_MAX_N) return 0;
    Arena a = Arena::counter(0);
    ClWs w;
    cl_carve(a, n, &w);
    return a.high;
}

extern "C" int trl_cluster_labels_lists(const long long* d_offsets, const int32_t* d_index, const uint8_t* d_valid, int n, int min_samples,
                                        int lanes_per_row, int32_t* d_degree, int32_t* d_labels, uint8_t* d_core, int32_t* d_count,
                                        void* d_ws, size_t ws_bytes, int* rounds_out, void* stream) {
    if (n < 0 || n > CL_LIST_MAX_N) { trl_set_error("trl_cluster_labels_lists: n = %d outside 0..%d", n, CL_LIST_MAX_N); return TRL_ERR_INVALID; }
    if (min_samples < 1) { trl_set_error("trl_cluster_labels_lists: min_samples = %d < 1", min_samples); return TRL_ERR_INVALID; }
    if (lanes_per_row != 0 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64) {
        trl_set_error("trl_cluster_labels_lists: lanes_per_row = %d (0, 4, 16 or 64)", lanes_per_row);
        return TRL_ERR_INVALID;
    }
    if (!d_count) { trl_set_error("trl_cluster_labels_lists: null count"); return TRL_ERR_INVALID; }
    if (n > 0 && (!d_offsets || !d_index || !d_degree || !d_labels || !d_core)) { trl_set_error("trl_cluster_labels_lists: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    ClWs w;
    if (n > 0 && (((uintptr_t)d_ws & 7) || !cl_carve(a, n, &w))) {
        trl_set_error("trl_cluster_labels_lists: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_cluster_lists_workspace(n));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_count));
    hipStream_t s = (hipStream_t)stream;
    if (rounds_out) *rounds_out = 0;
    if (n == 0) {
        TRL_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
        return TRL_OK;
    }
    int L = lanes_per_row;
    if (L == 0) {                     // the mean list length decides; the round loop below waits for the stream anyway
        long long total = 0;
        TRL_HIP(hipMemcpyAsync(&total, d_offsets + n, sizeof(total), hipMemcpyDeviceToHost, s));
        TRL_HIP(hipStreamSynchronize(s));
        L = cl_list_lanes(total / n);
    }
    const unsigned per_thread = (unsigned)((n + 255) / 256);
    k_cluster_list_degree<<<per_thread, 256, 0, s>>>(d_offsets, d_valid, n, d_degree);
    TRL_LAUNCH_CHECK();
    k_cluster_init<<<per_thread, 256, 0, s>>>(d_degree, n, min_samples, d_core, w.a);
    TRL_LAUNCH_CHECK();
    TRL_CHECK(cl_rounds("trl_cluster_labels_lists", w, n, s, rounds_out, [&](int* changed) {
        if (L == 4) cl_list_hook<4>(d_offsets, d_index, n, w.a, w.b, changed, s);
        else if (L == 16) cl_list_hook<16>(d_offsets, d_index, n, w.a, w.b, changed, s);
        else cl_list_hook<64>(d_offsets, d_index, n, w.a, w.b, changed, s);
    }));
    k_cluster_number<<<1, 1024, 0, s>>>(w.a, n, (n + 1023) / 1024, w.cid, d_count);
    TRL_LAUNCH_CHECK();
    if (L == 4) cl_list_assign<4>(d_offsets, d_index, d_degree, n, w.a, w.cid, d_labels, s);
    else if (L == 16) cl_list_assign<16>(d_offsets, d_index, d_degree, n, w.a, w.cid, d_labels, s);
    else cl_list_assign<64>(d_offsets, d_index, d_degree, n, w.a, w.cid, d_labels, s);
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
    GlPlan p;
    if (const char* why = hi_plan(n, m, nedges, max_strip_cols, &p)) { trl_set_error("trl_gallery_hist: %s", why); return TRL_ERR_INVALID; }
    if (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN) { trl_set_error("trl_gallery_hist: metric %d (0 cosine, 1 euclidean)", metric); return TRL_ERR_INVALID; }
    if (pairs != TRL_GL_PAIRS_ALL && pairs != TRL_GL_PAIRS_UPPER) { trl_set_error("trl_gallery_hist: pairs %d (0 all, 1 upper)", pairs); return TRL_ERR_INVALID; }
    if (pairs == TRL_GL_PAIRS_UPPER && n != m) { trl_set_error("trl_gallery_hist: upper pairs need n == m, not %d and %lld", n, m); return TRL_ERR_INVALID; }
    if (const char* why = gl_check_gallery(d_mat, ld, d_n2, m)) { trl_set_error("trl_gallery_hist: %s", why); return TRL_ERR_INVALID; }
    if (!d_edges || !d_counts || (n > 0 && (!d_q || !d_qid)) || (m > 0 && !d_gid)) { trl_set_error("trl_gallery_hist: null argument"); return TRL_ERR_INVALID; }
    Arena a;
    a.base = (char*)d_ws;
    a.cap = d_ws ? ws_bytes : 0;
    uint32_t* part;
    if (((uintptr_t)d_ws & 7) || !hi_carve(a, p, nedges, &part)) {
        trl_set_error("trl_gallery_hist: workspace of %zu bytes (need %zu, 8-byte aligned)", ws_bytes, trl_gallery_hist_workspace(n, m, nedges, max_strip_cols));
        return TRL_ERR_INVALID;
    }
    TRL_CHECK(gl_device_of(d_mat));
    hipStream_t s = (hipStream_t)stream;
    const int slots = 2 * (nedges + 2);
    if (n == 0 || m == 0) {
        TRL_HIP(hipMemsetAsync(d_counts, 0, (size_t)slots * sizeof(long long), s));
        return TRL_OK;
    }
    const int lds = (HI_EDGE_WORDS + GL_TILE_WORDS + GL_INFO_WORDS + GL_ROWS + slots) * 4;
    TRL_HIP(hipFuncSetAttribute((const void*)k_gallery_hist, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const long long wgs = p.strips * p.tiles;
    k_gallery_hist<<<(unsigned)wgs, 256, lds, s>>>(d_q, d_qvalid, d_qid, n, d_mat, ld, d_n2, d_gvalid, d_gid, m, metric, pairs, d_edges, nedges,
                                                  (int)p.tiles, p.gps, p.groups, part);
    TRL_LAUNCH_CHECK();
    k_gallery_hist_sum<<<(unsigned)((slots + HI_SUM_SLOTS - 1) / HI_SUM_SLOTS), 1024, 0, s>>>(part, wgs, slots, d_counts);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

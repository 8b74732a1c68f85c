// trl_pool.hip -- embedding templates ("Templates"; section 7, f-13): rows of 512 floats pooled per group id into
// one row per group -- an identity's enrolled photos, a track's frames, a cluster's members -- and each group's representative row.
// The rules are trl_pool.h's; this file is their schedule.
//
// The sum is defined in fixed point (trl_pool.h), so the schedule is free: the bits do not depend on it.  A workgroup takes a TILE of
// consecutive rows through LDS (coalesced reads, as k_gallery_pack), thread r carries row r's n2 chain (or reads it), and BEFORE ANY
// ATOMIC the tile is reduced per distinct group id: the contributing rows are ranked by (first row of their id in the tile, row), a
// thread walks the ranked rows for its two columns with one int64 sum, and a sum leaves the workgroup when the id changes.  Runs of
// equal ids (a tracker's output, a sorted gallery) and repeated ids cost one set of adds per tile, not one per row.  An add is a
// 64-bit integer atomicAdd; lane l of a wave owns columns 64 j + l, so a wave instruction adds 512 contiguous bytes.
// k_pool_rep_add is the same walk: the template row of each distinct id of the tile is gathered into LDS beside the rows, thread r
// runs row r's chain against it (and the template's own chain), and one 64-bit atomicMax of the tile's best key per group goes out.
// The key is trl_bestkey.h's, which the best shots of trl_quality.hip share; k_best_key_read and its launcher trl_best_key_read
// read an array of keys back for both.  The entry points' checks, device lookup and launches are trl_host.h's.
#include "trl_bestkey.h"
#include "trl_host.h"
#include "trl_pool.h"

namespace {

constexpr int PL_K = TRL_POOL_K;
constexpr int PL_PITCH = PL_K + 1;    // LDS row pitch in words: thread r walks row r, 32 rows on 32 banks
constexpr int PL_THREADS = 256;      // (trl_launch_lds' workgroup)
constexpr int PL_TILE_DEFAULT = 32;
constexpr int PL_TILE_MAX = 32;

struct PlRow {
    float c;            // the row's factor w / sqrtf(n2)
    float n2;
    int32_t g;          // its group, relative to g0; -1: the row does not contribute
    int32_t first;      // the first contributing row of the tile with that group
    long long wq;
};

// rows row0 .. row0 + rows - 1 -> tile (rows past m as zeros), then the tile's rows classified: info[r], order[0 .. *count) the
// contributing rows with equal groups side by side, *skipped.  Ends on a barrier.
// The loads of a batch are all issued before the first is stored: a thread has 16 (float4, rows 16-byte aligned) or 16 x 4 loads in
// flight, not one.
template <int ROWS>
__device__ __forceinline__ void pl_fill(float* tile, PlRow* info, int* order, int* counts, const float* __restrict__ x, long long ld,
                                        const float* __restrict__ n2, const int32_t* __restrict__ gid, const float* __restrict__ w,
                                        long long m, long long row0, long long g0, long long groups) {
    constexpr int rows = ROWS;
    const int tid = threadIdx.x;
    const int live = m - row0 < rows ? (int)(m - row0) : rows;
    const float* src = x + (size_t)row0 * (size_t)ld;
    if (((reinterpret_cast<uintptr_t>(x) & 15) | (ld & 3)) == 0) {
        constexpr int N = ROWS * PL_K / 4 / PL_THREADS;                      // float4 per thread: 4, 8 or 16
        float4 v[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int e = tid + PL_THREADS * i, r = e >> 7, c = e & 127;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < live) v[i] = *reinterpret_cast<const float4*>(src + (size_t)r * (size_t)ld + 4 * c);
        }
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int e = tid + PL_THREADS * i, r = e >> 7, c = e & 127;
            float* d = tile + r * PL_PITCH + 4 * c;
            d[0] = v[i].x, d[1] = v[i].y, d[2] = v[i].z, d[3] = v[i].w;
        }
    } else {
        constexpr int B = 16;                                                // loads per batch
        for (int e0 = 0; e0 < ROWS * PL_K; e0 += B * PL_THREADS) {
            float v[B];
#pragma unroll
            for (int i = 0; i < B; i++) {
                const int e = e0 + tid + PL_THREADS * i, r = e >> 9, k = e & (PL_K - 1);
                v[i] = r < live ? src[(size_t)r * (size_t)ld + k] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < B; i++) {
                const int e = e0 + tid + PL_THREADS * i, r = e >> 9, k = e & (PL_K - 1);
                tile[r * PL_PITCH + k] = v[i];
            }
        }
    }
    __syncthreads();
    if (tid < rows) {
        PlRow me;
        me.c = 0.f, me.n2 = 0.f, me.g = -1, me.first = -1, me.wq = 0;
        int cls = TRL_POOL_IGNORED;
        if (tid < live) {
            const int32_t id = gid[row0 + tid];
            const float wr = w ? w[row0 + tid] : 1.0f;
            cls = trl_pool_class(id, g0, groups, wr, 1.0f);                 // (ignored, or skipped by its weight: no chain needed)
            if (cls == TRL_POOL_CONTRIBUTES) {
                const float* xr = tile + tid * PL_PITCH;
                float acc = 0.f;
                if (n2) acc = n2[row0 + tid];
                else {
#pragma unroll 16
                    for (int k = 0; k < PL_K; k++) acc = __builtin_fmaf(xr[k], xr[k], acc);
                }
                cls = trl_pool_class(id, g0, groups, wr, acc);
                if (cls == TRL_POOL_CONTRIBUTES) {
                    me.c = trl_pool_factor(wr, acc);
                    me.n2 = acc;
                    me.g = (int32_t)((long long)id - g0);
                    me.wq = trl_pool_weight(wr);
                }
            }
        }
        info[tid] = me;
        order[PL_TILE_MAX + tid] = cls == TRL_POOL_SKIPPED;
    }
    __syncthreads();
    if (tid < rows && info[tid].g >= 0) {
        int first = tid;
        for (int j = tid - 1; j >= 0; j--)
            if (info[j].g == info[tid].g) first = j;
        info[tid].first = first;
    }
    __syncthreads();
    if (tid < rows && info[tid].g >= 0) {
        int rank = 0;                                                        // contributing rows in front of this one by (first, row)
        for (int j = 0; j < rows; j++)
            if (info[j].g >= 0 && (info[j].first < info[tid].first || (info[j].first == info[tid].first && j < tid))) rank++;
        order[rank] = tid;
    }
    if (tid == 0) {
        int c = 0, s = 0;
        for (int j = 0; j < rows; j++) c += info[j].g >= 0, s += order[PL_TILE_MAX + j];
        counts[0] = c, counts[1] = s;
    }
    __syncthreads();
}

constexpr size_t pl_lds_bytes(int rows, int tiles) {
    return (size_t)tiles * rows * PL_PITCH * 4 + (size_t)PL_TILE_MAX * sizeof(PlRow) + (2 * PL_TILE_MAX + 2) * sizeof(int);
}

struct PlFrame {
    float* tile;
    PlRow* info;
    int *order, *counts;
    __device__ __forceinline__ PlFrame() {
        extern __shared__ long long pl_lds[];                               // (8-byte aligned: PlRow holds an int64)
        info = reinterpret_cast<PlRow*>(pl_lds);
        order = reinterpret_cast<int*>(info + PL_TILE_MAX);
        counts = order + 2 * PL_TILE_MAX;
        tile = reinterpret_cast<float*>(counts + 2);
    }
};

template <int ROWS>
__global__ __launch_bounds__(PL_THREADS) void k_pool_add(unsigned long long* __restrict__ state, long long groups, long long g0,
                                                         const float* __restrict__ x, long long ld, const float* __restrict__ n2,
                                                         const int32_t* __restrict__ gid, const float* __restrict__ w, long long m) {
    constexpr int rows = ROWS;
    const PlFrame f;
    const int tid = threadIdx.x;
    pl_fill<ROWS>(f.tile, f.info, f.order, f.counts, x, ld, n2, gid, w, m, (long long)blockIdx.x * rows, g0, groups);
    const int nc = f.counts[0];
    if (tid == 0 && f.counts[1]) atomicAdd(state, (unsigned long long)f.counts[1]);
    if (nc == 0) return;
    unsigned long long* W = state + trl_pool_w_at(groups);
    unsigned long long* N = state + trl_pool_n_at(groups);
    unsigned long long* A = state + trl_pool_a_at(groups);
    // the weights and counts: the first row of each group takes its group's
    if (tid < rows && f.info[tid].first == tid) {
        long long wq = 0, n = 0;
        for (int j = tid; j < rows; j++)
            if (f.info[j].first == tid) wq += f.info[j].wq, n++;
        atomicAdd(W + f.info[tid].g, (unsigned long long)wq);
        atomicAdd(N + f.info[tid].g, (unsigned long long)n);
    }
    // the terms: wave v takes columns 64 j + lane for j = v and v + 4
    const int lane = tid & 63, wave = tid >> 6;
    const int k0 = 64 * wave + lane, k1 = k0 + 256;
    long long s0 = 0, s1 = 0;
    for (int i = 0; i < nc; i++) {
        const int r = f.order[i];
        const PlRow me = f.info[r];
        s0 += trl_pool_term(me.c, f.tile[r * PL_PITCH + k0]);
        s1 += trl_pool_term(me.c, f.tile[r * PL_PITCH + k1]);
        if (i + 1 == nc || f.info[f.order[i + 1]].first != me.first) {      // (uniform over the workgroup)
            unsigned long long* a = A + (size_t)me.g * PL_K;
            atomicAdd(a + k0, (unsigned long long)s0);
            atomicAdd(a + k1, (unsigned long long)s1);
            s0 = s1 = 0;
        }
    }
}

// one wave per group, four groups per workgroup
__global__ __launch_bounds__(PL_THREADS) void k_pool_finish(const long long* __restrict__ state, long long groups, int mode,
                                                            float* __restrict__ tmpl, int32_t* __restrict__ count, float* __restrict__ weight,
                                                            float* __restrict__ cohesion, long long* __restrict__ skipped) {
    __shared__ float t[4][PL_K];
    __shared__ float sq[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * 4 + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0 && skipped) *skipped = state[0];
    const bool live = g < groups;
    long long n = 0;
    float wf = 0.f;
    if (live) {
        const long long* a = state + trl_pool_a_at(groups) + (size_t)g * PL_K;
#pragma unroll
        for (int j = 0; j < 8; j++) t[wave][64 * j + lane] = trl_pool_value(a[64 * j + lane]);
        n = state[trl_pool_n_at(groups) + g];
        wf = trl_pool_value(state[trl_pool_w_at(groups) + g]);
    }
    __syncthreads();
    if (live && lane == 0) {
        float acc = 0.f;
#pragma unroll 16
        for (int k = 0; k < PL_K; k++) acc = __builtin_fmaf(t[wave][k], t[wave][k], acc);
        sq[wave] = __builtin_sqrtf(acc);
    }
    __syncthreads();
    if (!live) return;
    const float s = sq[wave];
#pragma unroll
    for (int j = 0; j < 8; j++) tmpl[(size_t)g * PL_K + 64 * j + lane] = trl_pool_element(mode, n, t[wave][64 * j + lane], s, wf);
    if (lane == 0) {
        count[g] = (int32_t)n;
        weight[g] = n == 0 ? 0.f : wf;
        cohesion[g] = trl_pool_cohesion(n, s, wf);
    }
}

template <int ROWS>
__global__ __launch_bounds__(PL_THREADS) void k_pool_rep_add(unsigned long long* __restrict__ key, long long groups, long long g0,
                                                             const float* __restrict__ tmpl, const float* __restrict__ x, long long ld,
                                                             const float* __restrict__ n2, const int32_t* __restrict__ gid,
                                                             const float* __restrict__ w, long long row_base, long long m) {
    constexpr int rows = ROWS;
    const PlFrame f;
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * rows;
    pl_fill<ROWS>(f.tile, f.info, f.order, f.counts, x, ld, n2, gid, w, m, row0, g0, groups);
    if (f.counts[0] == 0) return;
    float* tt = f.tile + rows * PL_PITCH;                                   // slot r: the template row of the group whose first row is r
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(tt + rows * PL_PITCH + (rows & 1));   // (8-byte aligned)
    // eight template rows at a time, their loads in flight together; a row is fetched once per distinct id of the tile
#pragma unroll
    for (int r0 = 0; r0 < rows; r0 += 8) {
        float a[8], b[8];
        bool need[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            need[i] = f.info[r0 + i].first == r0 + i;                        // (uniform over the workgroup)
            if (need[i]) {
                const float* src = tmpl + (size_t)f.info[r0 + i].g * PL_K;
                a[i] = src[tid];
                b[i] = src[tid + 256];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (need[i]) {
                tt[(r0 + i) * PL_PITCH + tid] = a[i];
                tt[(r0 + i) * PL_PITCH + tid + 256] = b[i];
            }
    }
    __syncthreads();
    if (tid < rows) {
        unsigned long long k = 0;
        const PlRow me = f.info[tid];
        if (me.g >= 0) {
            const float* xr = f.tile + tid * PL_PITCH;
            const float* tr = tt + me.first * PL_PITCH;
            float dot = 0.f, n2t = 0.f;
#pragma unroll 8
            for (int i = 0; i < PL_K; i++) {
                dot = __builtin_fmaf(tr[i], xr[i], dot);
                n2t = __builtin_fmaf(tr[i], tr[i], n2t);
            }
            k = trl_best_key(trl_pool_cosine(dot, n2t, me.n2), row_base + row0 + tid);
        }
        keys[tid] = k;
    }
    __syncthreads();
    if (tid < rows && f.info[tid].first == tid) {
        unsigned long long best = 0;
        for (int j = tid; j < rows; j++)
            if (f.info[j].first == tid && keys[j] > best) best = keys[j];
        if (best) atomicMax(key + f.info[tid].g, best);
    }
}

// the read-back of an array of best-row keys: trl_pool_rep_finish's and trl_best_read's (trl_quality.hip)
__global__ __launch_bounds__(PL_THREADS) void k_best_key_read(const unsigned long long* __restrict__ key, long long groups,
                                                              int32_t* __restrict__ index, float* __restrict__ score) {
    const long long g = (long long)blockIdx.x * PL_THREADS + threadIdx.x;
    if (g >= groups) return;
    int32_t i;
    float s;
    trl_best_key_decode(key[g], &i, &s);
    index[g] = i;
    score[g] = s;
}

// the tile a caller's tile_rows means; 0 when the kernels do not support it
int pl_tile(int tile_rows) { return tile_rows == 0 ? PL_TILE_DEFAULT : tile_rows == 8 || tile_rows == 16 || tile_rows == 32 ? tile_rows : 0; }

// what trl_pool_add and trl_pool_rep_add refuse alike
const char* pl_check_rows(long long ld, long long m, long long row0, int tile_rows) {
    if (m < 0 || m > TRL_POOL_MAX_ROWS) return "m outside 0..2^30";
    if (ld < PL_K) return "ld_rows < 512";
    if (row0 < 0 || row0 + m > 0x7fffffffLL) return "row0 + m outside 0..2^31 - 1";
    if (!pl_tile(tile_rows)) return "tile_rows is not 0, 8, 16 or 32";
    return nullptr;
}

// the instantiation for a tile of `rows` rows (pl_tile's values)
#define PL_LAUNCH(kernel, rows, ...)                                                  \
    ((rows) == 8 ? trl_launch_lds(kernel<8>, __VA_ARGS__) : (rows) == 16 ? trl_launch_lds(kernel<16>, __VA_ARGS__) \
                                                                         : trl_launch_lds(kernel<32>, __VA_ARGS__))

}  // namespace

extern "C" size_t trl_pool_state_bytes(long long groups) {
    if (groups < 0 || groups > TRL_POOL_MAX_GROUPS) return 0;
    return (size_t)trl_pool_words(groups) * 8;
}

extern "C" int trl_pool_reset(void* d_state, long long groups, void* stream) {
    TRL_CHECK(trl_check_groups("trl_pool_reset", "state is", d_state, groups));
    TRL_CHECK(trl_device_of(d_state));
    TRL_HIP(hipMemsetAsync(d_state, 0, trl_pool_state_bytes(groups), (hipStream_t)stream));
    return TRL_OK;
}

extern "C" int trl_pool_add(void* d_state, long long groups, long long g0, const float* d_rows, long long ld_rows, const float* d_n2,
                            const int32_t* d_gid, const float* d_w, long long m, int tile_rows, void* stream) {
    const char* who = "trl_pool_add";
    TRL_CHECK(trl_check_groups(who, "state is", d_state, groups));
    if (const char* why = pl_check_rows(ld_rows, m, 0, tile_rows)) return trl_refuse(who, why);
    if (m == 0) return TRL_OK;
    if (!d_rows || !d_gid) return trl_refuse(who, "null argument");
    const int rows = pl_tile(tile_rows);
    TRL_CHECK(trl_device_of(d_state));
    return PL_LAUNCH(k_pool_add, rows, (m + rows - 1) / rows, pl_lds_bytes(rows, 1), (hipStream_t)stream, (unsigned long long*)d_state, groups,
                     g0, d_rows, ld_rows, d_n2, d_gid, d_w, m);
}

extern "C" int trl_pool_finish(const void* d_state, long long groups, int mode, float* d_template, int32_t* d_count, float* d_weight,
                               float* d_cohesion, long long* d_skipped, void* stream) {
    const char* who = "trl_pool_finish";
    TRL_CHECK(trl_check_groups(who, "state is", d_state, groups));
    if (mode != TRL_POOL_UNIT && mode != TRL_POOL_MEAN) return trl_refuse(who, "mode is not 0 (unit) or 1 (mean)");
    if (groups > 0 && (!d_template || !d_count || !d_weight || !d_cohesion)) return trl_refuse(who, "null argument");
    if (groups == 0 && !d_skipped) return TRL_OK;
    TRL_CHECK(trl_device_of(d_state));
    k_pool_finish<<<(unsigned)(groups > 0 ? (groups + 3) / 4 : 1), PL_THREADS, 0, (hipStream_t)stream>>>(
        (const long long*)d_state, groups, mode, d_template, d_count, d_weight, d_cohesion, d_skipped);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_pool_rep_reset(unsigned long long* d_key, long long groups, void* stream) {
    TRL_CHECK(trl_check_groups("trl_pool_rep_reset", "state is", d_key, groups));
    if (groups == 0) return TRL_OK;
    TRL_CHECK(trl_device_of(d_key));
    TRL_HIP(hipMemsetAsync(d_key, 0, (size_t)groups * 8, (hipStream_t)stream));
    return TRL_OK;
}

extern "C" int trl_pool_rep_add(unsigned long long* d_key, long long groups, long long g0, const float* d_template, const float* d_rows,
                                long long ld_rows, const float* d_n2, const int32_t* d_gid, const float* d_w, long long row0, long long m,
                                int tile_rows, void* stream) {
    const char* who = "trl_pool_rep_add";
    TRL_CHECK(trl_check_groups(who, "state is", d_key, groups));
    if (const char* why = pl_check_rows(ld_rows, m, row0, tile_rows)) return trl_refuse(who, why);
    if (m == 0 || groups == 0) return TRL_OK;
    if (!d_template || !d_rows || !d_gid) return trl_refuse(who, "null argument");
    const int rows = pl_tile(tile_rows);
    TRL_CHECK(trl_device_of(d_key));
    return PL_LAUNCH(k_pool_rep_add, rows, (m + rows - 1) / rows, pl_lds_bytes(rows, 2) + (size_t)rows * 8 + 8, (hipStream_t)stream, d_key,
                     groups, g0, d_template, d_rows, ld_rows, d_n2, d_gid, d_w, row0, m);
}

int trl_best_key_read(const char* who, const char* what, const unsigned long long* d_key, long long groups, int32_t* d_index, float* d_score,
                      hipStream_t s) {
    TRL_CHECK(trl_check_groups(who, what, d_key, groups));
    if (groups == 0) return TRL_OK;
    if (!d_index || !d_score) return trl_refuse(who, "null argument");
    TRL_CHECK(trl_device_of(d_key));
    k_best_key_read<<<(unsigned)((groups + PL_THREADS - 1) / PL_THREADS), PL_THREADS, 0, s>>>(d_key, groups, d_index, d_score);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_pool_rep_finish(const unsigned long long* d_key, long long groups, int32_t* d_index, float* d_score, void* stream) {
    return trl_best_key_read("trl_pool_rep_finish", "state is", d_key, groups, d_index, d_score, (hipStream_t)stream);
}

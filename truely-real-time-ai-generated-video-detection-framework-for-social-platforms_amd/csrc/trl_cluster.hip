// trl_cluster.hip -- DBSCAN labels over links that are already there.  No tile, no gallery, no matrix core:
// the links come from trl_gallery.hip, as the packed bitmap of trl_cluster_links (up to 65,536 rows) or as the CSR lists of the range
// search with self = 1 (up to 16,777,216), and the label stage is written once over a NEIGHBOUR SOURCE that enumerates a row's
// neighbours either way.  Labels come from rounds of hooking and pointer jumping, a launch each.  Every kernel below reads buffers
// that no workgroup writes in the same launch, so nothing depends on one workgroup seeing another's stores; a round is a copy and
// two launches (b = a; hook: a -> b; jump: b -> a) and the host decides between small batches of rounds.  Refusals, the workspace
// check and the device lookup are trl_host.h's; the bitmap's row limit, shared with trl_cluster_links, is trl_cluster.h's.
#include <type_traits>

#include "trl_cluster.h"
#include "trl_host.h"
#include "trl_scan.h"

namespace {

constexpr int CL_NONE = 0x7fffffff;   // the label of a row that is not core
constexpr int CL_JUMPS = 32;          // pointer chases of one jump launch (over a buffer the launch does not write)
constexpr int CL_BATCH = 4;           // rounds queued between two looks at the change flags
constexpr int CL_LIST_MAX_N = 1 << 24;

// a thread per row: the row's list length, + 1 for the row itself; 0 for an invalid row
__global__ void k_cluster_list_degree(const long long* __restrict__ offsets, const uint8_t* __restrict__ valid, int n, int32_t* __restrict__ degree) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    degree[i] = (!valid || valid[i] != 0) ? (int)(offsets[i + 1] - offsets[i]) + 1 : 0;
}

__global__ void k_cluster_init(const int32_t* __restrict__ degree, int n, int min_samples, uint8_t* __restrict__ core, int32_t* __restrict__ lab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int d = degree[i];
    const bool c = d > 0 && d >= min_samples;
    core[i] = c;
    lab[i] = c ? i : CL_NONE;
}

// ---- neighbour sources: LANES lanes share a row, and each(row, sub, f) calls f(j) for lane sub's share of the row's neighbours j,
// every one of them in 0 .. n - 1.  The LANES lanes of a row are an aligned group of their wave and leave a kernel together, so the
// xor shuffles of cl_min stay among lanes that are there; a workgroup of 256 threads holds 256 / LANES rows side by side.

// the set bits of row `row` of the link bitmap: one wave per row
struct ClBits {
    static constexpr int LANES = 64;
    const uint32_t* __restrict__ adj;
    long long pitch;
    int n, words;
    template <typename F>
    __device__ __forceinline__ void each(long long row, int sub, F&& f) const {
        const uint32_t* a = adj + (size_t)row * (size_t)pitch;
        for (int w = sub; w < words; w += LANES) {
            uint32_t bits = a[w];
            if (w == words - 1 && (n & 31)) bits &= (1u << (n & 31)) - 1u;      // (a caller's bitmap is never followed past n)
            while (bits) {
                const int b = __ffs(bits) - 1;
                bits &= bits - 1;
                f(32 * w + b);
            }
        }
    }
};

// the entries of the CSR list index[offsets[row] .. offsets[row + 1]).  Lists of face clusters hold tens of entries, so a row is
// walked by L = 4 / 16 / 64 lanes.  An entry outside 0 .. n - 1 is skipped, never followed.
template <int L>
struct ClList {
    static constexpr int LANES = L;
    const long long* __restrict__ offsets;
    const int32_t* __restrict__ index;
    int n;
    template <typename F>
    __device__ __forceinline__ void each(long long row, int sub, F&& f) const {
        const long long end = offsets[row + 1];
        for (long long p = offsets[row] + sub; p < end; p += L) {
            const uint32_t j = (uint32_t)index[p];
            if (j < (uint32_t)n) f((int)j);
        }
    }
};

// the smallest of f(label of j) over the neighbours j of `row`, by the lanes that share the row (each of them returns it); rows that
// are not core carry CL_NONE and drop out of the minimum by themselves
template <typename Src, typename F>
__device__ __forceinline__ int cl_min(const Src& src, long long row, int sub, const int32_t* __restrict__ lab, F&& f) {
    int m = CL_NONE;
    src.each(row, sub, [&](int j) __attribute__((always_inline)) {
        const int v = f(lab[j]);
        m = v < m ? v : m;
    });
#pragma unroll
    for (int off = Src::LANES / 2; off >= 1; off >>= 1) {
        const int o = __shfl_xor(m, off, 64);
        m = o < m ? o : m;
    }
    return m;
}

// per core row: m = the smallest label among the row's core neighbours; where m is below the row's own label, both the row and the
// row its label names (its tree's root, after a jump) take it: out[row] = min(out[row], m), out[own] = min(out[own], m).
// `out` is a copy of `in` made in front of the launch and this launch touches it with atomicMin only -- never a plain store beside
// an atomic on one line -- and min commutes, so `out` does not depend on the order the waves run in.  *changed likewise is only
// ever touched by atomics, the memset in front of the batch and the copy behind it, and lies in an allocation of its own.
template <typename Src>
__device__ __forceinline__ void cl_hook(const Src& src, int n, const int32_t* __restrict__ in, int32_t* out, int* changed) {
    const int sub = threadIdx.x & (Src::LANES - 1);
    const long long row = (long long)blockIdx.x * (256 / Src::LANES) + threadIdx.x / Src::LANES;
    if (row >= n) return;
    const int own = in[row];
    if (own == CL_NONE) return;
    const int m = cl_min(src, row, sub, in, [](int l) { return l; });
    if (sub == 0 && m < own) {
        atomicMin(out + row, m);
        atomicMin(out + own, m);
        atomicOr(changed, 1);
    }
}

// per row: a core row takes its root's number; a valid row that is not core the smallest number among its core neighbours' clusters
// (a border row), -1 without one (noise); an invalid row -1
template <typename Src>
__device__ __forceinline__ void cl_assign(const Src& src, const int32_t* __restrict__ degree, int n, const int32_t* __restrict__ lab,
                                          const int32_t* __restrict__ cid, int32_t* __restrict__ labels) {
    const int sub = threadIdx.x & (Src::LANES - 1);
    const long long row = (long long)blockIdx.x * (256 / Src::LANES) + threadIdx.x / Src::LANES;
    if (row >= n) return;
    const int own = lab[row];
    int out = -1;
    if (own != CL_NONE) {
        out = cid[own];
    } else if (degree[row] > 0) {
        const int m = cl_min(src, row, sub, lab, [&](int l) { return l == CL_NONE ? CL_NONE : cid[l]; });
        out = m == CL_NONE ? -1 : m;
    }
    if (sub == 0) labels[row] = out;
}

__global__ __launch_bounds__(256) void k_cluster_hook(const uint32_t* __restrict__ adj, long long pitch, int n, int words,
                                                      const int32_t* __restrict__ in, int32_t* out, int* changed) {
    cl_hook(ClBits{adj, pitch, n, words}, n, in, out, changed);
}

__global__ __launch_bounds__(256) void k_cluster_assign(const uint32_t* __restrict__ adj, long long pitch, const int32_t* __restrict__ degree,
                                                        int n, int words, const int32_t* __restrict__ lab, const int32_t* __restrict__ cid,
                                                        int32_t* __restrict__ labels) {
    cl_assign(ClBits{adj, pitch, n, words}, degree, n, lab, cid, labels);
}

template <int L>
__global__ __launch_bounds__(256) void k_cluster_list_hook(const long long* __restrict__ offsets, const int32_t* __restrict__ index, int n,
                                                           const int32_t* __restrict__ in, int32_t* out, int* changed) {
    cl_hook(ClList<L>{offsets, index, n}, n, in, out, changed);
}

template <int L>
__global__ __launch_bounds__(256) void k_cluster_list_assign(const long long* __restrict__ offsets, const int32_t* __restrict__ index,
                                                             const int32_t* __restrict__ degree, int n, const int32_t* __restrict__ lab,
                                                             const int32_t* __restrict__ cid, int32_t* __restrict__ labels) {
    cl_assign(ClList<L>{offsets, index, n}, degree, n, lab, cid, labels);
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
// Thread t owns rows t * per .. + per - 1.
__global__ __launch_bounds__(1024) void k_cluster_number(const int32_t* __restrict__ lab, int n, int per, int32_t* __restrict__ cid,
                                                         int32_t* __restrict__ count) {
    const int t = threadIdx.x;
    const int lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    int c = 0;
    for (int i = lo; i < hi; i++) c += lab[i] == i;
    int base = trl_scan_1024(c);
    if (t == 1023) *count = base + c;
    for (int i = lo; i < hi; i++) cid[i] = lab[i] == i ? base++ : -1;
}

// the label stage's workspace, carved once: cl_workspace is a dry run of this
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

size_t cl_workspace(int n, int max_n) {
    if (n < 0 || n > max_n) return 0;
    Arena a = Arena::counter(0);
    ClWs w;
    cl_carve(a, n, &w);
    return a.high;
}

// The rounds: copy, hook (a -> b, launched by `hook` with the round's change flag) and jump (b -> a) until a round changes nothing,
// CL_BATCH rounds queued between two looks at the flags.  Every round before the last lowers at least one label, and a label is at
// least 0 and at most its row's index -- whatever the links hold -- so the loop ends; the bound of n rounds is a second line of
// defence.  *rounds_out (may be null): the rounds up to and including the first that changed nothing.
template <typename Hook>
int cl_rounds(const char* who, const ClWs& w, int n, hipStream_t s, int* rounds_out, Hook&& hook) {
    int rounds = 0;
    for (bool done = false; !done;) {
        if (rounds >= n + CL_BATCH) { trl_set_error("%s: no fixed point after %d rounds", who, rounds); return TRL_ERR_STATE; }
        TRL_HIP(hipMemsetAsync(w.changed, 0, CL_BATCH * sizeof(int), s));
        for (int r = 0; r < CL_BATCH; r++) {
            TRL_HIP(hipMemcpyAsync(w.b, w.a, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            hook(w, w.changed + r);
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

// Either entry: checks, carve, init, rounds, number, assign.  `accept` is the entry's own check of its arguments, run where the entries
// have always run it: false with the error set when it refuses; `prepare` runs in front of k_cluster_init and may fill d_degree; `hook` and
// `assign` launch the source's kernels over the carved workspace.
template <typename Accept, typename Prepare, typename Hook, typename Assign>
int cl_labels(const char* who, int max_n, Accept&& accept, bool links_null, const int32_t* d_degree, int n, int min_samples,
              int32_t* d_labels, uint8_t* d_core, int32_t* d_count, void* d_ws, size_t ws_bytes, int* rounds_out, hipStream_t s,
              Prepare&& prepare, Hook&& hook, Assign&& assign) {
    if (n < 0 || n > max_n) { trl_set_error("%s: n = %d outside 0..%d", who, n, max_n); return TRL_ERR_INVALID; }
    if (min_samples < 1) { trl_set_error("%s: min_samples = %d < 1", who, min_samples); return TRL_ERR_INVALID; }
    if (!accept()) return TRL_ERR_INVALID;
    if (!d_count) return trl_refuse(who, "null count");
    if (n > 0 && (links_null || !d_degree || !d_labels || !d_core)) return trl_refuse(who, "null argument");
    Arena a = Arena::over(d_ws, ws_bytes);
    ClWs w;
    if (n > 0 && !trl_workspace_ok(who, d_ws, ws_bytes, cl_carve(a, n, &w), [&] { return cl_workspace(n, max_n); })) return TRL_ERR_INVALID;
    TRL_CHECK(trl_device_of(d_count));
    if (rounds_out) *rounds_out = 0;
    if (n == 0) {
        TRL_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
        return TRL_OK;
    }
    TRL_CHECK(prepare());
    k_cluster_init<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(d_degree, n, min_samples, d_core, w.a);
    TRL_LAUNCH_CHECK();
    TRL_CHECK(cl_rounds(who, w, n, s, rounds_out, hook));
    k_cluster_number<<<1, 1024, 0, s>>>(w.a, n, (n + 1023) / 1024, w.cid, d_count);
    TRL_LAUNCH_CHECK();
    assign(w);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

unsigned cl_grid(int n, int lanes) { return (unsigned)((n + 256 / lanes - 1) / (256 / lanes)); }

// the lanes per row for lists of `mean` entries on average, from profiles/cluster_lists_kernel_stats.csv: at
// the sizes this stage is for, 4 lanes win up to lists of 127 and 16 lanes at 1,023; 64 lanes won nowhere past 1,024 rows
int cl_list_lanes(long long mean) { return mean < 384 ? 4 : 16; }

// f(the lanes per row as a compile-time constant)
template <typename F>
void cl_with_lanes(int lanes, F&& f) {
    if (lanes == 4) f(std::integral_constant<int, 4>{});
    else if (lanes == 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}

}  // namespace

extern "C" size_t trl_cluster_workspace(int n) { return cl_workspace(n, CL_MAX_N); }

extern "C" int trl_cluster_labels(const uint32_t* d_adj, long long pitch_words, const int32_t* d_degree, int n, int min_samples,
                                  int32_t* d_labels, uint8_t* d_core, int32_t* d_count, void* d_ws, size_t ws_bytes, int* rounds_out,
                                  void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int words = (int)(((long long)n + 31) / 32);
    return cl_labels(
        "trl_cluster_labels", CL_MAX_N,
        [&] {
            if (pitch_words < words) trl_set_error("trl_cluster_labels: pitch_words = %lld < %d", pitch_words, words);
            return pitch_words >= words;
        },
        !d_adj, d_degree, n, min_samples, d_labels, d_core, d_count,
        d_ws, ws_bytes, rounds_out, s, []() -> int { return TRL_OK; },
        [&](const ClWs& w, int* changed) { k_cluster_hook<<<cl_grid(n, 64), 256, 0, s>>>(d_adj, pitch_words, n, words, w.a, w.b, changed); },
        [&](const ClWs& w) { k_cluster_assign<<<cl_grid(n, 64), 256, 0, s>>>(d_adj, pitch_words, d_degree, n, words, w.a, w.cid, d_labels); });
}

extern "C" size_t trl_cluster_lists_workspace(int n) { return cl_workspace(n, CL_LIST_MAX_N); }

extern "C" int trl_cluster_labels_lists(const long long* d_offsets, const int32_t* d_index, const uint8_t* d_valid, int n, int min_samples,
                                        int lanes_per_row, int32_t* d_degree, int32_t* d_labels, uint8_t* d_core, int32_t* d_count,
                                        void* d_ws, size_t ws_bytes, int* rounds_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int L = lanes_per_row;
    return cl_labels(
        "trl_cluster_labels_lists", CL_LIST_MAX_N,
        [&] {
            const bool ok = L == 0 || L == 4 || L == 16 || L == 64;
            if (!ok) trl_set_error("trl_cluster_labels_lists: lanes_per_row = %d (0, 4, 16 or 64)", L);
            return ok;
        },
        !d_offsets || !d_index, d_degree,
        n, min_samples, d_labels, d_core, d_count, d_ws, ws_bytes, rounds_out, s,
        [&]() -> int {
            if (L == 0) {             // the mean list length decides; the round loop waits for the stream anyway
                long long total = 0;
                TRL_HIP(hipMemcpyAsync(&total, d_offsets + n, sizeof(total), hipMemcpyDeviceToHost, s));
                TRL_HIP(hipStreamSynchronize(s));
                L = cl_list_lanes(total / n);
            }
            k_cluster_list_degree<<<cl_grid(n, 1), 256, 0, s>>>(d_offsets, d_valid, n, d_degree);
            TRL_LAUNCH_CHECK();
            return TRL_OK;
        },
        [&](const ClWs& w, int* changed) {
            cl_with_lanes(L, [&](auto LANES) {
                k_cluster_list_hook<decltype(LANES)::value><<<cl_grid(n, LANES), 256, 0, s>>>(d_offsets, d_index, n, w.a, w.b, changed);
            });
        },
        [&](const ClWs& w) {
            cl_with_lanes(L, [&](auto LANES) {
                k_cluster_list_assign<decltype(LANES)::value><<<cl_grid(n, LANES), 256, 0, s>>>(d_offsets, d_index, d_degree, n, w.a, w.cid, d_labels);
            });
        });
}

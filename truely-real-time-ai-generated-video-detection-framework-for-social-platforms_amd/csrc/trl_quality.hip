// trl_quality.hip -- face quality ("Face quality"; section 7, f-14): per face row the integer sums of luma and
// Laplacian over its rectangle of the source frame, the float chains on top of them, and the best shot of each group of rows.
// The rules are trl_quality.h's; this file is their schedule.  Context-free, like trl_draw and the gallery.
//
// k_quality_accum: the grid is faces x row bands.  A workgroup takes a band of its face's rectangle: the band's luma goes once into
// LDS as bytes, one halo row above and one below (reflected at the rectangle's edges), from reads that walk the BGR rows in address
// order; the Laplacian, its square and the histogram (integer LDS atomics, one copy per wave) come from LDS.  A workgroup that has
// more than one band (a tall rectangle, a small max_band_rows) keeps summing, and leaves with ONE round of global atomics: two
// 64-bit adds and the non-empty bins.  Integer adds commute, so the bits depend on neither the band height nor the arrival order.
// The accumulators live in the caller's workspace, zeroed on the stream in front of the kernel.
// k_quality_finish: one wave per face reads N, the sums of Y and Y^2, the clipped counts and the two percentiles off the histogram
// (a lane holds four bins; one scan) and lane 0 runs the float chains of trl_quality.h.
// Best shots: the key is trl_bestkey.h's (the templates' representative key), and trl_best_read ends in trl_pool.hip's
// trl_best_key_read.  The entry points' checks and device lookup are trl_host.h's; the workspace is carved over an Arena (ql_carve).
#include "trl_bestkey.h"
#include "trl_host.h"
#include "trl_quality.h"

namespace {

constexpr int QL_THREADS = 256;
constexpr int QL_WAVES = QL_THREADS / 64;
constexpr int QL_BAND_DEFAULT = 32;
constexpr int QL_LDS_MIN = 16384;                       // bytes of luma a workgroup holds: at least this, at least three frame rows
constexpr int QL_LDS_MAX = 3 * TRL_QUALITY_MAX_DIM;     // 48 KiB
constexpr int QL_GRID_BANDS = 64;                       // band slots of the grid; a workgroup strides over its face's bands

__device__ __forceinline__ long long ql_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(QL_THREADS) void k_quality_accum(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                              const int32_t* __restrict__ frame_of, const float* __restrict__ boxes,
                                                              int band_rows, int lds_luma, unsigned long long* __restrict__ sums,
                                                              int32_t* __restrict__ hists) {
    extern __shared__ long long ql_lds[];
    long long* part = ql_lds;                                               // [QL_WAVES][2]
    int* hist = reinterpret_cast<int*>(part + 2 * QL_WAVES);                // [QL_WAVES][256]
    uint8_t* luma = reinterpret_cast<uint8_t*>(hist + QL_WAVES * TRL_QUALITY_BINS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = blockIdx.y;
    int rect[4];
    const float box[4] = {boxes[4 * r], boxes[4 * r + 1], boxes[4 * r + 2], boxes[4 * r + 3]};
    const int f = frame_of[r];
    if (!trl_quality_rect(f, n, H, W, box, rect)) return;
    const int w = rect[2] - rect[0], h = rect[3] - rect[1];
    int rows = lds_luma / w - 2;                                            // >= 1: lds_luma >= 3 W
    if (rows > band_rows) rows = band_rows;
    const int bands = (h + rows - 1) / rows;
    if ((int)blockIdx.x >= bands) return;
    for (int i = tid; i < QL_WAVES * TRL_QUALITY_BINS; i += QL_THREADS) hist[i] = 0;
    const uint8_t* src = frames + ((size_t)f * (size_t)H + (size_t)rect[1]) * (size_t)W * 3 + (size_t)rect[0] * 3;
    const int dq = QL_THREADS / w, dr = QL_THREADS % w, j0 = tid / w, c0 = tid % w;
    int* myhist = hist + wave * TRL_QUALITY_BINS;
    long long sl = 0, sl2 = 0;
    for (int band = blockIdx.x; band < bands; band += gridDim.x) {
        const int y0 = band * rows, live = h - y0 < rows ? h - y0 : rows;
        __syncthreads();                                                    // (the histogram is zero; the last band's luma is read)
        // rows y0 - 1 .. y0 + live of the rectangle -> luma rows 0 .. live + 1
        for (int i = tid, j = j0, c = c0; i < (live + 2) * w; i += QL_THREADS) {
            const int y = trl_quality_reflect(y0 - 1 + j, h);
            const uint8_t* p = src + ((size_t)y * (size_t)W + (size_t)c) * 3;
            luma[i] = (uint8_t)trl_quality_luma(p[0], p[1], p[2]);          // (i == j w + c)
            c += dr, j += dq;
            if (c >= w) c -= w, j++;
        }
        __syncthreads();
        for (int i = tid, j = j0, c = c0; i < live * w; i += QL_THREADS) {
            const uint8_t* row = luma + (j + 1) * w;
            const int v = row[c];
            const int L = trl_quality_laplacian(v, row[c - w], row[c + w], row[trl_quality_reflect(c - 1, w)], row[trl_quality_reflect(c + 1, w)]);
            sl += L;
            sl2 += L * L;
            atomicAdd(myhist + v, 1);
            c += dr, j += dq;
            if (c >= w) c -= w, j++;
        }
    }
    sl = ql_wave_sum(sl), sl2 = ql_wave_sum(sl2);
    if (lane == 0) part[2 * wave] = sl, part[2 * wave + 1] = sl2;
    __syncthreads();
    if (tid < 2) {
        long long s = 0;
        for (int v = 0; v < QL_WAVES; v++) s += part[2 * v + tid];
        if (s) atomicAdd(sums + 2 * r + tid, (unsigned long long)s);
    }
    int c = 0;
#pragma unroll
    for (int v = 0; v < QL_WAVES; v++) c += hist[v * TRL_QUALITY_BINS + tid];   // (QL_THREADS == TRL_QUALITY_BINS)
    if (c) atomicAdd(hists + (size_t)r * TRL_QUALITY_BINS + tid, c);
}
static_assert(QL_THREADS == TRL_QUALITY_BINS, "a thread per bin");

// one wave per face, four faces per workgroup
__global__ __launch_bounds__(QL_THREADS) void k_quality_finish(int n, int H, int W, const int32_t* __restrict__ frame_of,
                                                               const float* __restrict__ boxes, const float* __restrict__ points,
                                                               long long m, trl_quality_params prm, const long long* __restrict__ sums,
                                                               const int32_t* __restrict__ hists, long long* __restrict__ raw_out,
                                                               float* __restrict__ feat_out, int32_t* __restrict__ hist_out,
                                                               int32_t* __restrict__ status_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * QL_WAVES + wave;
    if (r >= m) return;
    int rect[4];
    const float box[4] = {boxes[4 * r], boxes[4 * r + 1], boxes[4 * r + 2], boxes[4 * r + 3]};
    const int status = trl_quality_rect(frame_of[r], n, H, W, box, rect);
    const int2* hp = reinterpret_cast<const int2*>(hists + (size_t)r * TRL_QUALITY_BINS + 4 * lane);    // bins 4 lane .. 4 lane + 3
    const int2 b0 = hp[0], b1 = hp[1];                                      // (the workspace is 8-byte aligned)
    const int c[4] = {b0.x, b0.y, b1.x, b1.y};
    if (hist_out) {
#pragma unroll
        for (int k = 0; k < 4; k++) hist_out[(size_t)r * TRL_QUALITY_BINS + 4 * lane + k] = c[k];
    }
    const int mine = c[0] + c[1] + c[2] + c[3];
    int incl = mine;                                                        // N <= 2^28
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    const long long N = __shfl(incl, 63, 64);
    const long long dark = __shfl(incl, 3, 64), bright = N - __shfl(incl, 59, 64);
    long long s1 = 0, s2 = 0, cum = incl - mine;
    int p05 = TRL_QUALITY_BINS, p95 = TRL_QUALITY_BINS;
#pragma unroll
    for (int k = 3; k >= 0; k--) {                                          // (descending: the smallest bin that qualifies stays)
        long long ck = cum;
#pragma unroll
        for (int i = 0; i <= k; i++) ck += c[i];
        const int v = 4 * lane + k;
        if (20 * ck >= N) p05 = v;
        if (20 * ck >= 19 * N) p95 = v;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long v = 4 * lane + k;
        s1 += v * c[k], s2 += v * v * c[k];
    }
    s1 = ql_wave_sum(s1), s2 = ql_wave_sum(s2);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int a = __shfl_xor(p05, d, 64), e = __shfl_xor(p95, d, 64);
        p05 = a < p05 ? a : p05, p95 = e < p95 ? e : p95;
    }
    if (lane != 0) return;
    long long raw[TRL_QUALITY_RAW];
    raw[TRL_QR_N] = N, raw[TRL_QR_SY] = s1, raw[TRL_QR_SY2] = s2, raw[TRL_QR_SL] = sums[2 * r], raw[TRL_QR_SL2] = sums[2 * r + 1];
    raw[TRL_QR_DARK] = dark, raw[TRL_QR_BRIGHT] = bright, raw[TRL_QR_WIDTH] = rect[2] - rect[0];
    const int p[2] = {p05, p95};
    float pts[10], feat[TRL_QUALITY_FEAT];
#pragma unroll
    for (int i = 0; i < 10; i++) pts[i] = points ? points[10 * r + i] : 0.f;
    trl_quality_features(status, raw, p, rect[3] - rect[1], points != nullptr, pts, prm, feat);
#pragma unroll
    for (int i = 0; i < TRL_QUALITY_RAW; i++) raw_out[TRL_QUALITY_RAW * r + i] = raw[i];
#pragma unroll
    for (int i = 0; i < TRL_QUALITY_FEAT; i++) feat_out[TRL_QUALITY_FEAT * r + i] = feat[i];
    status_out[r] = status;
}

// ---- best shots -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QL_THREADS) void k_best_max(unsigned long long* __restrict__ keys, long long groups,
                                                         const float* __restrict__ quality, const int32_t* __restrict__ gid, long long m,
                                                         long long row_base) {
    const long long r = (long long)blockIdx.x * QL_THREADS + threadIdx.x;
    if (r >= m) return;
    const long long g = gid[r];
    const unsigned long long key = trl_best_key(quality[r], row_base + r);
    if (key && g >= 0 && g < groups) atomicMax(keys + g, key);
}

// a workgroup per row: the row that is its group's best copies its face
__global__ __launch_bounds__(QL_THREADS) void k_best_copy(const unsigned long long* __restrict__ keys, long long groups,
                                                          const float* __restrict__ quality, const int32_t* __restrict__ gid,
                                                          long long row_base, const uint32_t* __restrict__ faces, long long face_floats,
                                                          uint32_t* __restrict__ best) {
    const long long r = blockIdx.x, g = gid[r];
    if (g < 0 || g >= groups) return;
    const unsigned long long key = trl_best_key(quality[r], row_base + r);
    if (!key || keys[g] != key) return;
    const uint32_t* src = faces + (size_t)r * (size_t)face_floats;
    uint32_t* dst = best + (size_t)g * (size_t)face_floats;
    for (long long i = threadIdx.x; i < face_floats; i += QL_THREADS) dst[i] = src[i];
}

// the workspace of m face rows: per face the histogram (int32), then per face sum L, sum L^2 (int64).  trl_quality_workspace is a dry
// run of this; a histogram is 1024 bytes, so the sums start where the histograms end and the blocks hold 1040 m bytes together
bool ql_carve(Arena& a, long long m, int32_t** hists, unsigned long long** sums) {
    *hists = (int32_t*)a.alloc((size_t)m * TRL_QUALITY_BINS * sizeof(int32_t));
    *sums = (unsigned long long*)a.alloc((size_t)m * 2 * sizeof(unsigned long long));
    return *hists && *sums;
}

}  // namespace

extern "C" size_t trl_quality_workspace(long long m) {
    if (m < 0 || m > TRL_QUALITY_MAX_ROWS) return 0;
    Arena a = Arena::counter(0);
    int32_t* hists;
    unsigned long long* sums;
    ql_carve(a, m > 0 ? m : 1, &hists, &sums);
    return a.high;
}

extern "C" int trl_face_quality(const uint8_t* d_frames, int n, int H, int W, const int32_t* d_frame_of, const float* d_boxes,
                                const float* d_points, long long m, const trl_quality_params* params, int max_band_rows, void* d_ws,
                                size_t ws_bytes, long long* d_raw, float* d_feat, int32_t* d_hist, int32_t* d_status, void* stream) {
    const char* who = "trl_face_quality";
    if (m < 0 || m > TRL_QUALITY_MAX_ROWS) return trl_refuse(who, "m outside 0..2^24");
    if (n < 0) return trl_refuse(who, "n < 0");
    if (H < 1 || H > TRL_QUALITY_MAX_DIM || W < 1 || W > TRL_QUALITY_MAX_DIM) return trl_refuse(who, "H or W outside 1..16384");
    if (max_band_rows < 0) return trl_refuse(who, "max_band_rows < 0");
    const trl_quality_params prm = params ? *params : trl_quality_defaults();
    if (!trl_quality_params_ok(prm)) return trl_refuse(who, "a reference of the params is not finite and > 0");
    if (m == 0) return TRL_OK;
    if ((!d_frames && n > 0) || !d_frame_of || !d_boxes || !d_raw || !d_feat || !d_status) return trl_refuse(who, "null argument");
    if (!d_ws) return trl_refuse(who, "null workspace");
    Arena a = Arena::over(d_ws, ws_bytes);
    int32_t* hists;
    unsigned long long* sums;
    if (!trl_workspace_ok(who, d_ws, ws_bytes, ql_carve(a, m, &hists, &sums), [&] { return trl_quality_workspace(m); })) return TRL_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_device_of(d_ws));
    TRL_HIP(hipMemsetAsync(d_ws, 0, a.high, s));
    const int band_rows = max_band_rows ? max_band_rows : QL_BAND_DEFAULT;
    int lds_luma = (3 * W + 7) & ~7;
    if (lds_luma < QL_LDS_MIN) lds_luma = QL_LDS_MIN;
    int fit = lds_luma / W - 2;                                              // band rows of a rectangle as wide as the frame
    if (fit > band_rows) fit = band_rows;
    int slots = (H + fit - 1) / fit;
    if (slots > QL_GRID_BANDS) slots = QL_GRID_BANDS;
    const size_t lds = (size_t)QL_WAVES * 16 + (size_t)QL_WAVES * TRL_QUALITY_BINS * 4 + (size_t)lds_luma;
    static_assert((size_t)QL_WAVES * 16 + (size_t)QL_WAVES * TRL_QUALITY_BINS * 4 + QL_LDS_MAX <= 65536, "LDS of k_quality_accum");
    for (long long r0 = 0; r0 < m; r0 += 65535) {                           // (grid.y)
        const long long rows = m - r0 < 65535 ? m - r0 : 65535;
        k_quality_accum<<<dim3((unsigned)slots, (unsigned)rows), QL_THREADS, lds, s>>>(d_frames, n, H, W, d_frame_of + r0, d_boxes + 4 * r0,
                                                                                     band_rows, lds_luma, sums + 2 * r0,
                                                                                     hists + (size_t)r0 * TRL_QUALITY_BINS);
        TRL_LAUNCH_CHECK();
    }
    k_quality_finish<<<(unsigned)((m + QL_WAVES - 1) / QL_WAVES), QL_THREADS, 0, s>>>(n, H, W, d_frame_of, d_boxes, d_points, m, prm,
                                                                                    (const long long*)sums, hists, d_raw, d_feat, d_hist,
                                                                                    d_status);
    TRL_LAUNCH_CHECK();
    return TRL_OK;
}

extern "C" int trl_best_update(unsigned long long* d_keys, long long groups, const float* d_quality, const int32_t* d_gid, long long m,
                               long long row_base, const float* d_faces, long long face_floats, float* d_best_faces, void* stream) {
    const char* who = "trl_best_update";
    TRL_CHECK(trl_check_groups(who, "keys are", d_keys, groups));
    if (m < 0 || row_base < 0 || row_base + m > 0x7fffffffLL) return trl_refuse(who, "row_base + m outside 0..2^31 - 1");
    if ((d_faces != nullptr) != (d_best_faces != nullptr)) return trl_refuse(who, "faces without best_faces, or the reverse");
    if (d_faces && face_floats < 1) return trl_refuse(who, "face_floats < 1");
    if (m == 0 || groups == 0) return TRL_OK;
    if (!d_quality || !d_gid) return trl_refuse(who, "null argument");
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_device_of(d_keys));
    k_best_max<<<(unsigned)((m + QL_THREADS - 1) / QL_THREADS), QL_THREADS, 0, s>>>(d_keys, groups, d_quality, d_gid, m, row_base);
    TRL_LAUNCH_CHECK();
    if (d_faces) {
        k_best_copy<<<(unsigned)m, QL_THREADS, 0, s>>>(d_keys, groups, d_quality, d_gid, row_base, (const uint32_t*)d_faces, face_floats,
                                                      (uint32_t*)d_best_faces);
        TRL_LAUNCH_CHECK();
    }
    return TRL_OK;
}

extern "C" int trl_best_read(const unsigned long long* d_keys, long long groups, int32_t* d_row, float* d_quality, void* stream) {
    return trl_best_key_read("trl_best_read", "keys are", d_keys, groups, d_row, d_quality, (hipStream_t)stream);
}

// trl_api.hip -- C ABI of libtruely_hip.so (see include/truely_hip.h for the contract and the
// reference lines each entry point replaces).
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>

#include "trl_ctx.h"

static thread_local char g_err[512] = "";
int g_trl_no_fnconv = 0;
int g_trl_pnet_gate = 0;

#include <mutex>
namespace {
std::mutex g_gate_mu;
hipEvent_t g_gate_ev[64] = {};
bool g_gate_set[64] = {};
}
int trl_gate_wait(trl_ctx* c, hipStream_t s) {
    const int d = c->cfg.device;
    if (!g_trl_pnet_gate || d < 0 || d >= 64) return TRL_OK;
    std::lock_guard<std::mutex> lk(g_gate_mu);
    if (g_gate_set[d]) TRL_HIP(hipStreamWaitEvent(s, g_gate_ev[d], 0));
    return TRL_OK;
}
int trl_gate_record(trl_ctx* c, hipStream_t s) {
    const int d = c->cfg.device;
    if (!g_trl_pnet_gate || d < 0 || d >= 64) return TRL_OK;
    std::lock_guard<std::mutex> lk(g_gate_mu);
    if (!g_gate_ev[d]) TRL_HIP(hipEventCreateWithFlags(&g_gate_ev[d], hipEventDisableTiming));
    TRL_HIP(hipEventRecord(g_gate_ev[d], s));
    g_gate_set[d] = true;
    return TRL_OK;
}
void trl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" {

int trl_abi_version(void) { return TRL_ABI_VERSION; }
const char* trl_last_error(void) { return g_err; }

int trl_default_config(trl_config* cfg) {
    if (!cfg) return TRL_ERR_INVALID;
    cfg->device = 0;
    cfg->min_face_size = 20;           // facenet_pytorch MTCNN.__init__ defaults (server/model.py:18)
    cfg->thr0 = 0.6f; cfg->thr1 = 0.7f; cfg->thr2 = 0.7f;
    cfg->factor = 0.709;
    cfg->cap_level = 2048;
    cfg->cap_frame = 2048;
    cfg->max_faces = 64;
    cfg->pnet_mode = 0;
    cfg->embed_mode = 0;
    cfg->embed_precision = 0;
    return TRL_OK;
}

int trl_create(const trl_config* cfg, trl_ctx** out) {
    if (!cfg || !out) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    if (cfg->cap_level < 64 || cfg->cap_level > (1 << 24) || cfg->cap_frame < 64 || cfg->cap_frame > (1 << 24) || (cfg->cap_level & 3) ||
        (cfg->cap_frame & 3) || cfg->min_face_size < 12 || cfg->max_faces < 1 || !(cfg->factor > 0.1 && cfg->factor < 0.99) || cfg->embed_mode < 0 || cfg->embed_mode > 3 ||
        cfg->embed_precision < 0 || cfg->embed_precision > 2) {
        trl_set_error("bad trl_config (list start capacities must be multiples of 4 in [64, 2^24], min_face_size >= 12)");
        return TRL_ERR_INVALID;
    }
    TRL_HIP(hipSetDevice(cfg->device));
    trl_ctx* c = new trl_ctx();
    c->cfg = *cfg;
    // execution span of every fused PNet launch (two atomics per workgroup, summed on the device: trl_debug_pnet_span);
    // TRL_PNET_CLOCK additionally selects the DBG instantiation with per-phase wave clocks
    c->pnet_prof = trl_tune_set("TRL_PNET_CLOCK");
    if (hipMalloc((void**)&c->pnet_clk, 8 * 44) != hipSuccess || hipMemset(c->pnet_clk, 0, 8 * 44) != hipSuccess || hipMemset(c->pnet_clk, 0xFF, 8) != hipSuccess ||
        hipMalloc((void**)&c->pnet_cursor, 64) != hipSuccess || hipHostMalloc((void**)&c->h_pinned, 1024) != hipSuccess ||
        hipEventCreate(&c->ev_call0) != hipSuccess || hipEventCreate(&c->ev_call1) != hipSuccess) {
        trl_set_error("context allocation failed: %s", hipGetErrorString(hipGetLastError()));
        trl_destroy(c);                      // frees whatever was created
        return TRL_ERR_HIP;
    }
    memset(c->h_pinned, 0, 1024);
    *out = c;
    return TRL_OK;
}

int trl_destroy(trl_ctx* c) {
    if (!c) return TRL_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();            // (also ends a call that was queued and never finished: its kernels are done)
    c->pend.active = false;
    trl_free_weights(c);
    if (c->arena.base) (void)hipFree(c->arena.base);
    if (c->scratch.base) (void)hipFree(c->scratch.base);
    if (c->sims_tmp.base) (void)hipFree(c->sims_tmp.base);
    if (c->pyr_tab) (void)hipFree(c->pyr_tab);
    if (c->rz.dev) (void)hipFree(c->rz.dev);
    for (auto& b : c->fn_cap) if (b.p) (void)hipFree(b.p);
    if (c->pnet_clk) {
        // TRL_PNET_CLOCK: where the waves of the fused PNet launches spent their time (shader clocks per tile and wave, DBG instantiation)
        unsigned long long t[42];
        if (c->pnet_prof && hipMemcpy(t, c->pnet_clk, sizeof t, hipMemcpyDeviceToHost) == hipSuccess && t[2 + 32] > 0) {
            static const char* nm[8] = {"phase0", "barrier0", "phase1", "barrier1", "phase2", "barrier2", "phase3", "barrier3"};
            const double tiles = (double)t[2 + 32];
            fprintf(stderr, "[TRL_PNET_CLOCK] shader clocks per tile (wave 0..3), %.0f workgroup-tiles\n", tiles);
            for (int k = 0; k < 8; k++)
                fprintf(stderr, "[TRL_PNET_CLOCK] %-9s %8.0f %8.0f %8.0f %8.0f\n", nm[k], t[2 + k] / tiles, t[2 + 8 + k] / tiles, t[2 + 16 + k] / tiles, t[2 + 24 + k] / tiles);
            fprintf(stderr, "[TRL_PNET_CLOCK] fp16 screen: %llu M-tiles screened, %llu confirmed (%.2f %%)\n", t[39], t[40],
                    t[39] ? 100.0 * (double)t[40] / (double)t[39] : 0.0);
            fprintf(stderr, "[TRL_PNET_CLOCK] confirm queue: %llu M-tiles queued, %.0f per launch\n", t[41], t[37] ? (double)t[41] / (double)t[37] : 0.0);
        }
        (void)hipFree(c->pnet_clk);
    }
    if (c->pnet_cursor) (void)hipFree(c->pnet_cursor);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->ev_call0) (void)hipEventDestroy(c->ev_call0);
    if (c->ev_call1) (void)hipEventDestroy(c->ev_call1);
    for (auto& e : c->pnet_ev) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete c;
    return TRL_OK;
}

}  // extern "C"

// ---- red zones (trl_debug_redzone) ---------------------------------------------------------------------
// One workgroup column per gap: res[3 g] += bytes of gap g that differ from `byte`, res[3 g + 1] / [3 g + 2] = min / max of their
// offsets within the gap.  gaps[2 g] / [2 g + 1] = the gap's offset in the workspace and its length.  Reads only, all inside the gap.
__global__ void k_rz_scan(const unsigned char* __restrict__ base, const unsigned long long* __restrict__ gaps, unsigned long long* __restrict__ res,
                          int g0, unsigned byte) {
    const int g = g0 + blockIdx.y;
    const unsigned long long len = gaps[2 * g + 1];
    const unsigned char* p = base + gaps[2 * g];
    unsigned long long head = (16 - ((uintptr_t)p & 15)) & 15;            // bytes in front of the first aligned 16
    if (head > len) head = len;
    const unsigned long long nw = (len - head) / 16, tail0 = head + nw * 16;
    const unsigned long long w = 0x0101010101010101ull * (byte & 0xFF);
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, nt = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long cnt = 0, first = ~0ull, last = 0;
    auto look = [&](unsigned long long i) {
        if (p[i] == (unsigned char)byte) return;
        cnt++;
        if (i < first) first = i;
        if (i > last) last = i;
    };
    if (tid == 0) {
        for (unsigned long long i = 0; i < head; i++) look(i);
        for (unsigned long long i = tail0; i < len; i++) look(i);
    }
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + head);
    for (unsigned long long k = tid; k < nw; k += nt) {
        const ulonglong2 v = q[k];
        if (v.x == w && v.y == w) continue;
        for (int b = 0; b < 16; b++) look(head + k * 16 + b);
    }
    if (cnt) {
        atomicAdd(&res[3 * g], cnt);
        atomicMin(&res[3 * g + 1], first);
        atomicMax(&res[3 * g + 2], last);
    }
}

namespace {
struct RzGap { size_t off, len; int block; size_t block_bytes; };
// every stretch of `a` that belongs to no block: behind each live block up to the next one (the last: up to a.off), then the tail
void rz_gaps(const Arena& a, std::vector<RzGap>& out) {
    const size_t nb = a.blocks.size();
    for (size_t i = 0; i < nb; i++) {
        const size_t end = a.blocks[i].off + a.blocks[i].bytes, next = i + 1 < nb ? a.blocks[i + 1].off : a.off;
        if (next > end) out.push_back({end, next - end, (int)i, a.blocks[i].bytes});
    }
    if (a.cap > a.off) out.push_back({a.off, a.cap - a.off, (int)nb, 0});
}
// The sweep of one workspace.  refill_from >= 0 (a rewind to that offset): everything from there to the capacity is refilled
int rz_sweep(trl_ctx* c, Arena& a, const char* site, long long refill_from) {
    trl_ctx::RedZone& z = c->rz;
    TRL_HIP(hipDeviceSynchronize());             // the call's stream, and every other one
    if (!a.base) return TRL_OK;
    std::vector<RzGap> gaps;
    rz_gaps(a, gaps);
    const size_t ng = gaps.size();
    if (ng) {
        if (z.dev_gaps < ng) {
            if (z.dev) TRL_HIP(hipFree(z.dev));
            z.dev = nullptr; z.dev_gaps = 0;
            TRL_HIP(hipMalloc((void**)&z.dev, (ng + 256) * 5 * 8));
            z.dev_gaps = ng + 256;
        }
        std::vector<unsigned long long> tab(5 * ng, 0);
        for (size_t g = 0; g < ng; g++) { tab[2 * g] = gaps[g].off; tab[2 * g + 1] = gaps[g].len; tab[2 * ng + 3 * g + 1] = ~0ull; }
        TRL_HIP(hipMemcpy(z.dev, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
        // the gaps behind blocks are a guard long: a few workgroups each, 32 K gaps per launch; the tail (last) is the long one
        const bool has_tail = gaps.back().block == (int)a.blocks.size();
        const size_t nshort = has_tail ? ng - 1 : ng;
        for (size_t g0 = 0; g0 < nshort; g0 += 32768) {
            const unsigned ny = (unsigned)std::min<size_t>(32768, nshort - g0);
            k_rz_scan<<<dim3(4, ny), 256>>>((const unsigned char*)a.base, z.dev, z.dev + 2 * ng, (int)g0, (unsigned)z.byte);
            TRL_LAUNCH_CHECK();
        }
        if (has_tail) {
            k_rz_scan<<<dim3(4096, 1), 256>>>((const unsigned char*)a.base, z.dev, z.dev + 2 * ng, (int)(ng - 1), (unsigned)z.byte);
            TRL_LAUNCH_CHECK();
        }
        TRL_HIP(hipMemcpy(tab.data() + 2 * ng, z.dev + 2 * ng, 3 * ng * 8, hipMemcpyDeviceToHost));
        for (size_t g = 0; g < ng; g++) {
            z.bytes += (long long)gaps[g].len;
            const unsigned long long* r = &tab[2 * ng + 3 * g];
            if (!r[0]) continue;
            z.nhits++;
            if (z.hits.size() < TRL_RZ_MAX_HITS) {
                trl_rz_hit h;
                memset(&h, 0, sizeof h);
                h.arena = &a == &c->arena ? 0 : 1; h.block = gaps[g].block;
                strncpy(h.site, site, sizeof(h.site) - 1);
                h.block_bytes = (long long)gaps[g].block_bytes; h.gap_off = (long long)gaps[g].off; h.gap_bytes = (long long)gaps[g].len;
                h.first = (long long)r[1]; h.last = (long long)r[2]; h.count = (long long)r[0];
                z.hits.push_back(h);
            }
            TRL_HIP(hipMemset(a.base + gaps[g].off, z.byte, gaps[g].len));   // repaired: reported once
        }
    }
    z.sweeps++;
    if (refill_from >= 0 && (size_t)refill_from < a.cap) TRL_HIP(hipMemset(a.base + refill_from, z.byte, a.cap - (size_t)refill_from));
    TRL_HIP(hipDeviceSynchronize());
    return TRL_OK;
}
// Arena::on_rewind of the two workspaces while the guard is on (a failing HIP call here fails the next one of the entry point too)
void rz_on_rewind(Arena& a, size_t mark, const char* site, void* owner) { (void)rz_sweep((trl_ctx*)owner, a, site, (long long)mark); }
}  // namespace

int trl_rz_sweep_all(trl_ctx* c, const char* site) {
    TRL_CHECK(rz_sweep(c, c->arena, site, -1));
    return rz_sweep(c, c->scratch, site, -1);
}

int trl_ensure(trl_ctx* c, Arena& a, size_t bytes) {
    if (bytes <= a.cap) return TRL_OK;
    // Growing frees the old block, so it is only called while nothing allocated from `a` is live:
    // at the start of a call (arena) or between cascade stages (scratch).
    const size_t ncap = bytes + (bytes >> 3) + (32u << 20);
    TRL_HIP(hipDeviceSynchronize());
    if (a.guard && a.base) TRL_CHECK(rz_sweep(c, a, "ensure", -1));
    if (a.base) { TRL_HIP(hipFree(a.base)); a.base = nullptr; a.cap = 0; }
    TRL_HIP(hipMalloc((void**)&a.base, ncap));
    a.cap = ncap;
    a.off = 0;
    a.blocks.clear();
    if (c->dbg_poison >= 0) TRL_HIP(hipMemset(a.base, c->dbg_poison, ncap));   // test hook: workspaces that grow stay poisoned
    return TRL_OK;
}

// ---- hot path ---------------------------------------------------------------------------------------
int trl_check_idle(trl_ctx* c) {
    if (!c) { trl_set_error("null context"); return TRL_ERR_INVALID; }
    if (c->pend.active) { trl_set_error("the context has a call in flight: trl_detect_embed_end() first"); return TRL_ERR_STATE; }
    return TRL_OK;
}

static int check_call(trl_ctx* c, const void* frames, int n, int H, int W) {
    TRL_CHECK(trl_check_idle(c));
    if (!c->have_weights) { trl_set_error("trl_load_weights has not been called"); return TRL_ERR_STATE; }
    if (!frames || n <= 0 || n > 65535 || H < 12 || W < 12 || H > 16383 || W > 16383) {   // n: grid.y carries the frame index in several kernels
        trl_set_error("bad frame batch n=%d H=%d W=%d (1..65535 frames of 12..16383 px per side)", n, H, W);
        return TRL_ERR_INVALID;
    }
    // the pyramid and front kernels turn the frame pointer into dword and 16-byte loads (include/truely_hip.h)
    if (((uintptr_t)frames & 3) != 0) { trl_set_error("frame buffer must be 4-byte aligned"); return TRL_ERR_INVALID; }
    return TRL_OK;
}

static void collect_timings(trl_ctx* c) {
    float call_ms = 0.f, pnet_ms = 0.f, pyr_ms = 0.f;
    (void)hipEventElapsedTime(&call_ms, c->ev_call0, c->ev_call1);
    int launches = 0;
    if (c->cfg.pnet_mode == 0 && c->pnet_ev_used >= 2) {
        // pair 0 = pyramid kernel, pair 1 = the fused PNet kernel (the dominant kernel, one launch) with its confirm pass
        (void)hipEventElapsedTime(&pyr_ms, c->pnet_ev[0].first, c->pnet_ev[0].second);
        (void)hipEventElapsedTime(&pnet_ms, c->pnet_ev[1].first, c->pnet_ev[1].second);
        launches = 1;
    } else {
        for (int i = 0; i < c->pnet_ev_used; i++) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, c->pnet_ev[i].first, c->pnet_ev[i].second) == hipSuccess) pnet_ms += t;
        }
        launches = c->pnet_ev_used;
    }
    c->last_ms[0] = pnet_ms; c->last_ms[1] = call_ms; c->last_ms[2] = (float)launches; c->last_ms[3] = pyr_ms;
    c->pnet_kernel_ms = 0.f;
    if (c->cfg.pnet_mode == 0 && c->pnet_clk && c->pnet_prof) {   // diagnostic mode only: a blocking copy per call (the last launch's span)
        unsigned long long t = 0;
        int khz = 0;
        if (hipMemcpy(&t, c->pnet_clk + 38, sizeof t, hipMemcpyDeviceToHost) == hipSuccess &&
            hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device) == hipSuccess && khz > 0)
            c->pnet_kernel_ms = (float)((double)t / (double)khz);
    }
}

// The crops of call q (model.py:55-58 per frame, by embed_mode) into the caller's faces_out, or into a block of X in front of the
// embedder's walk, which then runs over them
static int crop_embed(trl_ctx* c, Arena& X, const trl_ctx::Pending& q, hipStream_t s) {
    const int n = q.n, H = q.H, W = q.W, S = c->cfg.embed_mode == 0 ? 80 : 160;
    float* faces = q.faces_out;
    if (!faces) {
        X.reset("crop_embed");                       // stream order: the cascade's kernels are done with it before these run
        faces = (float*)X.alloc((size_t)n * S * S * 3 * 4);
        if (!faces) { trl_set_error("arena exhausted"); return TRL_ERR_STATE; }
    }
    if (!X.counting) {
        if (c->cfg.embed_mode == 0) TRL_CHECK(trl_launch_crop_resize80(q.frames, n, H, W, q.rect, q.valid, faces, s));
        else if (c->cfg.embed_mode == 3) TRL_CHECK(trl_launch_crop_aligned(q.frames, n, H, W, c->cb.pts0, q.valid, S, true, faces, s));
        else TRL_CHECK(trl_launch_crop_area_std(q.frames, n, H, W, q.rect, q.valid, S, c->cfg.embed_mode == 2, faces, s));
    }
    return q.faces_out ? TRL_OK : trl_run_facenet(c, X, faces, n, S, S, q.valid, q.emb, s);
}
// c->fn_need_bytes = the count of an embedder call on n faces of h x w -- with `crops`, of crop_embed for an EMBED call of n
// frames.  It stays for the next call with the same key: equal batches pay one comparison, not a second walk
static int embed_need(trl_ctx* c, bool crops, int n, int h, int w) {
    const int key[6] = {n, h, w, c->cfg.embed_precision, g_trl_no_fnconv, crops};
    if (memcmp(key, c->fn_need_key, sizeof key) == 0) return TRL_OK;
    Arena count = Arena::counter(c->scratch.guard);
    trl_ctx::Pending q; q.n = n;
    TRL_CHECK(crops ? crop_embed(c, count, q, nullptr) : trl_run_facenet(c, count, nullptr, n, h, w, nullptr, nullptr, nullptr));
    memcpy(c->fn_need_key, key, sizeof key);
    c->fn_need_bytes = count.high;
    return TRL_OK;
}
// Every cascade entry point (trl_mtcnn_detect*, trl_detect_embed*, trl_detect_crop*) is one call in c->pend: call_begin()
// validates it and queues its first attempt, call_wait() is the call's one host synchronisation, the capacity check and --
// rarely -- the re-run; the blocking entry points do both.  call_enqueue() queues one attempt on the call's stream: the cascade
// (from the stage the last check chose), then the outputs of the call's kind.
static int call_enqueue(trl_ctx* c) {
    const trl_ctx::Pending& q = c->pend;
    hipStream_t s = (hipStream_t)q.stream;
    const int n = q.n, H = q.H, W = q.W;
    if (!q.attempt) TRL_HIP(hipEventRecord(c->ev_call0, s));   // trl_debug_timings: out[1] covers every attempt of the call
    TRL_CHECK(trl_cascade_detect(c, q.frames, n, H, W, s, q.attempt ? c->caps.resume_stage : 0));
    if (q.kind == trl_ctx::Pending::DETECT) {
        // model.py's per-frame outputs are not asked for: they go to the blocks behind the lists
        TRL_HIP(hipMemsetAsync(q.boxes, 0, (size_t)n * c->cfg.max_faces * 16, s));
        TRL_HIP(hipMemsetAsync(q.probs, 0, (size_t)n * c->cfg.max_faces * 4, s));
        if (q.points) TRL_HIP(hipMemsetAsync(q.points, 0, (size_t)n * c->cfg.max_faces * 40, s));
        TRL_CHECK(trl_cascade_finish(c, q.frames, n, H, W, q.boxes, q.probs, q.points, q.counts, c->cb.box0, c->cb.prob0, c->cb.rect, c->cb.valid, nullptr, s, q.order));
    } else {
        // model.py:47-58 (detect, largest box, crop + resize) and, EMBED, :59 (embed).  CROP: the crops go to the caller's faces_out
        // and the embedder does not run; EMBED: they live in scratch and are embedded.  (pts0: the landmarks that steer embed_mode 3's crop)
        TRL_CHECK(trl_cascade_finish(c, q.frames, n, H, W, nullptr, nullptr, nullptr, nullptr, q.box, q.prob, q.rect, q.valid,
                                     c->cfg.embed_mode == 3 ? c->cb.pts0 : nullptr, s));
        TRL_CHECK(crop_embed(c, c->scratch, q, s));
    }
    TRL_HIP(hipEventRecord(c->ev_call1, s));
    TRL_CHECK(trl_gate_record(c, s));
    return TRL_OK;
}

// q: the call the entry point describes (trl_ctx::Pending: kind, frames, stream, outputs)
static int call_begin(trl_ctx* c, const trl_ctx::Pending& q) {
    TRL_CHECK(check_call(c, q.frames, q.n, q.H, q.W));
    if (q.kind == trl_ctx::Pending::DETECT ? !(q.boxes && q.probs && q.counts) : !(q.box && q.prob && q.rect && q.valid && (q.emb || q.faces_out))) {
        trl_set_error("null output");
        return TRL_ERR_INVALID;
    }
    TRL_HIP(hipSetDevice(c->cfg.device));
    const int S = c->cfg.embed_mode == 0 ? 80 : 160;
    if (q.kind == trl_ctx::Pending::EMBED) TRL_CHECK(embed_need(c, true, q.n, S, S));
    c->scratch_after_cascade = q.kind == trl_ctx::Pending::EMBED ? c->fn_need_bytes : 0;
    c->pend = q;
    c->pend.active = true;
    c->pend.attempt = 0;
    const int st = call_enqueue(c);
    if (st != TRL_OK) c->pend.active = false;
    return st;
}

// Every attempt that overflows a capacity raises that capacity to the need the attempt measured (trl_caps_check), and a stage's
// need is measured once the stages in front of it ran on complete lists.  There are five capacities -- level lists, frame lists,
// spill workspace, R-Net batch, O-Net batch -- but a call can take more than six attempts: the spill pool can overflow twice (for
// the level lists, and again for the frame lists that exist only once the level lists are complete), and a per-frame total
// measured while the pool dropped lists is a lower bound.  The model device of tests/test_capacity_cpu.py (500 need sets, from
// empty to every cell of a 16383 px frame a candidate) needed at most 7: level lists, spill pool + frame lists, frame lists,
// spill pool, R-Net batch, O-Net batch, the attempt that fits.  The bound below is never reached by any input (detect_face()
// has no candidate limit, and neither has this call), it only turns a bug into an error.
enum { TRL_MAX_ATTEMPTS = 12 };

static int call_wait(trl_ctx* c, const char* site) {
    if (!c) { trl_set_error("null context"); return TRL_ERR_INVALID; }
    if (!c->pend.active) { trl_set_error("no call in flight on this context"); return TRL_ERR_STATE; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    hipStream_t s = (hipStream_t)c->pend.stream;
    int st = TRL_OK;
    for (;;) {
        if ((st = (hipStreamSynchronize(s) == hipSuccess ? TRL_OK : TRL_ERR_HIP)) != TRL_OK) { trl_set_error("hipStreamSynchronize: %s", hipGetErrorString(hipGetLastError())); break; }
        int retry = 0;
        if ((st = trl_cascade_check(c, c->pend.n, &retry)) != TRL_OK) break;
        c->caps.last_attempts = ++c->pend.attempt;
        if (!retry) break;
        if (c->pend.attempt >= TRL_MAX_ATTEMPTS) { trl_set_error("candidate capacities did not converge"); st = TRL_ERR_STATE; break; }
        if ((st = call_enqueue(c)) != TRL_OK) break;
    }
    c->pend.active = false;
    if (st == TRL_OK) collect_timings(c);
    if (st == TRL_OK) st = trl_rz_end(c, site);
    return st;
}

static int call_run(trl_ctx* c, const trl_ctx::Pending& q, const char* site) {
    TRL_CHECK(call_begin(c, q));
    return call_wait(c, site);
}

static trl_ctx::Pending detect_call(const uint8_t* d_frames, int n, int H, int W, float* d_boxes, float* d_probs, float* d_points,
                                    int32_t* d_counts, void* stream, int order) {
    trl_ctx::Pending q;
    q.kind = trl_ctx::Pending::DETECT;
    q.frames = d_frames; q.n = n; q.H = H; q.W = W; q.stream = stream;
    q.boxes = d_boxes; q.probs = d_probs; q.points = d_points; q.counts = d_counts; q.order = order;
    return q;
}

static trl_ctx::Pending embed_call(const uint8_t* d_frames, int n, int H, int W, float* d_box, float* d_prob, int32_t* d_rect,
                                   uint8_t* d_valid, float* d_emb, float* d_faces_out, void* stream) {
    trl_ctx::Pending q;
    q.kind = d_emb ? trl_ctx::Pending::EMBED : trl_ctx::Pending::CROP;
    q.frames = d_frames; q.n = n; q.H = H; q.W = W; q.stream = stream;
    q.box = d_box; q.prob = d_prob; q.rect = d_rect; q.valid = d_valid; q.emb = d_emb; q.faces_out = d_faces_out;
    return q;
}

extern "C" {

int trl_mtcnn_detect(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_boxes, float* d_probs, int32_t* d_counts,
                     void* stream) {
    return call_run(c, detect_call(d_frames, n, H, W, d_boxes, d_probs, nullptr, d_counts, stream, 0), "mtcnn_detect");
}

int trl_mtcnn_detect_landmarks(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_boxes, float* d_probs,
                               float* d_points, int32_t* d_counts, void* stream) {
    if (!d_points) { trl_set_error("null output"); return TRL_ERR_INVALID; }
    return trl_mtcnn_detect_ordered(c, d_frames, n, H, W, 0, d_boxes, d_probs, d_points, d_counts, stream);
}

int trl_mtcnn_detect_ordered(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, int order, float* d_boxes, float* d_probs,
                             float* d_points, int32_t* d_counts, void* stream) {
    if (order != 0 && order != 1) { trl_set_error("bad box order %d (0 = area, 1 = detection order)", order); return TRL_ERR_INVALID; }
    return call_run(c, detect_call(d_frames, n, H, W, d_boxes, d_probs, d_points, d_counts, stream, order), "mtcnn_detect");
}

int trl_detect_embed(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_box, float* d_prob, int32_t* d_rect,
                     uint8_t* d_valid, float* d_emb, void* stream) {
    if (!d_emb) { trl_set_error("null output"); return TRL_ERR_INVALID; }
    return call_run(c, embed_call(d_frames, n, H, W, d_box, d_prob, d_rect, d_valid, d_emb, nullptr, stream), "detect_embed");
}

int trl_detect_crop(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_box, float* d_prob, int32_t* d_rect,
                    uint8_t* d_valid, float* d_faces, void* stream) {
    if (!d_faces) { trl_set_error("null output"); return TRL_ERR_INVALID; }
    return call_run(c, embed_call(d_frames, n, H, W, d_box, d_prob, d_rect, d_valid, nullptr, d_faces, stream), "detect_crop");
}

int trl_detect_embed_begin(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_box, float* d_prob, int32_t* d_rect,
                           uint8_t* d_valid, float* d_emb, void* stream) {
    if (!d_emb) { trl_set_error("null output"); return TRL_ERR_INVALID; }
    return call_begin(c, embed_call(d_frames, n, H, W, d_box, d_prob, d_rect, d_valid, d_emb, nullptr, stream));
}

int trl_detect_crop_begin(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_box, float* d_prob, int32_t* d_rect,
                          uint8_t* d_valid, float* d_faces, void* stream) {
    if (!d_faces) { trl_set_error("null output"); return TRL_ERR_INVALID; }
    return call_begin(c, embed_call(d_frames, n, H, W, d_box, d_prob, d_rect, d_valid, nullptr, d_faces, stream));
}

int trl_detect_embed_end(trl_ctx* c) { return call_wait(c, "embed_end"); }

}  // extern "C"

// trl_facenet_embed / _masked / trl_facenet_features: d_valid nullable (zero rows where it is 0)
static int facenet_embed(trl_ctx* c, const float* d_faces, const uint8_t* d_valid, bool masked, int n, int h, int w, float* d_emb,
                         void* stream, bool features = false) {
    if (!c || !c->have_weights) { trl_set_error("context without weights"); return TRL_ERR_STATE; }
    TRL_CHECK(trl_check_idle(c));
    if (!d_faces || (masked && !d_valid) || !d_emb || n <= 0 || h < 75 || w < 75) { trl_set_error("bad face batch n=%d %dx%d (min 75x75)", n, h, w); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_CHECK(embed_need(c, false, n, h, w));
    TRL_CHECK(trl_scratch_begin(c, c->fn_need_bytes));
    TRL_CHECK(trl_run_facenet(c, c->scratch, d_faces, n, h, w, d_valid, d_emb, (hipStream_t)stream, features));
    TRL_CHECK(trl_gate_record(c, (hipStream_t)stream));
    return trl_rz_end(c, "facenet");
}

// trl_drift_score / trl_drift_update: d_state nullable (no state carried across calls)
static int drift(trl_ctx* c, void* d_state, const float* d_emb, const uint8_t* d_valid, int n, long long frame_count, int fps, float* d_sims,
                 uint8_t* d_flags, int32_t* d_result, void* stream) {
    TRL_HIP(hipSetDevice(c->cfg.device));
    float* sims = d_sims;
    if (!sims) {   // the scan needs the similarities even when the caller does not want them
        TRL_CHECK(trl_ensure(c, c->sims_tmp, (size_t)(n > 0 ? n : 1) * sizeof(float)));
        sims = (float*)c->sims_tmp.base;
    }
    return trl_launch_drift(d_emb, d_valid, n, frame_count, fps, sims, d_flags, d_result, (hipStream_t)stream, d_state);
}

extern "C" {

int trl_facenet_embed(trl_ctx* c, const float* d_faces, int n, int h, int w, float* d_emb, void* stream) {
    return facenet_embed(c, d_faces, nullptr, false, n, h, w, d_emb, stream);
}

int trl_facenet_embed_masked(trl_ctx* c, const float* d_faces, const uint8_t* d_valid, int n, int h, int w, float* d_emb, void* stream) {
    return facenet_embed(c, d_faces, d_valid, true, n, h, w, d_emb, stream);
}

int trl_facenet_features(trl_ctx* c, const float* d_faces, const uint8_t* d_valid, int n, int h, int w, float* d_feat, void* stream) {
    return facenet_embed(c, d_faces, d_valid, false, n, h, w, d_feat, stream, true);
}

int trl_facenet_num_classes(trl_ctx* c, int* C) {
    if (!c || !C) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    if (!c->have_weights) { trl_set_error("context without weights"); return TRL_ERR_STATE; }
    *C = c->num_classes;
    return TRL_OK;
}

int trl_facenet_logits(trl_ctx* c, const float* d_feat, int n, float* d_logits, long long ld, void* stream) {
    if (!c || !c->have_weights) { trl_set_error("context without weights"); return TRL_ERR_STATE; }
    TRL_CHECK(trl_check_idle(c));
    if (!c->logits_w) { trl_set_error("the loaded checkpoint has no logits layer"); return TRL_ERR_WEIGHTS; }
    if (!d_feat || !d_logits || n < 1 || ld < c->num_classes) {
        trl_set_error("bad logits call n=%d ld=%lld (%d classes)", n, ld, c->num_classes);
        return TRL_ERR_INVALID;
    }
    TRL_HIP(hipSetDevice(c->cfg.device));
    return trl_launch_logits(d_feat, n, c->logits_w->p, c->logits_w->ld, c->logits_b, c->num_classes, d_logits, ld, (hipStream_t)stream);
}

int trl_drift_score(trl_ctx* c, const float* d_emb, const uint8_t* d_valid, int n, long long frame_count, int fps, float* d_sims,
                    uint8_t* d_flags, int32_t* d_result, void* stream) {
    if (!c || !d_emb || !d_valid || !d_result || n < 0) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    return drift(c, nullptr, d_emb, d_valid, n, frame_count, fps, d_sims, d_flags, d_result, stream);
}

// trl_drift_score continued across the windows of ONE clip: d_state carries `previous embedding / run / hits` (model.py:60-75)
int trl_drift_update(trl_ctx* c, void* d_state, const float* d_emb, const uint8_t* d_valid, int n, long long frame_count, int fps,
                     float* d_sims, uint8_t* d_flags, int32_t* d_result, void* stream) {
    if (!c || !d_state || !d_result || n < 0 || (n > 0 && (!d_emb || !d_valid)) || ((uintptr_t)d_state & 3)) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    return drift(c, d_state, d_emb, d_valid, n, frame_count, fps, d_sims, d_flags, d_result, stream);
}

// ---- inspection hooks ----------------------------------------------------------------------------------
int trl_debug_stage_boxes(trl_ctx* c, int stage, int frame, float* h_boxes, int max_rows, int* n_out) {
    TRL_CHECK(trl_check_idle(c));
    if (!c->cb.cnt[0] || frame < 0 || frame >= c->cb.n || stage < 1 || stage > 3 || !n_out || (max_rows > 0 && !h_boxes)) {
        trl_set_error("no cascade state");
        return TRL_ERR_STATE;
    }
    const int32_t* cnt = c->cb.cnt[stage - 1];
    const float* src = c->cb.box[stage - 1];
    int32_t k = 0;
    TRL_HIP(hipDeviceSynchronize());
    TRL_HIP(hipMemcpy(&k, cnt + frame, 4, hipMemcpyDeviceToHost));
    *n_out = k;
    const int m = k < max_rows ? k : max_rows;
    if (m > 0) TRL_HIP(hipMemcpy(h_boxes, src + (size_t)frame * c->cb.capF * 5, (size_t)m * 20, hipMemcpyDeviceToHost));
    return TRL_OK;
}

__global__ void k_poison_lds(unsigned word, int nwords) {
    extern __shared__ unsigned lds_words[];
    for (int i = threadIdx.x; i < nwords; i += blockDim.x) lds_words[i] = word;
    __syncthreads();
    if (lds_words[(threadIdx.x * 97) % nwords] != word) __builtin_trap();   // keeps the stores alive
}

// Fills every byte of the activation workspaces with `byte` (0xFF = NaN patterns, 0x7F = huge finite floats): a
// result that depends on workspace contents left by an earlier call or process shows up as a parity failure.
int trl_debug_poison(trl_ctx* c, int byte) {
    TRL_CHECK(trl_check_idle(c));
    if (c->rz.guard) { trl_set_error("red zones are on: their fill byte is the poison"); return TRL_ERR_STATE; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_HIP(hipDeviceSynchronize());
    c->dbg_poison = byte & 0xFF;                 // sticky: blocks allocated later are filled too
    if (c->scratch.base) TRL_HIP(hipMemset(c->scratch.base, byte, c->scratch.cap));
    if (c->arena.base) TRL_HIP(hipMemset(c->arena.base, byte, c->arena.cap));
    // ... and the LDS of every CU (it keeps the previous kernel's contents): 1024 workgroups of 160 KB, one per CU at a time
    const int lds_bytes = 160 * 1024;
    TRL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_poison_lds), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    const unsigned w = (unsigned)(byte & 0xFF) * 0x01010101u;
    k_poison_lds<<<1024, 256, lds_bytes, 0>>>(w, lds_bytes / 4);
    TRL_LAUNCH_CHECK();   // cascade lists: every call re-initialises what it reads
    TRL_HIP(hipDeviceSynchronize());
    return TRL_OK;
}

int trl_debug_level_counts(trl_ctx* c, int frame, int32_t* h_cand, int32_t* h_keep, int* n_levels) {
    TRL_CHECK(trl_check_idle(c));
    if (!c->cb.lvl_cnt || frame < 0 || frame >= c->cb.n || !h_cand || !h_keep || !n_levels) { trl_set_error("no cascade state"); return TRL_ERR_STATE; }
    TRL_HIP(hipDeviceSynchronize());
    const int L = c->cb.L;
    TRL_HIP(hipMemcpy(h_cand, c->cb.lvl_cnt + (size_t)frame * L, (size_t)L * 4, hipMemcpyDeviceToHost));
    TRL_HIP(hipMemcpy(h_keep, c->cb.lvl_keep_cnt + (size_t)frame * L, (size_t)L * 4, hipMemcpyDeviceToHost));
    *n_levels = L;
    return TRL_OK;
}

// Candidate records (generateBoundingBox rows) one (frame, level) of the last call produced, in append order
int trl_debug_level_cands(trl_ctx* c, int frame, int level, void* h_rows, int max_rows, int* n_out) {
    TRL_CHECK(trl_check_idle(c));
    if (!c->cb.lvl_cnt || frame < 0 || frame >= c->cb.n || level < 0 || level >= c->cb.L || !n_out || (max_rows > 0 && !h_rows)) {
        trl_set_error("no cascade state");
        return TRL_ERR_STATE;
    }
    static_assert(sizeof(Cand) == 40, "trl_debug_level_cands row layout");
    TRL_HIP(hipDeviceSynchronize());
    int32_t k = 0;
    TRL_HIP(hipMemcpy(&k, c->cb.lvl_cnt + (size_t)frame * c->cb.L + level, 4, hipMemcpyDeviceToHost));
    if (k > c->cb.lay.capl[level]) k = c->cb.lay.capl[level];
    *n_out = k;
    const int m = k < max_rows ? k : max_rows;
    if (m > 0) TRL_HIP(hipMemcpy(h_rows, c->cb.lvl_rec + (size_t)frame * c->cb.lay.S + c->cb.lay.rec0[level], (size_t)m * sizeof(Cand), hipMemcpyDeviceToHost));
    return TRL_OK;
}

// The per-level NMS picks of one (frame, level) of the last call: indices into that level's candidate records (the rows
// trl_debug_level_cands returns, in the same append order), in pick order (descending score)
int trl_debug_level_keep(trl_ctx* c, int frame, int level, int32_t* h_idx, int max_rows, int* n_out) {
    TRL_CHECK(trl_check_idle(c));
    if (!c->cb.lvl_keep_cnt || frame < 0 || frame >= c->cb.n || level < 0 || level >= c->cb.L || !n_out || (max_rows > 0 && !h_idx)) {
        trl_set_error("no cascade state");
        return TRL_ERR_STATE;
    }
    TRL_HIP(hipDeviceSynchronize());
    int32_t k = 0;
    TRL_HIP(hipMemcpy(&k, c->cb.lvl_keep_cnt + (size_t)frame * c->cb.L + level, 4, hipMemcpyDeviceToHost));
    *n_out = k;
    const int m = k < max_rows ? k : max_rows;
    if (m > 0) TRL_HIP(hipMemcpy(h_idx, c->cb.lvl_keep_idx + (size_t)frame * c->cb.lay.S + c->cb.lay.rec0[level], (size_t)m * 4, hipMemcpyDeviceToHost));
    return TRL_OK;
}

int trl_debug_pyramid_level(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_out, int* h, int* w, void* stream) {
    TRL_CHECK(check_call(c, d_frame, 1, H, W));
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_scratch_begin(c, trl_pnet_fused_bytes(c, 1, H, W) + (1u << 20)));
    TRL_CHECK(trl_pyramid_export(c, d_frame, H, W, level, d_out, h, w, s));
    TRL_HIP(hipStreamSynchronize(s));
    return trl_rz_end(c, "pyramid_level");
}

int trl_debug_pyramid_batch(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_out, long long* pyr_stride,
                            int32_t* h_levels, int max_levels, int* n_levels, void* stream) {
    TRL_CHECK(check_call(c, d_frames, n, H, W));
    if (!pyr_stride || !n_levels || (max_levels > 0 && !h_levels)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    if (d_out) TRL_CHECK(trl_scratch_begin(c, trl_pnet_fused_bytes(c, n, H, W) + (1u << 20)));
    TRL_CHECK(trl_pyramid_export_batch(c, d_frames, n, H, W, d_out, pyr_stride, h_levels, max_levels, n_levels, s));
    TRL_HIP(hipStreamSynchronize(s));
    return trl_rz_end(c, "pyramid_batch");
}

int trl_debug_pyramid_plan(trl_ctx* c, int32_t* h_rows, int max_levels, int* n_levels) {
    TRL_CHECK(trl_check_idle(c));
    if (!n_levels || (max_levels > 0 && !h_rows)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *n_levels = c->pyr_plan.L;
    for (int l = 0; l < c->pyr_plan.L && l < max_levels; l++)
        for (int k = 0; k < TRL_PYR_PLAN_COLS; k++) h_rows[l * TRL_PYR_PLAN_COLS + k] = c->pyr_plan.row[l][k];
    return TRL_OK;
}

int trl_debug_facenet_plan(trl_ctx* c, trl_fn_plan_row* h_rows, int max_rows, int* n_rows) {
    TRL_CHECK(trl_check_idle(c));
    if (!n_rows || (max_rows > 0 && !h_rows)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *n_rows = (int)c->fn_plan.size();
    for (int i = 0; i < *n_rows && i < max_rows; i++) h_rows[i] = c->fn_plan[i];
    return TRL_OK;
}

int trl_debug_facenet_capture(trl_ctx* c, int conv_index) {
    TRL_CHECK(trl_check_idle(c));
    c->fn_cap_arm = conv_index < 0 ? -1 : conv_index;
    return TRL_OK;
}

int trl_debug_facenet_capture_read(trl_ctx* c, int view, void* h_dst, size_t max_bytes, int32_t* dims5) {
    TRL_CHECK(trl_check_idle(c));
    if (view < 0 || view > 2 || !dims5) { trl_set_error("bad capture view %d", view); return TRL_ERR_INVALID; }
    const auto& b = c->fn_cap[view];
    for (int k = 0; k < 5; k++) dims5[k] = b.dims[k];
    if (!h_dst || b.dims[3] == 0) return TRL_OK;
    const size_t bytes = (size_t)b.dims[0] * b.dims[1] * b.dims[2] * b.dims[3] * b.dims[4];
    if (bytes > max_bytes) { trl_set_error("capture needs %zu bytes", bytes); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_HIP(hipDeviceSynchronize());
    TRL_HIP(hipMemcpy(h_dst, b.p, bytes, hipMemcpyDeviceToHost));
    return TRL_OK;
}

int trl_debug_pnet_level(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_prob, float* d_reg, int* oh, int* ow,
                         void* stream) {
    TRL_CHECK(check_call(c, d_frame, 1, H, W));
    hipStream_t s = (hipStream_t)stream;
    const int L = trl_compute_levels(c, H, W);
    if (level < 0 || level >= L) { trl_set_error("level %d out of range (%d levels)", level, L); return TRL_ERR_INVALID; }
    const LevelGeom& g = c->lv[level];
    float* heads;
    TRL_CHECK(trl_carve_scratch(c, [&](Arena& X) { return trl_pnet_generic_level(c, X, d_frame, 1, H, W, g, &heads, s); }));
    TRL_CHECK(trl_launch_heads_to_maps(heads, g.oh * g.ow, d_prob, d_reg, s));
    *oh = g.oh; *ow = g.ow;
    TRL_HIP(hipStreamSynchronize(s));
    return trl_rz_end(c, "pnet_level_hook");
}

// test hooks: a whole net through the layer kernels over n crops [n][side][side][3]: d_out [n][6] (R-Net) / [n][16] (O-Net)
static int debug_net(trl_ctx* c, const NetDesc& d, const float* d_crops, int n, float* d_out, void* stream) {
    if (!c || !c->have_weights || !d_crops || !d_out || n <= 0) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    TRL_CHECK(trl_check_idle(c));
    TRL_CHECK(trl_carve_scratch(c, [&](Arena& X) { return trl_run_net(c, X, d, 0, Act::dense(d_crops, n, d.side, d.side, 3), d_out, (hipStream_t)stream); }));
    return trl_rz_end(c, "debug_net");
}
int trl_debug_rnet(trl_ctx* c, const float* d_crops, int n, float* d_out, void* stream) { return debug_net(c, trl_nets[TRL_RNET], d_crops, n, d_out, stream); }
int trl_debug_onet(trl_ctx* c, const float* d_crops, int n, float* d_out, void* stream) { return debug_net(c, trl_nets[TRL_ONET], d_crops, n, d_out, stream); }
// k_build_map's records on the device for a front launch outside the cascade: hb holds `slots` records of 8 words (the live ones
// first); c->cb then describes the batch and the record list, *total is the device-side count nb.
static int upload_records(trl_ctx* c, int nf, int H, int W, const std::vector<int32_t>& hb, int slots, int nb, int32_t** total, hipStream_t s) {
    Arena& A = c->arena;
    TRL_CHECK(trl_ensure(c, A, (size_t)slots * 32 + (1u << 20)));
    A.reset("records");
    CascadeBufs& B = c->cb;
    B = CascadeBufs();
    B.n = nf; B.H = H; B.W = W;
    // + 32: one record of slack for READS only.  No kernel stores into it: with the slack at 0 and red zones on
    // (trl_debug_redzone), the front kernel and the stage loop (capacity == count, > count, chunked) left every guard byte intact.
    B.cbox = (int32_t*)A.alloc((size_t)slots * 32 + 32);
    *total = (int32_t*)A.alloc(64);
    TRL_HIP(hipMemcpyAsync(B.cbox, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, s));
    TRL_HIP(hipMemcpyAsync(*total, &nb, 4, hipMemcpyHostToDevice, s));
    TRL_HIP(hipStreamSynchronize(s));                      // the host data may go out of scope
    return TRL_OK;
}
static const int32_t kRecordPoison = (int32_t)0xA5A5A5A5;  // frame / window words no live record has

// The production stage-2 / stage-3 loop (trl_stage_net, as the cascade runs it) over a launch capacity the caller chooses.  h_rows:
// nb host rows of `cols` floats -- (frame, x1, y1, x2, y2), or (x1, y1, x2, y2) of frame 0 when cols = 4 -- turned into
// k_build_map's records by pad() (detect_face.py: trunc, x = max(x1, 1), ex = min(x2, W), crop [y-1:ey, x-1:ex]); the device
// total is nb, and record slots past it (the kernels read them, then discard them) hold a poison pattern.  The workspace is sized
// like the cascade's: chunk = the rnet_chunk / onet_chunk option.  d_out: [capacity][6] (net = 24) or [capacity][16] (net = 48),
// device; only rows of live candidates are defined.  trl_debug_mtcnn_plan then lists the tail's conv launches of every chunk.
static int stage_net_on_rows(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const float* h_rows, int cols, int nb, int net,
                             int capacity, float* d_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TRL_HIP(hipSetDevice(c->cfg.device));
    const int slots = nb > capacity ? nb : capacity;
    std::vector<int32_t> hb((size_t)slots * 8, kRecordPoison);
    for (int i = 0; i < nb; i++) {
        const float* b = h_rows + (size_t)cols * i + cols - 4;
        const int f = cols == 5 ? (int)b[-1] : 0;
        if (f < 0 || f >= nf) { trl_set_error("record %d: frame %d of %d", i, f, nf); return TRL_ERR_INVALID; }
        const int bx = (int)truncf(b[0]), by = (int)truncf(b[1]), bex = (int)truncf(b[2]), bey = (int)truncf(b[3]);
        const int x = bx < 1 ? 1 : bx, y = by < 1 ? 1 : by, ex = bex > W ? W : bex, ey = bey > H ? H : bey;
        if (ey <= y - 1 || ex <= x - 1) { trl_set_error("record %d: empty crop window", i); return TRL_ERR_INVALID; }
        int32_t* r = &hb[8 * (size_t)i];
        r[0] = f; r[1] = y - 1; r[2] = x - 1; r[3] = ey - (y - 1); r[4] = ex - (x - 1); r[5] = r[6] = r[7] = 0;
    }
    int32_t* total = nullptr;
    TRL_CHECK(upload_records(c, nf, H, W, hb, slots, nb, &total, s));
    c->mt_plan.clear();
    c->mt_plan_arm = true;
    const int st = trl_carve_scratch(c, [&](Arena& X) { return trl_stage_net(c, X, net, d_frames, H, W, total, capacity, d_out, s); });
    c->mt_plan_arm = false;
    TRL_CHECK(st);
    TRL_HIP(hipStreamSynchronize(s));
    c->cb = CascadeBufs();                                 // no cascade state to inspect after this hook
    return trl_rz_end(c, "stage_net");
}

// test hook: the production stage-2 / stage-3 network path -- the fused front kernel (k_mtcnn_front: pad(), crop, area resample,
// conv1, PReLU, pool) followed by the layer tail -- on caller-chosen boxes of frame 0, so its crop paths (small boxes, big boxes,
// boxes clipped by the frame) are checked directly, not only through cascade records.  h_boxes: nb rows of x1,y1,x2,y2 (host),
// none with an empty crop window; d_out: [nb][6] (net = 24) or [nb][16] (net = 48), device.
int trl_debug_front_net(trl_ctx* c, const uint8_t* d_frame, int H, int W, const float* h_boxes, int nb, int net, float* d_out, void* stream) {
    TRL_CHECK(check_call(c, d_frame, 1, H, W));
    if (!h_boxes || !d_out || nb <= 0 || nb > (1 << 20) || (net != 24 && net != 48)) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    return stage_net_on_rows(c, d_frame, 1, H, W, h_boxes, 4, nb, net, nb, d_out, stream);
}

int trl_debug_stage_net(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const float* h_recs, int nb, int net, int capacity,
                        float* d_out, void* stream) {
    TRL_CHECK(check_call(c, d_frames, nf, H, W));
    if ((nb > 0 && !h_recs) || (capacity > 0 && !d_out) || nb < 0 || nb > (1 << 24) || capacity < 0 || capacity > (1 << 24) ||
        (net != 24 && net != 48)) {
        trl_set_error("bad argument");
        return TRL_ERR_INVALID;
    }
    return stage_net_on_rows(c, d_frames, nf, H, W, h_recs, 5, nb, net, capacity, d_out, stream);
}

// test hook: k_mtcnn_front alone.  h_win: nb host rows {frame, y0, x0, ih, iw}, k_build_map's record given directly (no pad()); the
// kernel checks nothing, so every row is checked here.  Record slots nb .. capacity-1 hold the poison of stage_net_on_rows, the
// device total is nb, and the launch is trl_stage_net's: one chunk at t0 = 0 over `capacity` slots, writing the pooled maps
// [capacity][11][11][28] (net = 24) / [capacity][23][23][32] (net = 48) straight into d_pool.  No tail runs.
int trl_debug_front(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const int32_t* h_win, int nb, int net, int capacity,
                    float* d_pool, void* stream) {
    TRL_CHECK(check_call(c, d_frames, nf, H, W));
    if ((nb > 0 && !h_win) || (capacity > 0 && !d_pool) || nb < 0 || nb > (1 << 20) || capacity < 0 || capacity > (1 << 20) ||
        (net != 24 && net != 48)) {
        trl_set_error("bad argument");
        return TRL_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    TRL_HIP(hipSetDevice(c->cfg.device));
    const int slots = nb > capacity ? nb : capacity;
    std::vector<int32_t> hb((size_t)slots * 8, kRecordPoison);
    for (int i = 0; i < nb; i++) {
        const int32_t* r = h_win + 5 * (size_t)i;
        const long long f = r[0], y0 = r[1], x0 = r[2], ih = r[3], iw = r[4];
        if (f < 0 || f >= nf || ih < 1 || iw < 1 || y0 < 0 || x0 < 0 || y0 + ih > H || x0 + iw > W) {
            trl_set_error("window %d: frame %lld of %d, rows %lld + %lld of %d, columns %lld + %lld of %d", i, f, nf, y0, ih, H, x0, iw, W);
            return TRL_ERR_INVALID;
        }
        int32_t* q = &hb[8 * (size_t)i];
        for (int k = 0; k < 5; k++) q[k] = r[k];
        q[5] = q[6] = q[7] = 0;
    }
    int32_t* total = nullptr;
    TRL_CHECK(upload_records(c, nf, H, W, hb, slots, nb, &total, s));
    TRL_CHECK(trl_launch_front(c, trl_net_of(net), d_frames, H, W, total, 0, capacity, d_pool, s));
    TRL_HIP(hipStreamSynchronize(s));
    c->cb = CascadeBufs();
    return trl_rz_end(c, "front");
}

// test hook: the cascade's list kernels on caller-built lists (trl_cascade_lists has the layout of every kind)
int trl_debug_lists(trl_ctx* c, int kind, int n, int H, int W, const int32_t* h_caps, int n_levels, const int32_t* h_counts,
                    const void* h_rows, const float* h_logits, float* h_pts, float* d_boxes, float* d_probs, float* d_points,
                    int32_t* d_counts, float* d_box0, float* d_prob0, int32_t* d_rect, uint8_t* d_valid, void* stream) {
    TRL_CHECK(trl_check_idle(c));
    if (kind < 1 || kind > 3 || n <= 0 || n > 65535 || H < 12 || W < 12 || H > 16383 || W > 16383 || !h_caps || !h_counts ||
        n_levels < (kind == 1 ? 1 : 0) || n_levels > 32 || (kind == 3 && !(d_boxes && d_probs && d_points && d_counts && d_box0 &&
        d_prob0 && d_rect && d_valid))) {
        trl_set_error("bad argument");
        return TRL_ERR_INVALID;
    }
    long long slots = 0, total = 0;
    for (int l = 0; l <= n_levels; l++) {
        const int cap = h_caps[l];
        if (cap < 4 || cap > (1 << 20) || (cap & 3)) { trl_set_error("capacity %d: multiples of 4 in [4, 2^20]", cap); return TRL_ERR_INVALID; }
        if (l < n_levels) slots += cap;
    }
    if ((long long)n * (slots + h_caps[n_levels]) > (1ll << 26)) { trl_set_error("lists too large"); return TRL_ERR_INVALID; }
    const int nc = kind == 1 ? n * n_levels : n;
    for (int i = 0; i < nc; i++) {
        const int cap = kind == 1 ? h_caps[i % n_levels] : h_caps[n_levels];
        if (h_counts[i] < 0 || h_counts[i] > cap) { trl_set_error("list %d: count %d, capacity %d", i, h_counts[i], cap); return TRL_ERR_INVALID; }
        total += h_counts[i];
    }
    if (total > 0 && (!h_rows || (kind > 1 && !h_logits))) { trl_set_error("null rows"); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    const int st = trl_cascade_lists(c, kind, n, H, W, h_caps, n_levels, h_counts, h_rows, h_logits, h_pts, d_boxes, d_probs, d_points, d_counts,
                                     d_box0, d_prob0, d_rect, d_valid, (hipStream_t)stream);
    TRL_CHECK(trl_rz_end(c, "lists_hook"));         // (after a TRL_ERR_CAPACITY too: the kernels ran)
    return st;
}

// the context's two arenas and, for `what` = 1 (embedder call on n faces of h x w) / 24 / 48 (trl_debug_rnet / _onet on n crops),
// the count of that call, with the call's own argument checks: host bookkeeping only
int trl_debug_workspace(trl_ctx* c, int what, int n, int h, int w, long long* h_out6) {
    TRL_CHECK(trl_check_idle(c));
    if (!h_out6 || (what != 0 && what != 1 && what != 24 && what != 48) || (what && n <= 0) || (what == 1 && (h < 75 || w < 75))) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    if (what && !c->have_weights) { trl_set_error("context without weights"); return TRL_ERR_STATE; }
    Arena X = Arena::counter(c->scratch.guard);
    if (what == 1) TRL_CHECK(embed_need(c, false, n, h, w));
    else if (what) { const NetDesc& d = trl_net_of(what); TRL_CHECK(trl_run_net(c, X, d, 0, Act::dense(nullptr, n, d.side, d.side, 3), nullptr, nullptr)); }
    const size_t v[6] = {c->scratch.cap, c->scratch.high, c->arena.cap, c->arena.off, c->arena_need, what == 1 ? c->fn_need_bytes : X.high};
    for (int k = 0; k < 6; k++) h_out6[k] = (long long)v[k];
    return TRL_OK;
}

// Red zones behind every block of the context's two workspaces, and the sweeps that check them (include/truely_hip.h; rz_sweep above)
int trl_debug_redzone(trl_ctx* c, long long guard, int byte) {
    TRL_CHECK(trl_check_idle(c));
    if (guard < 0 || guard > TRL_RZ_MAX_GUARD || (guard & 255) || byte < 0 || byte > 255) {
        trl_set_error("bad red zone: guard %lld (0, or a multiple of 256 up to %d), fill byte %d", guard, (int)TRL_RZ_MAX_GUARD, byte);
        return TRL_ERR_INVALID;
    }
    trl_ctx::RedZone& z = c->rz;
    if (!guard && !z.guard) return TRL_OK;
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_HIP(hipDeviceSynchronize());
    if (!z.guard) z.saved_poison = c->dbg_poison;
    // both workspaces start over, so that every byte of them is filled by trl_ensure and every block is known
    for (Arena* a : {&c->arena, &c->scratch}) {
        if (a->base) TRL_HIP(hipFree(a->base));
        a->base = nullptr; a->cap = a->off = a->high = 0;
        a->blocks.clear();
        a->guard = (size_t)guard; a->on_rewind = guard ? rz_on_rewind : nullptr; a->owner = c;
    }
    c->cb = CascadeBufs();
    c->arena_need = 0;
    c->fn_need_key[0] = 0;                       // the embedder's count depends on the guard
    z.guard = (size_t)guard; z.byte = byte;
    z.sweeps = z.bytes = z.nhits = 0;
    z.hits.clear();
    c->dbg_poison = guard ? byte : z.saved_poison;
    return TRL_OK;
}

int trl_debug_redzone_report(trl_ctx* c, int flags, long long* h_out4, trl_rz_hit* h_hits, int max_hits) {
    TRL_CHECK(trl_check_idle(c));
    if (!h_out4 || (max_hits > 0 && !h_hits)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    trl_ctx::RedZone& z = c->rz;
    if ((flags & TRL_RZ_SWEEP) && z.guard) {
        TRL_HIP(hipSetDevice(c->cfg.device));
        TRL_CHECK(trl_rz_sweep_all(c, "report"));
    }
    int m = 0;
    for (; m < (int)z.hits.size() && m < max_hits; m++) h_hits[m] = z.hits[m];
    h_out4[0] = z.sweeps; h_out4[1] = z.bytes; h_out4[2] = z.nhits; h_out4[3] = m;
    if (flags & TRL_RZ_CLEAR) { z.sweeps = z.bytes = z.nhits = 0; z.hits.clear(); }
    return TRL_OK;
}

int trl_debug_redzone_poke(trl_ctx* c, int arena, int block, long long offset, int value) {
    TRL_CHECK(trl_check_idle(c));
    trl_ctx::RedZone& z = c->rz;
    if (!z.guard) { trl_set_error("red zones are off"); return TRL_ERR_STATE; }
    if ((arena != 0 && arena != 1) || value < 0 || value > 255 || value == z.byte) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    Arena& a = arena ? c->scratch : c->arena;
    if (!a.base) { trl_set_error("the workspace has not been allocated"); return TRL_ERR_STATE; }
    std::vector<RzGap> gaps;
    rz_gaps(a, gaps);
    if (block < 0) block = (int)a.blocks.size();                            // the tail
    for (const RzGap& g : gaps) {
        if (g.block != block) continue;
        if (offset < 0 || (size_t)offset >= g.len) break;
        TRL_HIP(hipSetDevice(c->cfg.device));
        TRL_HIP(hipDeviceSynchronize());
        TRL_HIP(hipMemset(a.base + g.off + (size_t)offset, value, 1));    // inside [0, cap): a gap of this workspace
        TRL_HIP(hipDeviceSynchronize());
        return TRL_OK;
    }
    trl_set_error("no byte %lld in the gap behind block %d (%zu live blocks)", offset, block, a.blocks.size());
    return TRL_ERR_INVALID;
}

int trl_debug_mtcnn_plan(trl_ctx* c, trl_fn_plan_row* h_rows, int max_rows, int* n_rows) {
    TRL_CHECK(trl_check_idle(c));
    if (!n_rows || (max_rows > 0 && !h_rows)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *n_rows = (int)c->mt_plan.size();
    for (int i = 0; i < *n_rows && i < max_rows; i++) h_rows[i] = c->mt_plan[i];
    return TRL_OK;
}

// test hooks: the three face-crop kernels alone (include/truely_hip.h states the precondition on valid rows).  k_crop_resize80
// indexes frames by grid x, so any n is a legal launch; k_crop_aligned / k_crop_area_std index them by grid y, which the public
// entry points bound through check_call -- these hooks apply the same 65535.
static int check_crop_hook(trl_ctx* c, const void* d_frames, int n, int n_max, int H, int W, const void* d_rows, const void* d_valid,
                           int S, const void* d_faces) {
    if (!c || !d_frames || !d_rows || !d_valid || !d_faces || n <= 0 || n > n_max || H < 1 || W < 1 || S < 1 || S > 4096) {
        trl_set_error("bad argument (n=%d H=%d W=%d S=%d)", n, H, W, S);
        return TRL_ERR_INVALID;
    }
    return TRL_OK;
}
int trl_debug_crop_resize(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid,
                          float* d_faces, void* stream) {
    TRL_CHECK(check_crop_hook(c, d_frames, n, INT_MAX, H, W, d_rect, d_valid, 80, d_faces));
    TRL_CHECK(trl_launch_crop_resize80(d_frames, n, H, W, d_rect, d_valid, d_faces, (hipStream_t)stream));
    return trl_rz_end(c, "crop_resize");
}
// embedding mode 3's crop alone: d_pts [n][10] (x0..x4, y0..y4 per frame) -> f32 [n][S][S][3]
int trl_debug_crop_aligned(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, const float* d_pts, const uint8_t* d_valid, int S,
                           int rgb, float* d_faces, void* stream) {
    TRL_CHECK(check_crop_hook(c, d_frames, n, 65535, H, W, d_pts, d_valid, S, d_faces));
    TRL_CHECK(trl_launch_crop_aligned(d_frames, n, H, W, d_pts, d_valid, S, rgb != 0, d_faces, (hipStream_t)stream));
    return trl_rz_end(c, "crop_aligned");
}
// embedding modes 1 / 2's crop alone: d_rect [n][4] -> f32 [n][S][S][3]
int trl_debug_crop_area(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid, int S,
                        int rgb, float* d_faces, void* stream) {
    TRL_CHECK(check_crop_hook(c, d_frames, n, 65535, H, W, d_rect, d_valid, S, d_faces));
    TRL_CHECK(trl_launch_crop_area_std(d_frames, n, H, W, d_rect, d_valid, S, rgb != 0, d_faces, (hipStream_t)stream));
    return trl_rz_end(c, "crop_area");
}
// test hook: set the optimistic R-/O-Net batch capacities (candidates per frame) the next call starts from, and read back how
// many attempts the last call needed (> 1: a capacity was too small and the call was re-run with a larger one)
// test hook: the LDS tiers of the sort + NMS kernels (candidates per list; 0 keeps a value).  Lists longer than `full` take the
// spill tier (global memory): lowering it makes small test inputs exercise that tier.  Results never depend on the tiers.
int trl_debug_nms_tiers(trl_ctx* c, int small_tier, int full_tier) {
    TRL_CHECK(trl_check_idle(c));
    if ((small_tier && (small_tier < 16 || small_tier > 3072 || (small_tier & 3))) || (full_tier && (full_tier < 16 || full_tier > 3072 || (full_tier & 3)))) {
        trl_set_error("tiers must be multiples of 4 in [16, 3072]");
        return TRL_ERR_INVALID;
    }
    if (small_tier) c->nms_small = small_tier;
    if (full_tier) c->nms_full = full_tier;
    return TRL_OK;
}
// What the candidate lists of the last call looked like: h_out8 = {attempts, lists that took the spill tier, spill bytes used,
// spill bytes available, per-frame list capacity, record slots per frame (all levels), largest per-level count, largest per-frame
// stage-1 total}
int trl_debug_list_stats(trl_ctx* c, long long* h_out8) {
    if (!c || !h_out8) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    const int32_t* f = c->h_pinned + 4;
    unsigned long long used = 0;
    memcpy(&used, f + FLG_SPILL_CUR, 8);
    int mx = 0;
    for (int l = 0; l < 32; l++) if (f[FLG_LEVEL_MAX + l] > mx) mx = f[FLG_LEVEL_MAX + l];
    h_out8[0] = c->caps.last_attempts; h_out8[1] = f[FLG_SPILL_LISTS]; h_out8[2] = (long long)used; h_out8[3] = (long long)c->cb.spill_cap;
    h_out8[4] = c->cb.capF; h_out8[5] = c->cb.lay.S; h_out8[6] = mx; h_out8[7] = f[FLG_FRAME_MAX];
    return TRL_OK;
}

// test hooks of the shipped library (it reads no environment variable): "rnet_chunk" / "onet_chunk" = candidates per R-/O-Net
// launch set of this context (>= 16), "no_fnconv" = process-wide: FaceNet's small maps through the generic conv kernels,
// "pyr_row_bands" = row bands of the streaming pyramid pass of this context (0 = the pass's own policy), "tail_pool" = 1 (default):
// the R-/O-Net tail pools run in their conv's epilogue where one exists, 0: every pool is its own launch (the same bits),
// "pnet_defer" = 1: the fused PNet queues the conv3 M-tiles its screen confirms for a second kernel wherever the launch can defer,
// 0: every launch runs them inline; "pnet_defer_cap" = slots the queue starts from in place of the policy's start (0: the policy).
// Both forget what the queue's capacity had learned (trl_capacity.h)
int trl_debug_option(trl_ctx* c, const char* key, int value) {
    if (!key) { trl_set_error("null key"); return TRL_ERR_INVALID; }
    if (!strcmp(key, "no_fnconv")) { g_trl_no_fnconv = value ? 1 : 0; return TRL_OK; }
    if (!strcmp(key, "pnet_gate")) { g_trl_pnet_gate = value ? 1 : 0; return TRL_OK; }
    TRL_CHECK(trl_check_idle(c));
    if (!strcmp(key, "rnet_chunk") && value >= 16) { c->rnet_chunk = value; return TRL_OK; }
    if (!strcmp(key, "onet_chunk") && value >= 16) { c->onet_chunk = value; return TRL_OK; }
    if (!strcmp(key, "pnet_screen") && (value == 0 || value == 1)) { c->pnet_screen = value; return TRL_OK; }
    if (!strcmp(key, "pnet_defer") && (value == 0 || value == 1)) { c->pnet_defer = value; c->caps.defer = DeferCaps(); return TRL_OK; }
    if (!strcmp(key, "pnet_defer_cap") && value >= 0) { c->caps.defer = DeferCaps(); c->caps.defer.forced = value; return TRL_OK; }
    if (!strcmp(key, "pyr_row_bands") && value >= 0) { c->pyr_row_bands = value; return TRL_OK; }
    if (!strcmp(key, "tail_pool") && (value == 0 || value == 1)) { c->tail_pool = value; return TRL_OK; }
    trl_set_error("unknown option '%s' (or value %d out of range)", key, value);
    return TRL_ERR_INVALID;
}

int trl_debug_pnet_screen_bound(trl_ctx* c, float* A, float* B, int* on) {
    if (!c || !A || !B || !on) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *A = c->pnet_scrA; *B = c->pnet_scrB; *on = c->pnet_screen_ok && c->pnet_screen;
    return TRL_OK;
}

// The confirm queue of the last attempt of the last call: h_out4 = {slots (0: the exact chain ran inline), M-tiles that asked for a
// slot, M-tiles of the launch, calls the inline path is still held for}
int trl_debug_pnet_defer(trl_ctx* c, long long* h_out4) {
    if (!c || !h_out4) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    const DeferCaps& d = c->caps.defer;
    h_out4[0] = d.cap; h_out4[1] = d.cap > 0 ? c->h_pinned[4 + FLG_DEFER_N] : 0; h_out4[2] = d.mtiles; h_out4[3] = d.hold;
    return TRL_OK;
}

int trl_debug_pnet_screen_weights(trl_ctx* c, float* h_g16) {
    if (!c || !h_g16) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    for (int i = 0; i < 16; i++) h_g16[i] = c->pnet_scrG[i];
    return TRL_OK;
}

int trl_debug_batch_capacity(trl_ctx* c, float t2_per_frame, float t3_per_frame, int* last_attempts) {
    if (!c) { trl_set_error("null context"); return TRL_ERR_INVALID; }
    if (t2_per_frame > 0.f) c->caps.t_per_frame[0] = t2_per_frame;
    if (t3_per_frame > 0.f) c->caps.t_per_frame[1] = t3_per_frame;
    if (last_attempts) *last_attempts = c->caps.last_attempts;
    return TRL_OK;
}

// R-Net / O-Net candidate totals of the last call (what the front kernels and the tails processed)
int trl_debug_stage_totals(trl_ctx* c, int32_t* h_out2) {
    if (!c || !h_out2) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    h_out2[0] = c->h_pinned[4 + FLG_T2N]; h_out2[1] = c->h_pinned[4 + FLG_T3N];
    return TRL_OK;
}

// test / tuning hook: consecutive tiles a workgroup of the fused PNet launch takes per cursor fetch (0 = automatic).  Runs > 1
// let a tile reuse its left neighbour's halo columns (the carry path); results are identical for every value.
int trl_debug_pnet_run(trl_ctx* c, int run) {
    if (!c || run < 0 || run > 64) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    c->pnet_run = run;
    return TRL_OK;
}

int trl_debug_pnet_span(trl_ctx* c, int reset, double* ms_sum, int32_t* launches) {
    if (!c || !ms_sum || !launches) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *ms_sum = 0.0; *launches = 0;
    if (!c->pnet_clk) return TRL_OK;
    TRL_CHECK(trl_check_idle(c));
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_HIP(hipDeviceSynchronize());                 // the stamps are written by kernels on the callers' streams
    unsigned long long t[2] = {0, 0};
    int khz = 0;
    TRL_HIP(hipMemcpy(t, c->pnet_clk + 36, sizeof t, hipMemcpyDeviceToHost));
    TRL_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device));
    if (khz > 0) *ms_sum = (double)t[0] / (double)khz;
    *launches = (int32_t)t[1];
    if (reset) TRL_HIP(hipMemset(c->pnet_clk + 36, 0, 16));
    return TRL_OK;
}

int trl_debug_pnet_kernel_ms(trl_ctx* c, float* ms) {
    if (!c || !ms) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *ms = c->pnet_kernel_ms;
    return TRL_OK;
}

int trl_debug_timings(trl_ctx* c, float* out4) {
    if (!c || !out4) return TRL_ERR_INVALID;
    out4[0] = c->last_ms[0]; out4[1] = c->last_ms[1]; out4[2] = c->last_ms[2]; out4[3] = c->last_ms[3];
    return TRL_OK;
}

}  // extern "C"

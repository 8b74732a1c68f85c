// trl_api.hip -- C ABI of libtruely_hip.so (see include/truely_hip.h for the contract and the
// reference lines each entry point replaces): what a production call runs.  The trl_debug_* hooks are in trl_hooks.hip, the red
// zones in trl_redzone.hip.
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
    if (hipMalloc((void**)&c->pnet_clk, 8 * CLK_WORDS) != hipSuccess || hipMemset(c->pnet_clk, 0, 8 * CLK_WORDS) != hipSuccess ||
        hipMemset(c->pnet_clk + CLK_START, 0xFF, 8) != hipSuccess ||
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
    if (c->hook.rz.dev) (void)hipFree(c->hook.rz.dev);
    for (auto& b : c->hook.fn_cap) if (b.p) (void)hipFree(b.p);
    if (c->pnet_clk) {
        // TRL_PNET_CLOCK: where the waves of the fused PNet launches spent their time (shader clocks per tile and wave, DBG instantiation)
        unsigned long long t[CLK_QUEUED + 1];
        if (c->pnet_prof && hipMemcpy(t, c->pnet_clk, sizeof t, hipMemcpyDeviceToHost) == hipSuccess && t[CLK_ROT] > 0) {
            static const char* nm[8] = {"phase0", "barrier0", "phase1", "barrier1", "phase2", "barrier2", "phase3", "barrier3"};
            const double tiles = (double)t[CLK_ROT];
            fprintf(stderr, "[TRL_PNET_CLOCK] shader clocks per tile (wave 0..3), %.0f workgroup-tiles\n", tiles);
            for (int k = 0; k < 8; k++)
                fprintf(stderr, "[TRL_PNET_CLOCK] %-9s %8.0f %8.0f %8.0f %8.0f\n", nm[k], t[CLK_PHASE + k] / tiles, t[CLK_PHASE + 8 + k] / tiles,
                        t[CLK_PHASE + 16 + k] / tiles, t[CLK_PHASE + 24 + k] / tiles);
            fprintf(stderr, "[TRL_PNET_CLOCK] fp16 screen: %llu M-tiles screened, %llu confirmed (%.2f %%)\n", t[CLK_SCREENED], t[CLK_CONFIRMED],
                    t[CLK_SCREENED] ? 100.0 * (double)t[CLK_CONFIRMED] / (double)t[CLK_SCREENED] : 0.0);
            fprintf(stderr, "[TRL_PNET_CLOCK] confirm queue: %llu M-tiles queued, %.0f per launch\n", t[CLK_QUEUED],
                    t[CLK_LAUNCHES] ? (double)t[CLK_QUEUED] / (double)t[CLK_LAUNCHES] : 0.0);
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

int trl_ensure(trl_ctx* c, Arena& a, size_t bytes) {
    if (bytes <= a.cap) return TRL_OK;
    // Growing frees the old block, so it is only called while nothing allocated from `a` is live:
    // at the start of a call (arena) or between cascade stages (scratch).
    const size_t ncap = bytes + (bytes >> 3) + (32u << 20);
    TRL_HIP(hipDeviceSynchronize());
    if (a.guard && a.base) TRL_CHECK(trl_rz_sweep(c, "ensure", &a));
    if (a.base) { TRL_HIP(hipFree(a.base)); a.base = nullptr; a.cap = 0; }
    TRL_HIP(hipMalloc((void**)&a.base, ncap));
    a.cap = ncap;
    a.off = 0;
    a.blocks.clear();
    if (c->hook.dbg_poison >= 0) TRL_HIP(hipMemset(a.base, c->hook.dbg_poison, ncap));   // test hook: workspaces that grow stay poisoned
    return TRL_OK;
}

// ---- hot path ---------------------------------------------------------------------------------------
int trl_check_idle(trl_ctx* c) {
    if (!c) { trl_set_error("null context"); return TRL_ERR_INVALID; }
    if (c->pend.active) { trl_set_error("the context has a call in flight: trl_detect_embed_end() first"); return TRL_ERR_STATE; }
    return TRL_OK;
}

int trl_check_call(trl_ctx* c, const void* frames, int n, int H, int W) {
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
        if (hipMemcpy(&t, c->pnet_clk + CLK_LAST_SPAN, sizeof t, hipMemcpyDeviceToHost) == hipSuccess &&
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
int trl_embed_need(trl_ctx* c, bool crops, int n, int h, int w) {
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
    TRL_CHECK(trl_check_call(c, q.frames, q.n, q.H, q.W));
    if (q.kind == trl_ctx::Pending::DETECT ? !(q.boxes && q.probs && q.counts) : !(q.box && q.prob && q.rect && q.valid && (q.emb || q.faces_out))) {
        trl_set_error("null output");
        return TRL_ERR_INVALID;
    }
    TRL_HIP(hipSetDevice(c->cfg.device));
    const int S = c->cfg.embed_mode == 0 ? 80 : 160;
    if (q.kind == trl_ctx::Pending::EMBED) TRL_CHECK(trl_embed_need(c, true, q.n, S, S));
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
    TRL_CHECK(trl_embed_need(c, false, n, h, w));
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

}  // extern "C"

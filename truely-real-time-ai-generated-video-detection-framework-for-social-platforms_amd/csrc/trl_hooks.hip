// trl_hooks.hip -- the trl_debug_* inspection and test hooks of a context (include/truely_hip.h); the red-zone hooks are in
// trl_redzone.hip.  No production call runs anything in this file.
//
// Every hook opens in one of two ways.  One that touches the device or the workspaces: trl_hook_device (trl_ctx.h) -- no call in
// flight, the context's device current -- then its own argument checks (the stage hooks: trl_check_call's).  One that only reads or
// writes host fields of the context: hook_host, a null check with the hook's own message; those of them that must not change
// what a queued call still reads refuse it with trl_check_idle, whose null check is then theirs.  The three crop hooks launch
// beside a call in flight as they always did: check_crop_hook is their whole way in.
#include <limits.h>
#include <string.h>

#include "trl_ctx.h"

namespace {
// the host prologue.  args_ok: the hook's required pointers (and ranges, where it names none); msg == null: the last error stays
int hook_host(const trl_ctx* c, bool args_ok, const char* msg) {
    if (c && args_ok) return TRL_OK;
    if (msg) trl_set_error("%s", msg);
    return TRL_ERR_INVALID;
}
// at most max_rows of the n host rows row(0) .. row(n - 1) into h_rows; *n_out = n
template <class Row, class F> int copy_rows(Row* h_rows, int max_rows, int* n_out, int n, F&& row) {
    if (!n_out || (max_rows > 0 && !h_rows)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    *n_out = n;
    for (int i = 0; i < n && i < max_rows; i++) h_rows[i] = row(i);
    return TRL_OK;
}
// *n_out = the device count *d_count, at most `cap`; the first min(*n_out, max_rows) rows of row_bytes from d_rows into h_rows
int read_rows(const int32_t* d_count, int cap, const void* d_rows, size_t row_bytes, void* h_rows, int max_rows, int* n_out) {
    int32_t k = 0;
    TRL_HIP(hipDeviceSynchronize());
    TRL_HIP(hipMemcpy(&k, d_count, 4, hipMemcpyDeviceToHost));
    if (k > cap) k = cap;
    *n_out = k;
    const int m = k < max_rows ? k : max_rows;
    if (m > 0) TRL_HIP(hipMemcpy(h_rows, d_rows, (size_t)m * row_bytes, hipMemcpyDeviceToHost));
    return TRL_OK;
}
int no_cascade_state() { trl_set_error("no cascade state"); return TRL_ERR_STATE; }
}  // namespace

extern "C" __global__ void k_poison_lds(unsigned word, int nwords) {   // (C linkage: the name it had among the entry points of trl_api.hip)
    extern __shared__ unsigned lds_words[];
    for (int i = threadIdx.x; i < nwords; i += blockDim.x) lds_words[i] = word;
    __syncthreads();
    if (lds_words[(threadIdx.x * 97) % nwords] != word) __builtin_trap();   // keeps the stores alive
}

// ---- the state the last call left ----------------------------------------------------------------------
extern "C" {

int trl_debug_stage_boxes(trl_ctx* c, int stage, int frame, float* h_boxes, int max_rows, int* n_out) {
    TRL_CHECK(trl_hook_device(c));
    if (!c->cb.cnt[0] || frame < 0 || frame >= c->cb.n || stage < 1 || stage > 3 || !n_out || (max_rows > 0 && !h_boxes)) return no_cascade_state();
    return read_rows(c->cb.cnt[stage - 1] + frame, INT_MAX, c->cb.box[stage - 1] + (size_t)frame * c->cb.capF * 5, 20, h_boxes, max_rows, n_out);
}

int trl_debug_level_counts(trl_ctx* c, int frame, int32_t* h_cand, int32_t* h_keep, int* n_levels) {
    TRL_CHECK(trl_hook_device(c));
    if (!c->cb.lvl_cnt || frame < 0 || frame >= c->cb.n || !h_cand || !h_keep || !n_levels) return no_cascade_state();
    TRL_HIP(hipDeviceSynchronize());
    const int L = c->cb.L;
    TRL_HIP(hipMemcpy(h_cand, c->cb.lvl_cnt + (size_t)frame * L, (size_t)L * 4, hipMemcpyDeviceToHost));
    TRL_HIP(hipMemcpy(h_keep, c->cb.lvl_keep_cnt + (size_t)frame * L, (size_t)L * 4, hipMemcpyDeviceToHost));
    *n_levels = L;
    return TRL_OK;
}

// Candidate records (generateBoundingBox rows) one (frame, level) of the last call produced, in append order
int trl_debug_level_cands(trl_ctx* c, int frame, int level, void* h_rows, int max_rows, int* n_out) {
    TRL_CHECK(trl_hook_device(c));
    if (!c->cb.lvl_cnt || frame < 0 || frame >= c->cb.n || level < 0 || level >= c->cb.L || !n_out || (max_rows > 0 && !h_rows)) return no_cascade_state();
    static_assert(sizeof(Cand) == 40, "trl_debug_level_cands row layout");
    return read_rows(c->cb.lvl_cnt + (size_t)frame * c->cb.L + level, c->cb.lay.capl[level],
                     c->cb.lvl_rec + (size_t)frame * c->cb.lay.S + c->cb.lay.rec0[level], sizeof(Cand), h_rows, max_rows, n_out);
}

// The per-level NMS picks of one (frame, level) of the last call: indices into that level's candidate records (the rows
// trl_debug_level_cands returns, in the same append order), in pick order (descending score)
int trl_debug_level_keep(trl_ctx* c, int frame, int level, int32_t* h_idx, int max_rows, int* n_out) {
    TRL_CHECK(trl_hook_device(c));
    if (!c->cb.lvl_keep_cnt || frame < 0 || frame >= c->cb.n || level < 0 || level >= c->cb.L || !n_out || (max_rows > 0 && !h_idx)) return no_cascade_state();
    return read_rows(c->cb.lvl_keep_cnt + (size_t)frame * c->cb.L + level, INT_MAX,
                     c->cb.lvl_keep_idx + (size_t)frame * c->cb.lay.S + c->cb.lay.rec0[level], 4, h_idx, max_rows, n_out);
}

// What the candidate lists of the last call looked like: h_out8 = {attempts, lists that took the spill tier, spill bytes used,
// spill bytes available, per-frame list capacity, record slots per frame (all levels), largest per-level count, largest per-frame
// stage-1 total}
int trl_debug_list_stats(trl_ctx* c, long long* h_out8) {
    TRL_CHECK(hook_host(c, h_out8, "null argument"));
    const int32_t* f = trl_host_flags(c);
    unsigned long long used = 0;
    memcpy(&used, f + FLG_SPILL_CUR, 8);
    int mx = 0;
    for (int l = 0; l < 32; l++) if (f[FLG_LEVEL_MAX + l] > mx) mx = f[FLG_LEVEL_MAX + l];
    h_out8[0] = c->caps.last_attempts; h_out8[1] = f[FLG_SPILL_LISTS]; h_out8[2] = (long long)used; h_out8[3] = (long long)c->cb.spill_cap;
    h_out8[4] = c->cb.capF; h_out8[5] = c->cb.lay.S; h_out8[6] = mx; h_out8[7] = f[FLG_FRAME_MAX];
    return TRL_OK;
}

// R-Net / O-Net candidate totals of the last call (what the front kernels and the tails processed)
int trl_debug_stage_totals(trl_ctx* c, int32_t* h_out2) {
    TRL_CHECK(hook_host(c, h_out2, "null argument"));
    h_out2[0] = trl_host_flags(c)[FLG_T2N]; h_out2[1] = trl_host_flags(c)[FLG_T3N];
    return TRL_OK;
}

// The confirm queue of the last attempt of the last call: h_out4 = {slots (0: the exact chain ran inline), M-tiles that asked for a
// slot, M-tiles of the launch, calls the inline path is still held for}
int trl_debug_pnet_defer(trl_ctx* c, long long* h_out4) {
    TRL_CHECK(hook_host(c, h_out4, "null argument"));
    const DeferCaps& d = c->caps.defer;
    h_out4[0] = d.cap; h_out4[1] = d.cap > 0 ? trl_host_flags(c)[FLG_DEFER_N] : 0; h_out4[2] = d.mtiles; h_out4[3] = d.hold;
    return TRL_OK;
}

int trl_debug_timings(trl_ctx* c, float* out4) {
    TRL_CHECK(hook_host(c, out4, nullptr));
    out4[0] = c->last_ms[0]; out4[1] = c->last_ms[1]; out4[2] = c->last_ms[2]; out4[3] = c->last_ms[3];
    return TRL_OK;
}

int trl_debug_pnet_kernel_ms(trl_ctx* c, float* ms) {
    TRL_CHECK(hook_host(c, ms, "null argument"));
    *ms = c->pnet_kernel_ms;
    return TRL_OK;
}

int trl_debug_pnet_span(trl_ctx* c, int reset, double* ms_sum, int32_t* launches) {
    TRL_CHECK(hook_host(c, ms_sum && launches, "null argument"));
    *ms_sum = 0.0; *launches = 0;
    if (!c->pnet_clk) return TRL_OK;
    TRL_CHECK(trl_hook_device(c));
    TRL_HIP(hipDeviceSynchronize());                 // the stamps are written by kernels on the callers' streams
    unsigned long long t[2] = {0, 0};                // CLK_SPAN_SUM, CLK_LAUNCHES
    int khz = 0;
    TRL_HIP(hipMemcpy(t, c->pnet_clk + CLK_SPAN_SUM, sizeof t, hipMemcpyDeviceToHost));
    TRL_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device));
    if (khz > 0) *ms_sum = (double)t[0] / (double)khz;
    *launches = (int32_t)t[1];
    if (reset) TRL_HIP(hipMemset(c->pnet_clk + CLK_SPAN_SUM, 0, sizeof t));
    return TRL_OK;
}

int trl_debug_pnet_screen_bound(trl_ctx* c, float* A, float* B, int* on) {
    TRL_CHECK(hook_host(c, A && B && on, "null argument"));
    *A = c->pnet_scrA; *B = c->pnet_scrB; *on = c->pnet_screen_ok && c->opt.pnet_screen;
    return TRL_OK;
}

int trl_debug_pnet_screen_weights(trl_ctx* c, float* h_g16) {
    TRL_CHECK(hook_host(c, h_g16, "null argument"));
    for (int i = 0; i < 16; i++) h_g16[i] = c->pnet_scrG[i];
    return TRL_OK;
}

int trl_debug_pyramid_plan(trl_ctx* c, int32_t* h_rows, int max_levels, int* n_levels) {
    TRL_CHECK(trl_check_idle(c));
    struct Row { int32_t v[TRL_PYR_PLAN_COLS]; };
    return copy_rows((Row*)h_rows, max_levels, n_levels, c->hook.pyr_plan.L, [&](int l) { Row r; memcpy(r.v, c->hook.pyr_plan.row[l], sizeof r.v); return r; });
}

int trl_debug_facenet_plan(trl_ctx* c, trl_fn_plan_row* h_rows, int max_rows, int* n_rows) {
    TRL_CHECK(trl_check_idle(c));
    return copy_rows(h_rows, max_rows, n_rows, (int)c->hook.fn_plan.size(), [&](int i) { return c->hook.fn_plan[i]; });
}

int trl_debug_mtcnn_plan(trl_ctx* c, trl_fn_plan_row* h_rows, int max_rows, int* n_rows) {
    TRL_CHECK(trl_check_idle(c));
    return copy_rows(h_rows, max_rows, n_rows, (int)c->hook.mt_plan.size(), [&](int i) { return c->hook.mt_plan[i]; });
}

int trl_debug_facenet_capture(trl_ctx* c, int conv_index) {
    TRL_CHECK(trl_check_idle(c));
    c->hook.fn_cap_arm = conv_index < 0 ? -1 : conv_index;
    return TRL_OK;
}

int trl_debug_facenet_capture_read(trl_ctx* c, int view, void* h_dst, size_t max_bytes, int32_t* dims5) {
    TRL_CHECK(trl_hook_device(c));
    if (view < 0 || view > 2 || !dims5) { trl_set_error("bad capture view %d", view); return TRL_ERR_INVALID; }
    const auto& b = c->hook.fn_cap[view];
    for (int k = 0; k < 5; k++) dims5[k] = b.dims[k];
    if (!h_dst || b.dims[3] == 0) return TRL_OK;
    const size_t bytes = (size_t)b.dims[0] * b.dims[1] * b.dims[2] * b.dims[3] * b.dims[4];
    if (bytes > max_bytes) { trl_set_error("capture needs %zu bytes", bytes); return TRL_ERR_INVALID; }
    TRL_HIP(hipDeviceSynchronize());
    TRL_HIP(hipMemcpy(h_dst, b.p, bytes, hipMemcpyDeviceToHost));
    return TRL_OK;
}

// the context's two arenas and, for `what` = 1 (embedder call on n faces of h x w) / 24 / 48 (trl_debug_rnet / _onet on n crops),
// the count of that call, with the call's own argument checks: host bookkeeping only
int trl_debug_workspace(trl_ctx* c, int what, int n, int h, int w, long long* h_out6) {
    TRL_CHECK(trl_check_idle(c));
    if (!h_out6 || (what != 0 && what != 1 && what != 24 && what != 48) || (what && n <= 0) || (what == 1 && (h < 75 || w < 75))) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    if (what && !c->have_weights) { trl_set_error("context without weights"); return TRL_ERR_STATE; }
    Arena X = Arena::counter(c->scratch.guard);
    if (what == 1) TRL_CHECK(trl_embed_need(c, false, n, h, w));
    else if (what) { const NetDesc& d = trl_net_of(what); TRL_CHECK(trl_run_net(c, X, d, 0, Act::dense(nullptr, n, d.side, d.side, 3), nullptr, nullptr)); }
    const size_t v[6] = {c->scratch.cap, c->scratch.high, c->arena.cap, c->arena.off, c->arena_need, what == 1 ? c->fn_need_bytes : X.high};
    for (int k = 0; k < 6; k++) h_out6[k] = (long long)v[k];
    return TRL_OK;
}

// ---- what the next calls run on ------------------------------------------------------------------------
// Fills every byte of the activation workspaces with `byte` (0xFF = NaN patterns, 0x7F = huge finite floats): a
// result that depends on workspace contents left by an earlier call or process shows up as a parity failure.
int trl_debug_poison(trl_ctx* c, int byte) {
    TRL_CHECK(trl_hook_device(c));
    if (c->hook.rz.guard) { trl_set_error("red zones are on: their fill byte is the poison"); return TRL_ERR_STATE; }
    TRL_HIP(hipDeviceSynchronize());
    c->hook.dbg_poison = byte & 0xFF;            // sticky: blocks allocated later are filled too
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
    Options& o = c->opt;
    if (!strcmp(key, "rnet_chunk") && value >= 16) { o.rnet_chunk = value; return TRL_OK; }
    if (!strcmp(key, "onet_chunk") && value >= 16) { o.onet_chunk = value; return TRL_OK; }
    if (!strcmp(key, "pnet_screen") && (value == 0 || value == 1)) { o.pnet_screen = value; return TRL_OK; }
    if (!strcmp(key, "pnet_defer") && (value == 0 || value == 1)) { o.pnet_defer = value; c->caps.defer = DeferCaps(); return TRL_OK; }
    if (!strcmp(key, "pnet_defer_cap") && value >= 0) { c->caps.defer = DeferCaps(); c->caps.defer.forced = value; return TRL_OK; }
    if (!strcmp(key, "pyr_row_bands") && value >= 0) { o.pyr_row_bands = value; return TRL_OK; }
    if (!strcmp(key, "tail_pool") && (value == 0 || value == 1)) { o.tail_pool = value; return TRL_OK; }
    trl_set_error("unknown option '%s' (or value %d out of range)", key, value);
    return TRL_ERR_INVALID;
}

// test hook: the LDS tiers of the sort + NMS kernels (candidates per list; 0 keeps a value).  Lists longer than `full` take the
// spill tier (global memory): lowering it makes small test inputs exercise that tier.  Results never depend on the tiers.
int trl_debug_nms_tiers(trl_ctx* c, int small_tier, int full_tier) {
    TRL_CHECK(trl_check_idle(c));
    if ((small_tier && (small_tier < 16 || small_tier > 3072 || (small_tier & 3))) || (full_tier && (full_tier < 16 || full_tier > 3072 || (full_tier & 3)))) {
        trl_set_error("tiers must be multiples of 4 in [16, 3072]");
        return TRL_ERR_INVALID;
    }
    if (small_tier) c->opt.nms_small = small_tier;
    if (full_tier) c->opt.nms_full = full_tier;
    return TRL_OK;
}

// test / tuning hook: consecutive tiles a workgroup of the fused PNet launch takes per cursor fetch (0 = automatic).  Runs > 1
// let a tile reuse its left neighbour's halo columns (the carry path); results are identical for every value.
int trl_debug_pnet_run(trl_ctx* c, int run) {
    TRL_CHECK(hook_host(c, run >= 0 && run <= 64, "bad argument"));
    c->opt.pnet_run = run;
    return TRL_OK;
}

// test hook: set the optimistic R-/O-Net batch capacities (candidates per frame) the next call starts from, and read back how
// many attempts the last call needed (> 1: a capacity was too small and the call was re-run with a larger one)
int trl_debug_batch_capacity(trl_ctx* c, float t2_per_frame, float t3_per_frame, int* last_attempts) {
    TRL_CHECK(hook_host(c, true, "null context"));
    if (t2_per_frame > 0.f) c->caps.t_per_frame[0] = t2_per_frame;
    if (t3_per_frame > 0.f) c->caps.t_per_frame[1] = t3_per_frame;
    if (last_attempts) *last_attempts = c->caps.last_attempts;
    return TRL_OK;
}

// ---- parts of the pipeline on their own ----------------------------------------------------------------
int trl_debug_pyramid_level(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_out, int* h, int* w, void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frame, 1, H, W));
    hipStream_t s = (hipStream_t)stream;
    TRL_CHECK(trl_scratch_begin(c, trl_pnet_fused_bytes(c, 1, H, W) + (1u << 20)));
    TRL_CHECK(trl_pyramid_export(c, d_frame, H, W, level, d_out, h, w, s));
    TRL_HIP(hipStreamSynchronize(s));
    return trl_rz_end(c, "pyramid_level");
}

int trl_debug_pyramid_batch(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_out, long long* pyr_stride,
                            int32_t* h_levels, int max_levels, int* n_levels, void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frames, n, H, W));
    if (!pyr_stride || !n_levels || (max_levels > 0 && !h_levels)) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    hipStream_t s = (hipStream_t)stream;
    if (d_out) TRL_CHECK(trl_scratch_begin(c, trl_pnet_fused_bytes(c, n, H, W) + (1u << 20)));
    TRL_CHECK(trl_pyramid_export_batch(c, d_frames, n, H, W, d_out, pyr_stride, h_levels, max_levels, n_levels, s));
    TRL_HIP(hipStreamSynchronize(s));
    return trl_rz_end(c, "pyramid_batch");
}

int trl_debug_pnet_level(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_prob, float* d_reg, int* oh, int* ow,
                         void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frame, 1, H, W));
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

}  // extern "C"

// test hooks: a whole net through the layer kernels over n crops [n][side][side][3]: d_out [n][6] (R-Net) / [n][16] (O-Net)
static int debug_net(trl_ctx* c, const NetDesc& d, const float* d_crops, int n, float* d_out, void* stream) {
    TRL_CHECK(hook_host(c, c && c->have_weights && d_crops && d_out && n > 0, "bad argument"));
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_carve_scratch(c, [&](Arena& X) { return trl_run_net(c, X, d, 0, Act::dense(d_crops, n, d.side, d.side, 3), d_out, (hipStream_t)stream); }));
    return trl_rz_end(c, "debug_net");
}

static const int32_t kRecordPoison = (int32_t)0xA5A5A5A5;  // frame / window words no live record has
// k_build_map's records on the device for a front launch outside the cascade: `slots` records of 8 words, the nb live ones first --
// row(i, r) writes r[0..4] = {frame, y0, x0, ih, iw} of record i or refuses it -- and the poison in the slots behind them (the
// kernels read those, then discard them); c->cb then describes the batch and the record list, *total is the device-side count nb.
template <class F>
static int upload_records(trl_ctx* c, int nf, int H, int W, int slots, int nb, int32_t** total, hipStream_t s, F&& row) {
    std::vector<int32_t> hb((size_t)slots * 8, kRecordPoison);
    for (int i = 0; i < nb; i++) {
        int32_t* r = &hb[8 * (size_t)i];
        TRL_CHECK(row(i, r));
        r[5] = r[6] = r[7] = 0;
    }
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

// The production stage-2 / stage-3 loop (trl_stage_net, as the cascade runs it) over a launch capacity the caller chooses.  h_rows:
// nb host rows of `cols` floats -- (frame, x1, y1, x2, y2), or (x1, y1, x2, y2) of frame 0 when cols = 4 -- turned into
// k_build_map's records by pad() (detect_face.py: trunc, x = max(x1, 1), ex = min(x2, W), crop [y-1:ey, x-1:ex]); the device
// total is nb, and record slots past it hold upload_records' poison.  The workspace is sized
// like the cascade's: chunk = the rnet_chunk / onet_chunk option.  d_out: [capacity][6] (net = 24) or [capacity][16] (net = 48),
// device; only rows of live candidates are defined.  trl_debug_mtcnn_plan then lists the tail's conv launches of every chunk.
static int stage_net_on_rows(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const float* h_rows, int cols, int nb, int net,
                             int capacity, float* d_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int32_t* total = nullptr;
    TRL_CHECK(upload_records(c, nf, H, W, nb > capacity ? nb : capacity, nb, &total, s, [&](int i, int32_t* r) {
        const float* b = h_rows + (size_t)cols * i + cols - 4;
        const int f = cols == 5 ? (int)b[-1] : 0;
        if (f < 0 || f >= nf) { trl_set_error("record %d: frame %d of %d", i, f, nf); return TRL_ERR_INVALID; }
        const int bx = (int)truncf(b[0]), by = (int)truncf(b[1]), bex = (int)truncf(b[2]), bey = (int)truncf(b[3]);
        const int x = bx < 1 ? 1 : bx, y = by < 1 ? 1 : by, ex = bex > W ? W : bex, ey = bey > H ? H : bey;
        if (ey <= y - 1 || ex <= x - 1) { trl_set_error("record %d: empty crop window", i); return TRL_ERR_INVALID; }
        r[0] = f; r[1] = y - 1; r[2] = x - 1; r[3] = ey - (y - 1); r[4] = ex - (x - 1);
        return TRL_OK;
    }));
    c->hook.mt_plan.clear();
    c->hook.mt_plan_arm = true;
    const int st = trl_carve_scratch(c, [&](Arena& X) { return trl_stage_net(c, X, net, d_frames, H, W, total, capacity, d_out, s); });
    c->hook.mt_plan_arm = false;
    TRL_CHECK(st);
    TRL_HIP(hipStreamSynchronize(s));
    c->cb = CascadeBufs();                                 // no cascade state to inspect after this hook
    return trl_rz_end(c, "stage_net");
}

// test hooks: the three face-crop kernels alone (include/truely_hip.h states the precondition on valid rows).  k_crop_resize80
// indexes frames by grid x, so any n is a legal launch; k_crop_aligned / k_crop_area_std index them by grid y, which the public
// entry points bound through trl_check_call -- these hooks apply the same 65535.
static int check_crop_hook(trl_ctx* c, const void* d_frames, int n, int n_max, int H, int W, const void* d_rows, const void* d_valid,
                           int S, const void* d_faces) {
    if (!c || !d_frames || !d_rows || !d_valid || !d_faces || n <= 0 || n > n_max || H < 1 || W < 1 || S < 1 || S > 4096) {
        trl_set_error("bad argument (n=%d H=%d W=%d S=%d)", n, H, W, S);
        return TRL_ERR_INVALID;
    }
    return TRL_OK;
}

extern "C" {

int trl_debug_rnet(trl_ctx* c, const float* d_crops, int n, float* d_out, void* stream) { return debug_net(c, trl_nets[TRL_RNET], d_crops, n, d_out, stream); }
int trl_debug_onet(trl_ctx* c, const float* d_crops, int n, float* d_out, void* stream) { return debug_net(c, trl_nets[TRL_ONET], d_crops, n, d_out, stream); }

// test hook: the production stage-2 / stage-3 network path -- the fused front kernel (k_mtcnn_front: pad(), crop, area resample,
// conv1, PReLU, pool) followed by the layer tail -- on caller-chosen boxes of frame 0, so its crop paths (small boxes, big boxes,
// boxes clipped by the frame) are checked directly, not only through cascade records.  h_boxes: nb rows of x1,y1,x2,y2 (host),
// none with an empty crop window; d_out: [nb][6] (net = 24) or [nb][16] (net = 48), device.
int trl_debug_front_net(trl_ctx* c, const uint8_t* d_frame, int H, int W, const float* h_boxes, int nb, int net, float* d_out, void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frame, 1, H, W));
    if (!h_boxes || !d_out || nb <= 0 || nb > (1 << 20) || (net != 24 && net != 48)) { trl_set_error("bad argument"); return TRL_ERR_INVALID; }
    return stage_net_on_rows(c, d_frame, 1, H, W, h_boxes, 4, nb, net, nb, d_out, stream);
}

int trl_debug_stage_net(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const float* h_recs, int nb, int net, int capacity,
                        float* d_out, void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frames, nf, H, W));
    if ((nb > 0 && !h_recs) || (capacity > 0 && !d_out) || nb < 0 || nb > (1 << 24) || capacity < 0 || capacity > (1 << 24) ||
        (net != 24 && net != 48)) {
        trl_set_error("bad argument");
        return TRL_ERR_INVALID;
    }
    return stage_net_on_rows(c, d_frames, nf, H, W, h_recs, 5, nb, net, capacity, d_out, stream);
}

// test hook: k_mtcnn_front alone.  h_win: nb host rows {frame, y0, x0, ih, iw}, k_build_map's record given directly (no pad()); the
// kernel checks nothing, so every row is checked here.  Record slots nb .. capacity-1 hold upload_records' poison, the
// device total is nb, and the launch is trl_stage_net's: one chunk at t0 = 0 over `capacity` slots, writing the pooled maps
// [capacity][11][11][28] (net = 24) / [capacity][23][23][32] (net = 48) straight into d_pool.  No tail runs.
int trl_debug_front(trl_ctx* c, const uint8_t* d_frames, int nf, int H, int W, const int32_t* h_win, int nb, int net, int capacity,
                    float* d_pool, void* stream) {
    TRL_CHECK(trl_hook_device(c));
    TRL_CHECK(trl_check_call(c, d_frames, nf, H, W));
    if ((nb > 0 && !h_win) || (capacity > 0 && !d_pool) || nb < 0 || nb > (1 << 20) || capacity < 0 || capacity > (1 << 20) ||
        (net != 24 && net != 48)) {
        trl_set_error("bad argument");
        return TRL_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* total = nullptr;
    TRL_CHECK(upload_records(c, nf, H, W, nb > capacity ? nb : capacity, nb, &total, s, [&](int i, int32_t* q) {
        const int32_t* r = h_win + 5 * (size_t)i;
        const long long f = r[0], y0 = r[1], x0 = r[2], ih = r[3], iw = r[4];
        if (f < 0 || f >= nf || ih < 1 || iw < 1 || y0 < 0 || x0 < 0 || y0 + ih > H || x0 + iw > W) {
            trl_set_error("window %d: frame %lld of %d, rows %lld + %lld of %d, columns %lld + %lld of %d", i, f, nf, y0, ih, H, x0, iw, W);
            return TRL_ERR_INVALID;
        }
        for (int k = 0; k < 5; k++) q[k] = r[k];
        return TRL_OK;
    }));
    TRL_CHECK(trl_launch_front(c, trl_net_of(net), d_frames, H, W, total, 0, capacity, d_pool, s));
    TRL_HIP(hipStreamSynchronize(s));
    c->cb = CascadeBufs();
    return trl_rz_end(c, "front");
}

// test hook: the cascade's list kernels on caller-built lists (trl_cascade_lists has the layout of every kind)
int trl_debug_lists(trl_ctx* c, int kind, int n, int H, int W, const int32_t* h_caps, int n_levels, const int32_t* h_counts,
                    const void* h_rows, const float* h_logits, float* h_pts, float* d_boxes, float* d_probs, float* d_points,
                    int32_t* d_counts, float* d_box0, float* d_prob0, int32_t* d_rect, uint8_t* d_valid, void* stream) {
    TRL_CHECK(trl_hook_device(c));
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
    const int st = trl_cascade_lists(c, kind, n, H, W, h_caps, n_levels, h_counts, h_rows, h_logits, h_pts, d_boxes, d_probs, d_points, d_counts,
                                     d_box0, d_prob0, d_rect, d_valid, (hipStream_t)stream);
    TRL_CHECK(trl_rz_end(c, "lists_hook"));         // (after a TRL_ERR_CAPACITY too: the kernels ran)
    return st;
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

}  // extern "C"

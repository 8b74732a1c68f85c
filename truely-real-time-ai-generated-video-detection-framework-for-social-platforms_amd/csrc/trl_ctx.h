// trl_ctx.h -- the opaque context behind the C ABI.
#pragma once
#include "trl_common.h"
#include "trl_capacity.h"   // LvLayout, the FLG_* words, CascadeCaps
#include "trl_facenet.h"    // FaceNet's table of convs: FN_ROWS

// One PNet candidate (generateBoundingBox row + its cell index).  40 bytes.
struct Cand {
    float x1, y1, x2, y2, score;
    float r0, r1, r2, r3;
    int cell;
};

struct LevelGeom {
    double scale;
    int h, w;        // pyramid level size
    int oh, ow;      // PNet output map size
    int chunk;       // generic path: frames per step, so that one step's workspace stays under 2 GB (size_scratch)
};

struct CascadeBufs {   // device pointers into the arena, valid until the next call
    int n = 0, L = 0, H = 0, W = 0;
    LvLayout lay;                    // record slots per level (trl_capacity.h).  Both list capacities follow the content: a call that
    int capF = 0;                    // overflows one is re-run with larger lists.  capF: rows per frame of box[] / pts3
    int32_t* lvl_cnt = nullptr;      // [n][L]
    Cand* lvl_rec = nullptr;         // [n][S]
    int32_t* lvl_keep_cnt = nullptr; // [n][L]
    int32_t* lvl_keep_idx = nullptr; // [n][S]
    // the box lists behind stages 1-3, indexed by stage - 1
    int32_t* cnt[3] = {nullptr, nullptr, nullptr};   // [n]
    float* box[3] = {nullptr, nullptr, nullptr};     // [n][capF][5]
    float* pts3 = nullptr;                           // [n][capF][10]: stage 3's landmarks
    int32_t* off[2] = {nullptr, nullptr};            // [n+1] exclusive scans of cnt[0] / cnt[1]: the R-Net / O-Net batch
    int32_t* cbox = nullptr;     // [n*capF][8]: candidate t of the current stage = {frame, y0, x0, ih, iw, 0, 0, 0} (pad()'s crop window)
    int32_t* flags = nullptr;        // [TRL_NFLAGS]: the FLG_* words (trl_capacity.h)
    char* pq = nullptr;              // the fused PNet's confirm queue: pq_cap slots of TRL_DEFER_SLOT bytes (trl_capacity.h); none when 0
    int pq_cap = 0;
    char* spill = nullptr;           // global-memory workspace of the NMS spill tier (lists longer than the LDS tier)
    size_t spill_cap = 0;
    float* box0 = nullptr; float* prob0 = nullptr; int32_t* rect = nullptr; uint8_t* valid = nullptr; float* pts0 = nullptr;   // k_select's per-frame outputs where the call asks for none
};
// One MTCNN network, described once (the table trl_nets[] in trl_nets.hip): the layer walker, the front launcher, the cascade's
// stage loop and the loader's tensor check all read it.
struct NetLayer { const char* name; const char* prelu; int k, st, cout; };   // a valid k x k conv `name` (+ bias, + PReLU `prelu` or none) of
                                                                             // cout channels; name == null: a ceil-mode max pool k / st
enum { TRL_PNET_DEFER_DEFAULT = 1 };   // (the measurement behind the default)
// What only trl_debug_option, trl_debug_nms_tiers and trl_debug_pnet_run change (trl_hooks.hip): the product path reads these nine and
// never writes them
struct Options {
    int rnet_chunk = 49152, onet_chunk = 16384;   // R-/O-Net candidates per launch set (trl_cascade.hip; trl_debug_option shrinks them for tests)
    int tail_pool = 1;               // trl_debug_option "tail_pool": 0 = every R-/O-Net tail pool is its own launch (trl_run_net)
    int nms_small = 512, nms_full = 2048;   // LDS tiers of the sort + NMS kernels (candidates); longer lists take the spill tier
                                            // (trl_debug_nms_tiers lowers them so that small test inputs reach every tier)
    int pnet_screen = 1;             // trl_debug_option "pnet_screen": 0 = every M-tile takes the exact f32 path
    int pnet_defer = TRL_PNET_DEFER_DEFAULT;   // trl_debug_option "pnet_defer": 1 = confirmed conv3 M-tiles run in a second kernel where the launch can defer
    int pnet_run = 0;                // > 0: tiles per cursor fetch of the fused PNet launch (trl_debug_pnet_run); 0 = automatic
    int pyr_row_bands = 0;           // trl_debug_option "pyr_row_bands": > 0 forces the row bands of the streaming pyramid pass (tests)
};
struct NetDesc {
    const char* name;
    int side;                        // crop side (0: PNet takes any map)
    int nl; NetLayer layer[9];       // the last one is the merged heads conv, written straight into the caller's output
    int tail;                        // first layer behind the fused front kernel (trl_front.hip), whose pooled map is [P][P][C1]
    int P, C1;
    int nout;                        // output floats per item
    int Options::*chunk;             // the context's candidates-per-launch-set option of this net
};
enum { TRL_PNET = 0, TRL_RNET = 1, TRL_ONET = 2 };
extern const NetDesc trl_nets[3];
inline const NetDesc& trl_net_of(int net) { return trl_nets[net == 24 ? TRL_RNET : TRL_ONET]; }   // the API's net argument: 24 / 48
struct NetLayerW { const DevW* w = nullptr; const float* b = nullptr; const float* slope = nullptr; };   // a conv layer's device tensors
struct FnW { const DevW* w = nullptr; const float* scale = nullptr; const float* shift = nullptr; const float* bias = nullptr; };   // a FaceNet row's

// The 64-bit diagnostic words of trl_ctx::pnet_clk (device).  The fused PNet kernel and k_pnet_span write them (trl_pnet.hip);
// trl_destroy (the TRL_PNET_CLOCK report), collect_timings and trl_debug_pnet_span read them.
enum {
    CLK_START = 0, CLK_END = 1,      // first workgroup start / last workgroup end (wall clock) of the fused PNet launch in flight
    CLK_PHASE = 2,                   // DBG: [CLK_PHASE + 8 wave + k], shader clocks of wave 0..3 in phase / at barrier k = 0..7
    CLK_ROT = CLK_PHASE + 32,        // DBG: workgroup-tiles the phase clocks were summed over
    CLK_SPAN_SUM = 36, CLK_LAUNCHES = 37, CLK_LAST_SPAN = 38,   // summed spans and their count (trl_debug_pnet_span), the last launch's span
    CLK_SCREENED = 39, CLK_CONFIRMED = 40,   // DBG: conv3 M-tiles screened / confirmed
    CLK_QUEUED = 41,                 // M-tiles queued for the confirm pass
    CLK_PEND_SCREENED = 42, CLK_PEND_CONFIRMED = 43,   // DBG: a DEFER launch's own two counts until it is known to have fitted
    CLK_WORDS = 44
};
static_assert(CLK_LAUNCHES == CLK_SPAN_SUM + 1, "trl_debug_pnet_span reads and clears the two as one pair");

// State that only a test hook reads or writes (trl_hooks.hip, trl_redzone.hip); the product path feeds it where a hook asked for it
struct Hooks {
    int dbg_poison = -1;             // >= 0 after trl_debug_poison: byte written into every newly allocated workspace
    // trl_debug_redzone (trl_redzone.hip): while rz.guard != 0, `arena` and `scratch` carry that guard, dbg_poison is the fill byte and
    // every byte of the two that belongs to no block is checked against it at each rewind, before a grow and at the end of each call
    struct RedZone {
        size_t guard = 0; int byte = 0, saved_poison = -1;
        long long sweeps = 0, bytes = 0, nhits = 0;
        std::vector<trl_rz_hit> hits;                 // the first TRL_RZ_MAX_HITS
        unsigned long long* dev = nullptr; size_t dev_gaps = 0;   // device: the gap table of a sweep and its results
    } rz;
    // what the last build_pyramid chose per level (trl_debug_pyramid_plan): rows of TRL_PYR_PLAN_COLS ints; L = 0 after a refused call
    struct { int L = 0; int32_t row[16][TRL_PYR_PLAN_COLS] = {}; } pyr_plan;
    std::vector<trl_fn_plan_row> fn_plan;   // the conv launches of the last embedder call (trl_debug_facenet_plan)
    // the R-/O-Net tail conv launches of the last trl_debug_stage_net call, every chunk (trl_debug_mtcnn_plan); recorded only
    // while that hook runs (mt_plan_arm)
    std::vector<trl_fn_plan_row> mt_plan;
    bool mt_plan_arm = false;
    // trl_debug_facenet_capture: armed conv index (-1: off) and its three copied views (input / residual / output)
    int fn_cap_arm = -1;
    struct { void* p = nullptr; size_t cap = 0; int32_t dims[5] = {0, 0, 0, 0, 0}; } fn_cap[3];
};

struct trl_ctx {
    trl_config cfg;
    bool have_weights = false;
    char* wdev = nullptr;            // all weights, device
    size_t wbytes = 0;
    std::vector<DevW> wmat;          // the matrices in wdev, each the owner of its 16-bit copy where it has one; mt, fn and logits_w point into it
    // Resolved by trl_load_weights (trl_weights.hip), which refuses a blob that lacks or mis-shapes any of them: the tensors of every
    // layer of trl_nets[], of every row of FaceNet's table (trl_facenet.h), and the conv1 PReLU slope class of R-Net / O-Net
    // (trl_front.hip).  No path looks a tensor up by name: the name -> tensor directory ends with the load.
    NetLayerW mt[3][9];
    FnW fn[FN_ROWS];
    int front_mode[3] = {0, 0, 0};
    // InceptionResnetV1's classifier, when the blob holds one ("facenet.logits.w" [512][C] / ".b" [C], both or neither): always f32
    const DevW* logits_w = nullptr;
    const float* logits_b = nullptr;
    int num_classes = 0;
    Arena arena;                     // per-call persistent blocks (cascade lists)
    Arena scratch;                   // transient activations; only ever grown while empty (trl_scratch_begin)
    size_t arena_need = 0;           // the count of the last list layout (trl_debug_workspace)
    int fn_need_key[6] = {0}; size_t fn_need_bytes = 0;   // the last embedder dry run (trl_embed_need): what its walk branches on, its count
    Arena sims_tmp;                  // similarities when trl_drift_score is called with d_sims == NULL
    int32_t* h_pinned = nullptr;     // pinned host copy of the FLG_* words (trl_host_flags): 1,024 bytes
    CascadeBufs cb;
    LevelGeom lv[32];
    hipEvent_t ev_call0 = nullptr, ev_call1 = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pnet_ev;
    int pnet_ev_used = 0;
    float last_ms[4] = {0, 0, 0, 0};
    int pnet_mono1 = 0;              // conv1 PReLU slopes all >= 0
    int pnet_unit = 0;               // no PNet PReLU slope above 1 (negative ones allowed): prelu(v) == max(v, s v)
    float pnet_scrA = 0.f, pnet_scrB = 0.f;   // fp16 conv3 screen of the fused PNet: |d_screen - d_exact| <= A X + B (trl_pnet_prepare)
    float pnet_scrG[16] = {};        // the bound the kernel applies: sum over the cell's 3x3x16 inputs of pnet_scrG[channel] |x|, + B (sum of the 144 coefficients <= A)
    int pnet_screen_ok = 0;          // the conv3 weights fit fp16 (else the screen is off for this net)
    int32_t* pnet_cursor = nullptr;           // device: 8 per-XCD tile cursors of the fused PNet launch
    unsigned long long* pnet_clk = nullptr;   // device: the CLK_WORDS diagnostic words of the fused PNet launches (the CLK_* enum above)
    bool pnet_prof = false;                   // TRL_PNET_CLOCK: the DBG instantiation with per-phase wave clocks
    float pnet_kernel_ms = 0.f;      // its span in ms (collect_timings)
    Options opt;
    Hooks hook;
    // Optimistic capacities of the candidate lists, the spill pool and the R-Net / O-Net batches: launches and workspaces are sized
    // by them, and a call that overflows one is re-run with a larger value (trl_capacity.h)
    CascadeCaps caps;
    size_t scratch_after_cascade = 0;   // scratch bytes the rest of the call needs (crops + FaceNet): sized with the cascade's
    // the call in progress: queued by trl_detect_embed_begin / trl_detect_crop_begin and not yet finished by trl_detect_embed_end,
    // or a blocking trl_detect_embed / trl_detect_crop / trl_mtcnn_detect* between its enqueue and its wait (trl_api.hip)
    struct Pending {
        enum Kind { EMBED, CROP, DETECT };
        bool active = false; int attempt = 0; Kind kind = EMBED;
        const uint8_t* frames = nullptr; int n = 0, H = 0, W = 0;
        void* stream = nullptr;
        // EMBED / CROP: model.py:47-58 per frame, then the embeddings (EMBED) or the crops into faces_out (CROP)
        float* box = nullptr; float* prob = nullptr; int32_t* rect = nullptr; uint8_t* valid = nullptr; float* emb = nullptr;
        float* faces_out = nullptr;
        // DETECT: MTCNN.detect's boxes [n][max_faces][4], probs, points [n][max_faces][10] (nullable), counts; order as k_select's
        float* boxes = nullptr; float* probs = nullptr; float* points = nullptr; int32_t* counts = nullptr; int order = 0;
    } pend;
    uint32_t* pyr_tab = nullptr;     // pyramid bin-edge tables for the last (H, W)
    int pyr_tab_H = 0, pyr_tab_W = 0;
    // one-pass kernel for the finest levels (k_pyramid_fine): ownership table inside pyr_tab, source tile shape; nlev == 0: not usable for this shape
    struct { int nlev = 0, own0 = 0, band_cols = 0, strip_rows = 0, n_bands = 0, n_strips = 0; } pyr_fine;
};
inline int32_t* trl_host_flags(const trl_ctx* c) { return c->h_pinned; }   // the FLG_* words of the last attempt, copied behind its kernels

// The kernel a conv launcher picked (set by trl_launch_conv / trl_launch_fn_group / trl_launch_conv_bf16 as they choose, read by
// the FaceNet walker for trl_debug_facenet_plan): host bookkeeping only.
struct TrlConvChoice { int family = 0, bm = 0, bn = 0, bk = 0, pad = 0, nz = 1; };
extern thread_local TrlConvChoice g_trl_conv_choice;

// Optional device-wide ordering of the wide phases of different contexts (trl_api.hip; OFF by default, trl_debug_option
// "pnet_gate"): a fused PNet launch waits for the END of the most recent call queued on the device, whichever context queued it,
// so it runs alone (its HIP event pair is its duration) while the memory-bound pyramid kernels in front of it overlap the previous
// call's narrow R-/O-Net / embedder kernels.  Measured with two contexts in flight: 18.8 k frames/s and a clean clock, against
// 19.1 k with the launches left to the hardware queues and 18.6 k with one context (profiles/round4_pnet_gate_ab.txt).
int trl_gate_wait(trl_ctx* c, hipStream_t s);      // before the fused PNet launch
int trl_gate_record(trl_ctx* c, hipStream_t s);    // behind the last kernel of a call
extern int g_trl_pnet_gate;                        // trl_debug_option("pnet_gate"): 0 (default) / 1
int trl_ensure(trl_ctx* c, Arena& a, size_t bytes);   // grow (never while blocks of `a` are live)
// a call's first use of the scratch: empty, a new high-water mark, at least `bytes` (the count of the carve that follows); where one
// carve is the whole call (trl_carve_scratch), carve(X) over a counting arena, then over the scratch grown to that count
inline int trl_scratch_begin(trl_ctx* c, size_t bytes) { c->scratch.reset("scratch_begin"); c->scratch.high = 0; return trl_ensure(c, c->scratch, bytes); }
// the red-zone sweep at the end of an entry point that queued work on the arenas (trl_debug_redzone; nothing while it is off).
// site: the entry point's label in the report.  trl_rz_sweep (trl_redzone.hip) sweeps both workspaces, or only `one` (trl_ensure,
// before it frees a guarded workspace to grow it)
int trl_rz_sweep(trl_ctx* c, const char* site, Arena* one = nullptr);
inline int trl_rz_end(trl_ctx* c, const char* site) { return c->hook.rz.guard ? trl_rz_sweep(c, site) : TRL_OK; }
template <class F> int trl_carve_scratch(trl_ctx* c, F&& carve) {
    Arena X = Arena::counter(c->scratch.guard);
    TRL_CHECK(carve(X)); TRL_CHECK(trl_scratch_begin(c, X.high));
    return carve(c->scratch);
}
// A context holds at most one call in flight (trl_detect_embed_begin .. _end); anything else that touches its workspaces meanwhile
// would corrupt that call silently: TRL_ERR_STATE (and TRL_ERR_INVALID for a null context)
int trl_check_idle(trl_ctx* c);
// trl_check_idle, then what every entry point that takes frames requires: weights, 1..65535 frames of 12..16383 px per side, a
// 4-byte aligned buffer (trl_api.hip; the stage hooks of trl_hooks.hip apply the same)
int trl_check_call(trl_ctx* c, const void* frames, int n, int H, int W);
// c->fn_need_bytes = the scratch count of an embedder call on n faces of h x w -- with `crops`, of an EMBED call's crops and
// embedder on n frames (trl_api.hip; trl_debug_workspace reports it)
int trl_embed_need(trl_ctx* c, bool crops, int n, int h, int w);
// The way into a test hook that touches the device or the workspaces (trl_hooks.hip, trl_redzone.hip): no call in flight, and the
// context's device current before the hook synchronises, copies or launches
inline int trl_hook_device(trl_ctx* c) { TRL_CHECK(trl_check_idle(c)); TRL_HIP(hipSetDevice(c->cfg.device)); return TRL_OK; }
void trl_free_weights(trl_ctx* c);   // trl_weights.hip: the device weights and every 16-bit copy; the context then has none

// networks (trl_nets.hip).  Every walk takes its activations from X; over a counting X it still checks every shape (the walk of
// trl_load_weights).
// features: d_emb receives the 512 values in front of F.normalize (last_bn's output) instead of the embedding
int trl_run_facenet(trl_ctx* c, Arena& X, const float* d_faces, int n, int h, int w, const uint8_t* d_valid, float* d_emb, hipStream_t s,
                    bool features = false);
// Layers first .. last of net d over x (x.n items; the maps of layer `first`): d_out [x.n][oh][ow][d.nout].  With m_dev, x.n is the
// CAPACITY of the launch and the items that exist are clamp(*m_dev - m_base, 0, x.n) (device-sized, no host sync).  While
// c->hook.mt_plan_arm its conv launches are appended to c->hook.mt_plan ("rnet.conv2" .. "onet.heads").
int trl_run_net(trl_ctx* c, Arena& X, const NetDesc& d, int first, const Act& x, float* d_out, hipStream_t s, const int32_t* m_dev = nullptr,
                int m_base = 0);
// trl_load_weights, after the upload: himg is the staged host image, laid out like c->wdev (trl_host_of reads a device tensor's copy)
inline const float* trl_host_of(const trl_ctx* c, const char* himg, const float* dev) { return (const float*)(himg + ((const char*)dev - c->wdev)); }
int trl_front_slope_class(const float* h_slope, int n);
// the fused front kernel of R-Net / O-Net over records t0 .. t0 + nc - 1 of c->cb.cbox: pooled maps [nc][P][P][C1]
int trl_launch_front(trl_ctx* c, const NetDesc& d, const uint8_t* d_frames, int H, int W, const int32_t* d_total, int t0, int nc, float* d_pool, hipStream_t s);
// stage 2 / 3 network over `cap` candidate slots of c->cb.cbox, *d_total of them live (trl_cascade.hip): chunked front + tail
int trl_stage_net(trl_ctx* c, Arena& X, int net, const uint8_t* d_frames, int H, int W, const int32_t* d_total, int cap, float* d_out, hipStream_t s);

// cascade (trl_cascade.hip)
int trl_cascade_detect(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, hipStream_t s, int resume = 0);
int trl_cascade_finish(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_boxes, float* d_probs, float* d_points,
                       int32_t* d_counts, float* d_box0, float* d_prob0, int32_t* d_rect, uint8_t* d_valid, float* d_pts0, hipStream_t s,
                       int order = 0);   // order: 0 = area (select_largest=True), 1 = detection order
int trl_cascade_check(trl_ctx* c, int n, int* retry);   // after the call's stream synchronisation
int trl_cascade_lists(trl_ctx* c, int kind, int n, int H, int W, const int32_t* h_caps, int L, const int32_t* h_counts, const void* h_rows,
                      const float* h_logits, float* h_pts, float* d_boxes, float* d_probs, float* d_points, int32_t* d_counts, float* d_box0,
                      float* d_prob0, int32_t* d_rect, uint8_t* d_valid, hipStream_t s);   // trl_debug_lists
int trl_launch_area_level(const uint8_t* d_frames, int nf, int H, int W, int h, int w, float* d_level, hipStream_t s);
int trl_launch_heads_to_maps(const float* d_heads, int cells, float* d_prob, float* d_reg, hipStream_t s);
int trl_compute_levels(trl_ctx* c, int H, int W);
// the crops between the cascade and the embedder (trl_crops.hip)
int trl_launch_crop_resize80(const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid,
                             float* d_faces, hipStream_t s);
int trl_launch_crop_aligned(const uint8_t* d_frames, int n, int H, int W, const float* d_pts0, const uint8_t* d_valid, int S, bool rgb,
                            float* d_faces, hipStream_t s);
int trl_launch_crop_area_std(const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect, const uint8_t* d_valid, int S,
                             bool rgb, float* d_faces, hipStream_t s);
// stage 1 on the generic layer path, one level g of nf frames: the level materialised in X (reset first), *d_heads =
// [nf][oh][ow][6] behind it, PNet's layers over it
int trl_pnet_generic_level(trl_ctx* c, Arena& X, const uint8_t* d_frames, int nf, int H, int W, const LevelGeom& g, float** d_heads, hipStream_t s);
// fused PNet (trl_pnet.hip)
int trl_pnet_prepare(trl_ctx* c, const char* himg);   // slope classes and the screen bound, from the host image
bool trl_pnet_can_defer(const trl_ctx* c);             // this context's fused launches have a DEFER instantiation and the screen is on
long long trl_pnet_mtiles(const trl_ctx* c, int L, int n);   // conv3 M-tiles (2 output rows x 16 cells) of a fused launch over n frames
size_t trl_pnet_fused_bytes(trl_ctx* c, int n, int H, int W);
int trl_pnet_fused_all(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, hipEvent_t* ev, hipStream_t s);
int trl_pyramid_export(trl_ctx* c, const uint8_t* d_frame, int H, int W, int level, float* d_out, int* h, int* w, hipStream_t s);
int trl_pyramid_export_batch(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, float* d_out, long long* pyr_stride,
                             int32_t* h_levels, int max_levels, int* n_levels, hipStream_t s);

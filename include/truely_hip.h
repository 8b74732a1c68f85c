/*
 * truely_hip.h -- C ABI of libtruely_hip.so: the MI355X (gfx950) implementation of Truely's
 * per-frame visual hot path.
 *
 * The reference has no FFI / plugin layer: its boundary is the Python function
 *     run(video_path_one, video_path_two) -> int          (server/model.py:11-14)
 * imported by the FastAPI handlers (server/server.py:35,611,856), which internally makes two
 * library calls per sampled frame:
 *     boxes, _ = mtcnn.detect(frame)                       (server/model.py:47)
 *     emb = facenet_model(face_tensor)                     (server/model.py:59)
 * followed by the cosine-drift state machine (server/model.py:60-66,86-95).
 * Every entry point below names the reference lines it replaces.  Plain pointers and sizes only:
 * no torch types.  All `d_*` pointers are DEVICE pointers owned by the caller (e.g. the
 * data_ptr() of torch-ROCm tensors); `stream` is a hipStream_t passed as void*.
 *
 * Error convention: every function returns TRL_OK (0) or a negative trl_status; a thread-local
 * message is available from trl_last_error().  (model.run() itself maps failures to the
 * reference's `return 0`, server/model.py:20-34,83-88.)
 *
 * Threading: a context is bound to one device and one in-flight call; use one context per GPU /
 * rank.  Calls on distinct contexts are independent.
 */
#ifndef TRUELY_HIP_H
#define TRUELY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRL_ABI_VERSION 7

typedef enum {
    TRL_OK = 0,
    TRL_ERR_INVALID = -1,   /* bad argument / shape */
    TRL_ERR_HIP = -2,       /* HIP runtime error (message has hipGetErrorString) */
    TRL_ERR_WEIGHTS = -3,   /* blob malformed or tensor missing */
    TRL_ERR_CAPACITY = -4,  /* (ABI <= 6: a candidate list exceeded its configured capacity.  Since ABI 7 no input can
                             *  produce it: lists grow to what the content needs, as detect_face() has no limit;
                             *  trl_jpeg_header returns it for a buffer that is too small) */
    TRL_ERR_STATE = -5      /* call order (e.g. no weights loaded).  A re-run bound also reports it ("candidate capacities
                             *  did not converge"), which no input reaches: each re-run raises the one capacity that
                             *  overflowed to the measured need, and there are five capacities (trl_api.hip) */
} trl_status;

typedef struct trl_ctx trl_ctx;

/* MTCNN() constructor arguments that affect detect() (facenet_pytorch MTCNN.__init__ defaults,
 * as instantiated at server/model.py:18) plus capacities of the device-side candidate lists. */
typedef struct {
    int    device;          /* HIP device ordinal */
    int    min_face_size;   /* 20 */
    float  thr0, thr1, thr2;/* 0.6 0.7 0.7 */
    double factor;          /* 0.709 */
    int    cap_level;       /* START capacity of the per-(frame, pyramid level) candidate lists   [2048] */
    int    cap_frame;       /* START capacity of the per-frame box lists of stages 1-3           [2048]
                             * Lists are never longer than the geometry allows (a level has oh x ow cells) and grow with
                             * the content: a call whose frames need more is re-run internally with larger lists (and
                             * sorted / suppressed through a global-memory tier beyond the LDS tier), never refused. */
    int    max_faces;       /* max boxes returned per frame by trl_mtcnn_detect          [64]   */
    int    pnet_mode;       /* 0 = fused PNet kernel, 1 = generic layer path (validation) */
    int    embed_mode;      /* 0 = reference: 80x80 INTER_LINEAR crop, BGR, /255 (model.py:41,57-58)  [default]
                             * 1 = SURVEY 8(f)-4 native mode: facenet-pytorch extract_face (160x160 area
                             *     resample, .byte(), (x-127.5)/128), channel order kept; 2 = same, BGR->RGB
                             * 3 = 8(f)-4 "landmark-aligned": 160x160 similarity warp of the largest face from its five
                             *     O-Net landmarks to the scaled 112x112 five-point template (bilinear, replicated
                             *     borders), (x-127.5)/128, RGB -- this project's definition, oracle: orc_crop_aligned */
    int    embed_precision; /* 0 = f32, bit-exact with the oracle                                        [default]
                             * 1 = bf16 activations/weights on the bf16 matrix cores for InceptionResnetV1 only
                             *     (BASELINE configs[2]); detector, crops and valid mask stay f32-exact; embeddings
                             *     agree with the f32 path to ~1e-2 (cosine > 0.999), see tests/test_gpu_api.py
                             * 2 = the same on fp16 (BASELINE configs[4]): three more mantissa bits, cosine > 0.99999 */
} trl_config;

int  trl_abi_version(void);
const char* trl_last_error(void);
int  trl_default_config(trl_config* cfg);

/* Replaces the per-call model construction at server/model.py:18-19: create once, load the
 * packed weights (TRLW0001 blob from weights.pack_state_dicts) once, reuse for every clip. */
int  trl_create(const trl_config* cfg, trl_ctx** out);
int  trl_destroy(trl_ctx* ctx);
/* trl_load_weights checks every tensor the four networks use -- present, and of the shape its layer needs -- and returns
 * TRL_ERR_WEIGHTS, naming the tensor, for a blob that falls short: no later call can miss one.  A context whose load was
 * refused has no weights. */
int  trl_load_weights(trl_ctx* ctx, const void* host_blob, size_t nbytes);

/* server/model.py:47  `boxes, probs = mtcnn.detect(frame)` for a batch of n frames.
 *   d_frames : u8  [n][H][W][3]  BGR as cv2.VideoCapture.read() yields (model.py:43).  The ADDRESS must be a multiple of 4,
 *              here and in every call that takes a frame batch for the cascade or one of its stages (a device allocation's
 *              start always is; a view `buf[k:]`, or `frames[1:]` of a batch whose frames are not a multiple of 4 bytes, need
 *              not be): the pyramid and front kernels turn d_frames into dword and 16-byte loads.  Any other address:
 *              TRL_ERR_INVALID, nothing launched.  The frame size itself is free (frames inside a batch sit at any byte
 *              phase).  A load may cover the whole dword that holds the batch's last byte, i.e. up to 3 bytes past it, which
 *              an aligned device allocation always grants; those bytes never reach a result.
 *   d_boxes  : f32 [n][max_faces][4]   x1,y1,x2,y2, largest area first (select_largest=True)
 *   d_probs  : f32 [n][max_faces]
 *   d_counts : i32 [n]                 number of faces (0 <=> detect() returned None) */
int  trl_mtcnn_detect(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                      float* d_boxes, float* d_probs, int32_t* d_counts, void* stream);

/* `mtcnn.detect(frame, landmarks=True)`: the same call returning the 5 facial landmarks O-Net predicts as well.  The
 * reference discards them (`boxes, _ = mtcnn.detect(frame)`, server/model.py:47); facenet-pytorch computes them on every
 * call (detect_face.py stage 3), so they are exported for callers that align faces.
 *   d_points : f32 [n][max_faces][10]  x0..x4, y0..y4 of each face, same order as d_boxes */
int  trl_mtcnn_detect_landmarks(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                                float* d_boxes, float* d_probs, float* d_points, int32_t* d_counts, void* stream);

/* `mtcnn.detect(frame, landmarks=...)` with the box order chosen: order 0 = largest area first (select_largest=True, what the
 * two calls above return); order 1 = detect_face's own order (select_largest=False): the pick order of the final NMS, i.e.
 * descending score -- the stage-3 rows as trl_debug_stage_boxes(3) shows them, truncated to max_faces.  d_points may be NULL.
 * (ABI v7, additive) */
int  trl_mtcnn_detect_ordered(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W, int order,
                              float* d_boxes, float* d_probs, float* d_points, int32_t* d_counts, void* stream);

/* facenet-pytorch 2.6.0 MTCNN.select_boxes on detect's output (d_boxes [n][max_faces][4], d_probs [n][max_faces], d_counts [n],
 * in the order detect returned them): d_pick [n] receives the slot of the selected box of each frame, or -1 (no face, or no box
 * over the threshold).  method 0 = 'largest' (key (x2-x1)*(y2-y1) in f32), 1 = 'probability', 2 = 'largest_over_threshold'
 * (boxes with prob > threshold (f32), then the area key), 3 = 'center_weighted_size' (f64 area - center_weight * squared
 * distance of the f32 box centre from (W/2, H/2)).  Ties go to the LAST tied box in detect's order (np.argsort(key)[::-1] of a
 * stable sort).  No host synchronisation.  (ABI v7, additive) */
int  trl_select_faces(trl_ctx* ctx, int n, const float* d_boxes, const float* d_probs, const int32_t* d_counts, int H, int W,
                      int method, float threshold, double center_weight, int32_t* d_pick, void* stream);

/* facenet-pytorch 2.6.0 extract_face for m boxes of the n u8 frames [n][H][W][3]: row r crops frame d_frame_of[r] around
 * d_boxes [m][4] (x1,y1,x2,y2 f32) with `margin` pixels of the S x S output (margin*(x2-x1)/(S-margin) in f64, clamp, int()),
 * resamples the crop to S x S as crop_resize does for the input kind -- resample 0 = torch.Tensor (imresample, area, .byte()),
 * 1 = PIL image (Image.BILINEAR, Pillow's two 8-bit passes), 2 = numpy array (cv2.INTER_AREA) -- keeping the frame's channel
 * order, and writes d_out [m][S][S][3] f32 (NHWC, what trl_facenet_embed reads): (v-127.5)/128 with post_process, else v.
 * d_status [m] (may be NULL): 1 = face written, 0 = d_frame_of[r] < 0 (zeros written), -1 = empty crop (zeros written;
 * facenet-pytorch raises).  1 <= S <= 1024, 0 <= margin < S.  No host synchronisation.  (ABI v7, additive) */
int  trl_extract_faces(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W, const int32_t* d_frame_of, const float* d_boxes,
                       int m, int S, int margin, int resample, int post_process, float* d_out, int32_t* d_status, void* stream);

/* server/model.py:59  `facenet_model(face_tensor)`:  InceptionResnetV1(...).eval() forward.
 *   d_faces : f32 [n][h][w][3] NHWC, already scaled as model.py:58 does (to_tensor: /255)
 *   d_emb   : f32 [n][512], L2-normalised */
int  trl_facenet_embed(trl_ctx* ctx, const float* d_faces, int n, int h, int w, float* d_emb, void* stream);

/* InceptionResnetV1(classify=True): the checkpoint's `logits` layer (vggface2: 512 -> 8631 classes, casia-webface: 10575), when the
 * blob holds it ("facenet.logits.w" [512][C] and "facenet.logits.b" [C], both or neither, 1 <= C <= 65535: trl_load_weights
 * refuses anything else).  (ABI v7, additive)
 * trl_facenet_num_classes: *C = classes of the loaded checkpoint's logits layer; *C = 0 when the blob has none.
 * trl_facenet_features: InceptionResnetV1 up to and including last_bn -- what F.normalize / logits read.  d_faces as
 *   trl_facenet_embed; d_valid nullable (zero rows where !valid, as trl_facenet_embed_masked); d_feat f32 [n][512].
 * trl_facenet_logits: logits = feat @ W + b for n rows: d_logits f32, row r at d_logits + r*ld, ld >= C; columns C..ld-1 are
 *   not written.  logit[r][c] is the f32 chain acc = b[c]; k = 0..511 ascending: acc = fmaf(feat[r][k], W[k][c], acc), whatever
 *   n (always f32, also under embed_precision 1 / 2).  No host synchronisation.
 * Refusals as trl_facenet_embed's: a context with a call in flight or without weights TRL_ERR_STATE; a blob without logits
 * TRL_ERR_WEIGHTS ("the loaded checkpoint has no logits layer"); null pointers, n < 1, ld < C TRL_ERR_INVALID, nothing launched. */
int  trl_facenet_num_classes(trl_ctx* ctx, int* C);
int  trl_facenet_features(trl_ctx* ctx, const float* d_faces, const uint8_t* d_valid, int n, int h, int w, float* d_feat, void* stream);
int  trl_facenet_logits(trl_ctx* ctx, const float* d_feat, int n, float* d_logits, long long ld, void* stream);

/* server/model.py:47-59 fused for a batch of sampled frames: detect, take boxes[0], int-cast +
 * clamp (model.py:49-53), crop, cv2.resize(...,(80,80)) (model.py:55-57), to_tensor (model.py:58),
 * embed (model.py:59).
 *   d_box   : f32 [n][4]   boxes[0] (zeros if none)
 *   d_prob  : f32 [n]
 *   d_rect  : i32 [n][4]   clamped integer crop rectangle x0,y0,x1,y1
 *   d_valid : u8  [n]      1 iff an embedding was produced for the frame (model.py:48,54,56)
 *   d_emb   : f32 [n][512] (zero rows where !valid) */
int  trl_detect_embed(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                      float* d_box, float* d_prob, int32_t* d_rect, uint8_t* d_valid, float* d_emb,
                      void* stream);

/* The two halves of trl_detect_embed, for callers that embed the faces of SEVERAL frame batches in one embedder call
 * (the embedder's 100 small launches amortise over more faces: 2.22 ms per 256 faces alone, 1.77 ms at 768 per call).
 * trl_detect_crop = model.py:47-58: d_faces [n][S][S][3] f32 receives the crops (S = 80, or 160 in the native embed modes; zero
 * where !valid).  trl_facenet_embed_masked = model.py:59 with zero rows where !valid.  Results are bit-identical to
 * trl_detect_embed whatever the grouping. */
int  trl_detect_crop(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                     float* d_box, float* d_prob, int32_t* d_rect, uint8_t* d_valid, float* d_faces, void* stream);
int  trl_facenet_embed_masked(trl_ctx* ctx, const float* d_faces, const uint8_t* d_valid, int n, int h, int w, float* d_emb, void* stream);

/* The same two calls split into "queue" and "finish", so ONE host thread can keep several contexts (one per batch in flight, or
 * one per GPU) busy without a thread per context: *_begin validates, queues every kernel of the call on `stream` and returns
 * without synchronising; trl_detect_embed_end is the call's one host synchronisation, checks the candidate capacities and -- rarely,
 * when a candidate list or an optimistic R-/O-Net batch capacity was too small for the content -- re-runs the call with larger
 * ones before returning.  Outputs are valid after _end.  A
 * context holds at most one call in flight (TRL_ERR_STATE from every entry point that would touch its workspaces meanwhile); the buffers must stay alive until _end returns.
 * server/model.py:42-59 is strictly one frame at a time; this is the batched, overlapped form of the same two library calls. */
int  trl_detect_embed_begin(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                            float* d_box, float* d_prob, int32_t* d_rect, uint8_t* d_valid, float* d_emb, void* stream);
int  trl_detect_crop_begin(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                           float* d_box, float* d_prob, int32_t* d_rect, uint8_t* d_valid, float* d_faces, void* stream);
int  trl_detect_embed_end(trl_ctx* ctx);

/* server/model.py:60-66,70,75,86-95: cosine similarity against the last embedded frame, the
 * run-length counter, and the 0..100 score.  n = number of sampled frames (in time order),
 * frame_count = frames decoded, fps as int(cap.get(CAP_PROP_FPS)) (model.py:28).
 *   d_sims   : f32 [n]  (2.0 where no comparison happened)        may be NULL
 *              The value 2.0 marks "no comparison".  A NaN or infinite similarity (a zero or non-finite embedding, a norm
 *              that underflows) is a comparison, and it resets the run unless it is -inf (model.py:62-65).
 *   d_flags  : u8  [n]  1 where the frame was counted "AI detected" (model.py:66)  may be NULL
 *   d_result : i32 [4]  {score, final run length, hits, total sampled frames} */
int  trl_drift_score(trl_ctx* ctx, const float* d_emb, const uint8_t* d_valid, int n,
                     long long frame_count, int fps, float* d_sims, uint8_t* d_flags,
                     int32_t* d_result, void* stream);

/* The same state machine continued across the WINDOWS of one clip, for callers that stream (model.run): d_state
 * (TRL_DRIFT_STATE_BYTES device bytes, zero-filled before the clip's first window) carries what model.py's loop variables
 * `previous_embedding`, `consecutive_count`, `ai_detected_frames` hold between two sampled frames (model.py:60-75).  The n
 * embeddings of the window are compared in order, the first one with the carried embedding; d_sims / d_flags (may be NULL)
 * cover the window; d_result as above, computed for `frame_count` = frames decoded so far (n = 0 with the clip's final count
 * gives the final score).  Windows of any sizes give the similarities, flags and score of one trl_drift_score over the clip. (ABI v7) */
#define TRL_DRIFT_STATE_BYTES 2064
int  trl_drift_update(trl_ctx* ctx, void* d_state, const float* d_emb, const uint8_t* d_valid, int n,
                      long long frame_count, int fps, float* d_sims, uint8_t* d_flags, int32_t* d_result, void* stream);

/* SURVEY 8(f)-1, device-side ingest in place of the CPU decode + sampling at server/model.py:43,46:
 * d_nv12 holds n_in decoder-output frames (NV12: H*W luma bytes, then H/2 rows of interleaved U,V);
 * frames 0, step, 2*step, ... are converted to u8 BGR [n_out][H][W][3] (OpenCV's integer BT.601
 * limited-range arithmetic) ready for trl_detect_embed.  step = max(1, int(fps / 7)) (model.py:40).
 * *n_out = ceil(n_in / step).  H even and >= 2, W % 4 == 0 and >= 4, both buffers 4-byte aligned, step >= 1, n_in >= 0:
 * TRL_ERR_INVALID otherwise, with nothing written.  n_in = 0 is an empty batch: TRL_OK, *n_out = 0, and the two
 * buffers are not looked at (they may be NULL, as the pointer of a 0-frame tensor is). */
int  trl_ingest_nv12(trl_ctx* ctx, const uint8_t* d_nv12, int n_in, int H, int W, int step,
                     uint8_t* d_bgr, int* n_out, void* stream);
/* the same for PLANAR 4:2:0 (I420: Y plane, U plane, V plane -- YUV4MPEG2 files, software decoders): no host-side repacking (ABI v7) */
int  trl_ingest_i420(trl_ctx* ctx, const uint8_t* d_i420, int n_in, int H, int W, int step,
                     uint8_t* d_bgr, int* n_out, void* stream);

/* ---- inspection hooks used by the parity tests (stage-by-stage vs the oracle) ------------- */
/* Boxes of one frame after cascade stage 1/2/3 of the LAST trl_mtcnn_detect / trl_detect_embed
 * call (host output, rows of 5: x1,y1,x2,y2,score).  Returns the count in *n_out. */
int  trl_debug_stage_boxes(trl_ctx* ctx, int stage, int frame, float* h_boxes, int max_rows, int* n_out);
/* Per-level PNet candidate / kept counts of one frame (host output, up to 32 levels each). */
int  trl_debug_level_counts(trl_ctx* ctx, int frame, int32_t* h_cand, int32_t* h_keep, int* n_levels);
/* Candidate records of one (frame, pyramid level) of the last call, as the PNet kernel appended them (arbitrary order):
 * rows of 40 bytes {x1,y1,x2,y2,score,r0,r1,r2,r3 : f32; cell : i32}, cell = y*ow + x of the PNet output map.  With
 * thr0 = 0 every cell is a candidate, so this reads the fused kernel's own probability / regression maps. */
int  trl_debug_level_cands(trl_ctx* ctx, int frame, int level, void* h_rows, int max_rows, int* n_out);
/* The per-level NMS picks (detect_face.py stage 1: batched_nms 0.5 per scale) of one (frame, level) of the last call: indices into
 * the rows trl_debug_level_cands returns (append order), in pick order.  With it a test can check the keep set of a list of ANY
 * length against the definition of greedy NMS (a box is kept iff no kept box of higher priority overlaps it by more than the
 * threshold) without an O(n^2) reference run. (ABI v7) */
int  trl_debug_level_keep(trl_ctx* ctx, int frame, int level, int32_t* h_idx, int max_rows, int* n_out);
/* test hook: LDS tiers of the sort + NMS kernels in candidates per list (0 keeps a value; multiples of 4 in [16, 3072]; defaults
 * 512 / 2048).  Lists longer than `full_tier` are sorted and suppressed in global memory (the spill tier); lowering the tiers
 * lets small inputs reach it.  Results never depend on the tiers. (ABI v7) */
int  trl_debug_nms_tiers(trl_ctx* ctx, int small_tier, int full_tier);
/* candidate-list statistics of the last call: h_out8 = {attempts, lists that took the spill tier, spill bytes used, spill bytes
 * available, rows per frame of the stage lists, record slots per frame over all levels, largest per-level candidate count,
 * largest per-frame stage-1 total} (ABI v7) */
int  trl_debug_list_stats(trl_ctx* ctx, long long* h_out8);
/* test hooks that used to be environment variables (the library reads none; experiment switches exist only in a `make TUNING=1`
 * build): key "rnet_chunk" / "onet_chunk" = candidates per R-/O-Net launch set of this context (>= 16: small inputs then run
 * the multi-chunk path); "no_fnconv" (process-wide, ctx may be NULL) = FaceNet's small maps through the generic conv kernels,
 * value 0 restores the default; "pnet_gate" (process-wide, default 0) = 1: a fused PNet launch waits for the end of the previous
 * call queued on its device by ANY context, so that with several contexts in flight it runs alone (a timing aid: the HIP event
 * pair of trl_debug_timings is then the launch's duration).  Results never depend on them. (ABI v7) */
int  trl_debug_option(trl_ctx* ctx, const char* key, int value);
/* test hook: the fused PNet screens conv3 of every 32-cell M-tile on the fp16 matrix cores and recomputes it with the exact f32
 * chain only where some cell's screened logit difference d satisfies d + A X + B >= the prefilter bound (X: the cell's largest
 * |conv2 activation|).  Returns A, B (computed at weight load) and whether the screen is on (*on = 0: the conv3 weights do not fit
 * fp16, or trl_debug_option(ctx, "pnet_screen", 0) switched it off; every M-tile then takes the exact path).  Results are the
 * same either way. (ABI v7) */
int  trl_debug_pnet_screen_bound(trl_ctx* ctx, float* A, float* B, int* on);
/* test hook: the bound the screen applies is per input, E = sum over the cell's 3 x 3 x 16 conv2 inputs of g[channel] |x| + B, with
 * g[channel] the largest of that channel's nine per-tap coefficients of A (so 9 * sum(g) >= A, and E <= A X + B up to that slack).
 * h_g16 receives the sixteen g (infinities where the conv3 weights do not fit fp16). */
int  trl_debug_pnet_screen_weights(trl_ctx* ctx, float* h_g16);
/* test hook: the R-/O-Net launches are sized by optimistic per-frame candidate capacities; set them (<= 0 keeps a value) and read
 * how many attempts the last call took (a too-small capacity makes the call re-run itself with a larger one) */
int  trl_debug_batch_capacity(trl_ctx* ctx, float t2_per_frame, float t3_per_frame, int* last_attempts);
/* test hook: level `level` of one frame's image pyramid as the fused PNet kernel reads it; d_out holds h*w*3 floats
 * (capacity: at least (int(H*m+1))*(int(W*m+1))*3 with m = 12/min_face_size) */
int  trl_debug_pyramid_level(trl_ctx* ctx, const uint8_t* d_frame, int H, int W, int level, float* d_out, int* h, int* w, void* stream);
/* test hook: the image pyramid of an n-frame device batch, built by the same pyramid pass trl_detect_embed's fused PNet makes.
 * d_out receives the raw workspace: n x *pyr_stride pixels of 3 floats (frame f, level l at f * pyr_stride + pix0), each level's
 * padding up to pix_pad pixels included.  d_out == NULL: layout only, nothing is launched.  h_levels receives {pix0, h, w, pix_pad}
 * per level (room for max_levels levels), *n_levels the level count.  More than 16 levels: TRL_ERR_INVALID. (ABI v7) */
int  trl_debug_pyramid_batch(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W, float* d_out, long long* pyr_stride,
                             int32_t* h_levels, int max_levels, int* n_levels, void* stream);
/* test hook: what the last pyramid pass of this context chose for each level (host bookkeeping of the pass; *n_levels = 0 when it
 * was refused).  Rows of TRL_PYR_PLAN_COLS ints: {kernel (TRL_PYR_* below), row_bands, col_bands, cols_per_band, frames per
 * launch, khmax (tallest bin, source rows)}; the band fields are 0 for the per-level and fine-level kernels, frames per launch
 * is n for the one-pass kernels and the frame chunk for the per-level ones. (ABI v7) */
#define TRL_PYR_PLAN_COLS 6
enum { TRL_PYR_FINE = 1, TRL_PYR_S4 = 2, TRL_PYR_S8 = 3, TRL_PYR_SW4 = 4, TRL_PYR_SW8 = 5,
       TRL_PYR_L0_3 = 6, TRL_PYR_L0_4 = 7, TRL_PYR_L0_5 = 8, TRL_PYR_L1 = 9, TRL_PYR_L2 = 10 };
int  trl_debug_pyramid_plan(trl_ctx* ctx, int32_t* h_rows, int max_levels, int* n_levels);
/* test hook: the conv launches of the context's last embedder call, in walk order: one row per conv, recorded host-side where the
 * launcher picks the kernel (no device work, no influence on the choice).  family = TRL_FNK_* below; bm / bn / bk = the workgroup
 * tile and K chunk of the instantiation; pad = its PAD template argument (0 for families without one); nz = convs sharing the launch
 * (grouped small-map launches); precision = 0 f32, 1 bf16, 2 fp16; has_res = the conv adds a residual.  *n_rows = the call's conv
 * count (rows past max_rows are not written). (ABI v7) */
enum { TRL_FNK_FN_CONV = 1, TRL_FNK_FN_SPLIT4 = 2, TRL_FNK_CONV_TAP = 3, TRL_FNK_IGEMM_VEC = 4, TRL_FNK_IGEMM_SCALAR = 5,
       TRL_FNK_SPLITK4 = 6, TRL_FNK_SPLITK4_TAP = 7, TRL_FNK_TAP48 = 8, TRL_FNK_BF16 = 9 };
typedef struct {
    int32_t conv, family, bm, bn, bk, pad, nz, m, cout, k, precision, has_res;
    char layer[48];
} trl_fn_plan_row;
int  trl_debug_facenet_plan(trl_ctx* ctx, trl_fn_plan_row* h_rows, int max_rows, int* n_rows);
/* test hook: arm conv `conv_index` (the walk order of trl_debug_facenet_plan; -1 disarms).  The next embedder call on ctx copies
 * that conv's input view, residual view (if any) and output view right behind its launch, on the call's stream, into buffers of
 * the context: dense NHWC in the activation's element type (f32, or 16-bit in reduced-precision mode).  The call disarms it.
 * trl_debug_facenet_capture_read: view 0 input / 1 residual / 2 output; dims = {n, h, w, c, bytes per element} (c = 0: no such
 * view); h_dst may be NULL to query the dims, else it receives n*h*w*c elements if they fit max_bytes (TRL_ERR_INVALID if not). */
int  trl_debug_facenet_capture(trl_ctx* ctx, int conv_index);
int  trl_debug_facenet_capture_read(trl_ctx* ctx, int view, void* h_dst, size_t max_bytes, int32_t* dims5);
/* test hook: fill the activation workspaces with a byte pattern (0xFF -> NaNs) before the next call */
int  trl_debug_poison(trl_ctx* ctx, int byte);
/* PNet on one pyramid level of frame 0: face-prob map and regression map (device outputs). */
int  trl_debug_pnet_level(trl_ctx* ctx, const uint8_t* d_frame, int H, int W, int level,
                          float* d_prob, float* d_reg, int* oh, int* ow, void* stream);
/* R-Net / O-Net on prepared crops: d_crops f32 [n][S][S][3]; d_out f32 [n][6] / [n][16]
 * = {logit0, logit1, reg[4], (landmarks[10])}. */
int  trl_debug_rnet(trl_ctx* ctx, const float* d_crops, int n, float* d_out, void* stream);
int  trl_debug_onet(trl_ctx* ctx, const float* d_crops, int n, float* d_out, void* stream);
/* The production stage-2 / stage-3 network path (fused front kernel + layer tail) on caller-chosen boxes of ONE frame:
 * h_boxes = nb host rows x1,y1,x2,y2 (as after rerec); net = 24 (R-Net, d_out [nb][6]) or 48 (O-Net, d_out [nb][16]). */
int  trl_debug_front_net(trl_ctx* ctx, const uint8_t* d_frame, int H, int W, const float* h_boxes, int nb, int net,
                         float* d_out, void* stream);
/* The production stage-2 / stage-3 loop (chunked front kernel + layer tail, as the cascade runs it) at a caller-chosen launch
 * capacity: h_recs = nb host rows (frame, x1, y1, x2, y2) over nf frames, cropped by pad() as the cascade's records are; the device
 * total is nb, and capacity (>= 0, below or above nb) sizes every launch.  Chunks follow trl_debug_option "rnet_chunk" /
 * "onet_chunk".  d_out: [capacity][6] (net = 24) or [capacity][16] (net = 48), device; rows past nb are not defined. (ABI v7) */
int  trl_debug_stage_net(trl_ctx* ctx, const uint8_t* d_frames, int nf, int H, int W, const float* h_recs, int nb, int net,
                         int capacity, float* d_out, void* stream);
/* k_mtcnn_front (crop, area resample, conv1, PReLU, pool) ALONE, on windows the caller gives directly: h_win = nb host rows of
 * int32 {frame, y0, x0, ih, iw}, the record the cascade's k_build_map writes after pad() -- rows y0 .. y0+ih-1 and columns
 * x0 .. x0+iw-1 of that frame.  Each row is checked (0 <= frame < nf, ih, iw >= 1, the window inside the frame: TRL_ERR_INVALID
 * otherwise, nothing launched).  The device total is nb; the launch covers `capacity` slots (one chunk at t0 = 0, as the first
 * chunk of trl_debug_stage_net), and record slots past nb hold that hook's poison.  d_pool: [capacity][11][11][28] (net = 24) or
 * [capacity][23][23][32] (net = 48), device, written directly by the kernel: maps past nb are not touched.  No tail runs.
 * (ABI v7, additive) */
int  trl_debug_front(trl_ctx* ctx, const uint8_t* d_frames, int nf, int H, int W, const int32_t* h_win, int nb, int net,
                     int capacity, float* d_pool, void* stream);
/* The cascade's list kernels on lists the caller builds, launched by the cascade's own host code (LDS tiers of
 * trl_debug_nms_tiers, workgroup sizes, spill pool, overflow flags: trl_debug_list_stats).  h_caps: n_levels level capacities,
 * then the per-frame capacity (multiples of 4).  kind 1: h_rows = 40-byte candidate records {x1, y1, x2, y2, score, r0..r3, cell}
 * of every (frame, level) in append order, frame-major, h_counts [n][n_levels] -> per-level NMS, cross-level NMS, regression
 * (read with trl_debug_level_keep, trl_debug_stage_boxes stage 1).  kind 2: h_rows = stage-1 rows {x1, y1, x2, y2, score} of every
 * frame, h_counts [n], h_logits = R-Net outputs [total][6] -> stage-2 rows (trl_debug_stage_boxes stage 2).  kind 3: stage-2 rows
 * and O-Net outputs [total][16] -> stage-3 rows (stage 3), their landmarks into h_pts [n][capacity][10] (nullable), and the
 * detect() selection into d_boxes [n][max_faces][4], d_probs, d_points [n][max_faces][10], d_counts, d_box0 [n][4], d_prob0,
 * d_rect [n][4], d_valid [n] (device).  Slots past the counts hold the trl_debug_poison byte.  A list the capacities cannot hold:
 * TRL_ERR_CAPACITY. (ABI v7) */
int  trl_debug_lists(trl_ctx* ctx, int kind, int n, int H, int W, const int32_t* h_caps, int n_levels, const int32_t* h_counts,
                     const void* h_rows, const float* h_logits, float* h_pts, float* d_boxes, float* d_probs, float* d_points,
                     int32_t* d_counts, float* d_box0, float* d_prob0, int32_t* d_rect, uint8_t* d_valid, void* stream);
/* The tail conv launches of the last trl_debug_stage_net call, chunk after chunk, in the rows of
 * trl_debug_facenet_plan: layer = "rnet.conv2", ..., "onet.heads", conv = row index.  Other calls do not record. (ABI v7) */
int  trl_debug_mtcnn_plan(trl_ctx* ctx, trl_fn_plan_row* h_rows, int max_rows, int* n_rows);
/* The three face-crop kernels alone, on caller-chosen rows.  Common to all three: frames u8 [n][H][W][3] with H, W >= 1 (the
 * cascade's 12 px minimum does not apply), d_valid u8 [n]; a row with valid = 0 gets an all-zero face and its rectangle / points
 * are never read.  PRECONDITION of a row with valid = 1 (the cascade's selection kernel guarantees it; the hooks do not check
 * device memory): 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H.  Nothing outside the rectangle is read.
 * trl_debug_crop_resize = model.py:55-58: d_rect i32 [n][4] = x0,y0,x1,y1 -> f32 [n][80][80][3] in [0,1].  Its kernel takes the
 * frame index from grid x, so any n > 0 is legal; the other two take it from grid y: 1 <= n <= 65535, the bound every public
 * entry point already applies to a frame batch. */
int  trl_debug_crop_resize(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W,
                           const int32_t* d_rect, const uint8_t* d_valid, float* d_faces, void* stream);
/* embed_mode 3's crop alone: d_pts [n][10] = x0..x4, y0..y4 per frame -> f32 [n][S][S][3], 1 <= S <= 4096 (any values, NaN
 * included: samples outside the frame replicate its border) */
int  trl_debug_crop_aligned(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W, const float* d_pts,
                            const uint8_t* d_valid, int S, int rgb, float* d_faces, void* stream);
/* embed_mode 1 / 2's crop alone (extract_face for tensor input: area pooling to S x S, .byte(), (v - 127.5) / 128; rgb != 0
 * reverses the channels): d_rect as for trl_debug_crop_resize -> f32 [n][S][S][3], 1 <= S <= 4096. (ABI v7) */
int  trl_debug_crop_area(trl_ctx* ctx, const uint8_t* d_frames, int n, int H, int W, const int32_t* d_rect,
                         const uint8_t* d_valid, int S, int rgb, float* d_faces, void* stream);
/* Time (ms, HIP events on the call's stream) of the last trl_detect_embed / trl_detect_crop / trl_mtcnn_detect* call:
 * out[0] = PNet kernel (fused: the one persistent launch; generic: sum over levels),
 * out[1] = whole call, every attempt of a re-run call included (before this library version trl_mtcnn_detect* timed only the
 * last attempt), out[2] = number of PNet launches timed, out[3] = pyramid kernel. */
int  trl_debug_timings(trl_ctx* ctx, float* out4);
/* The context's two workspaces.  Every one of them is sized by a dry run of the code that carves it (the same allocation sequence
 * against an arena that only counts), so "need" below is exactly what the real run takes.  h_out6 = {scratch capacity (bytes),
 * scratch high-water offset of the last call that used it, cascade-list arena capacity, arena offset, arena need of the last
 * cascade call or trl_debug_lists, dry-run need of the call `what` describes}: what = 0 none (0 bytes); 1 = trl_facenet_embed /
 * _masked / trl_facenet_features on n faces of h x w; 24 / 48 = trl_debug_rnet / trl_debug_onet on n crops (h, w ignored).
 * Nothing runs, nothing is allocated or synchronised.  (ABI v7, additive) */
int  trl_debug_workspace(trl_ctx* ctx, int what, int n, int h, int w, long long* h_out6);
/* Red zones: do the kernels store only inside the workspace block they were handed?  trl_debug_redzone(ctx, guard, byte), on an
 * idle context, frees the context's two workspaces (cascade-list arena and scratch; no cascade state survives) and, for guard > 0
 * (a multiple of 256, at most TRL_RZ_MAX_GUARD), makes every block they hand out be followed by `guard` bytes that belong to no
 * block; dry runs count the same, so need == carve still holds (trl_debug_workspace).  `byte` (0..255) is the fill: it implies
 * trl_debug_poison(byte) for memory allocated later, and trl_debug_poison itself is refused while the guard is on.  While it is
 * on, the library SWEEPS a workspace before each rewind of its allocator, before it frees one to grow it, and at the end of every
 * entry point that queued work on one: it waits for the device, compares every byte outside the live blocks (alignment padding,
 * guards, the tail up to the capacity) with the fill byte, and records one hit per altered gap (the gap is then repaired, so it is
 * reported once).  At a rewind everything from the new offset to the capacity is refilled; a sweep at the end of a call refills
 * nothing.  A hit never fails a call.  guard = 0 switches the mode off and restores the poison setting from before.
 * trl_debug_redzone_report: h_out4 = {sweeps, guard bytes checked, hits, hits copied to h_hits} since the switch was set (or the
 * last clear); flags: TRL_RZ_CLEAR forgets them after reporting, TRL_RZ_SWEEP sweeps both workspaces first (site "report").
 * A hit: arena 0 = cascade lists / 1 = scratch; site = the label of the rewind or entry point that swept ("stage_carve", "chunk",
 * "scratch_begin", "embed_end", ...); block = ordinal of the block in front of the gap since the last full rewind and block_bytes
 * its size (block = number of live blocks and block_bytes = 0: the tail behind the last guard); gap_off / gap_bytes = the gap
 * within the workspace; first / last = first and last altered byte, relative to the gap; count = altered bytes.
 * trl_debug_redzone_poke (self-test): one hipMemset of `value` (!= the fill byte) at byte `offset` of the gap behind block
 * `block` (the tail: block = -1 or the number of live blocks) of arena `arena`; the next sweep reports exactly that.  (ABI v7, additive) */
enum { TRL_RZ_MAX_GUARD = 1 << 20, TRL_RZ_MAX_HITS = 256, TRL_RZ_CLEAR = 1, TRL_RZ_SWEEP = 2 };
typedef struct {
    int32_t arena, block;
    char site[24];
    long long block_bytes, gap_off, gap_bytes, first, last, count;
} trl_rz_hit;
int  trl_debug_redzone(trl_ctx* ctx, long long guard, int byte);
int  trl_debug_redzone_report(trl_ctx* ctx, int flags, long long* h_out4, trl_rz_hit* h_hits, int max_hits);
int  trl_debug_redzone_poke(trl_ctx* ctx, int arena, int block, long long offset, int value);
/* R-Net / O-Net candidate totals of the last call over the whole batch: h_out2[0] = boxes that entered stage 2, [1] = stage 3 */
int  trl_debug_stage_totals(trl_ctx* ctx, int32_t* h_out2);
/* test / tuning hook: consecutive tiles (band order: three tile rows, column by column) a workgroup of the fused PNet launch takes
 * per cursor fetch (0 = automatic: 24 for large batches, down to 1 for small ones).  With runs > 1 a tile reuses the halo columns /
 * rows its left / upper neighbour computed; same results. */
int  trl_debug_pnet_run(trl_ctx* ctx, int run);
/* TUNING builds only (0 otherwise): execution span (first workgroup start -> last workgroup end, device wall clock) of the last
 * fused PNet launch, in ms */
int  trl_debug_pnet_kernel_ms(trl_ctx* ctx, float* ms);
/* TUNING builds with TRL_PNET_SPAN set only (0 launches otherwise): the same span summed on the device over every fused PNet
 * launch of this context since the last reset.  The context must be idle.  The shipped library times the launch with the HIP
 * event pair on its stream (trl_debug_timings out[0]); fused launches of different contexts on one device are ordered one after
 * the other, so that pair measures execution, not queueing. (ABI v6) */
int  trl_debug_pnet_span(trl_ctx* ctx, int reset, double* ms_sum, int32_t* launches);

/* ---- Motion-JPEG output (run()'s annotated video, server/model.py:35-36,77) ------------------------------------------------
 * A baseline JPEG encoder whose files are byte-identical to Pillow's Image.save(format="JPEG", quality, subsampling=2) on the
 * RGB frame (libjpeg-turbo: 4:2:0, Annex K tables scaled by quality, no restart markers, no optimisation; SOI, APP0 JFIF, DQT
 * luma, DQT chroma, SOF0, DHT DC0 AC0 DC1 AC1, SOS, scan, EOI).  An encoder object owns its workspace and is independent of
 * every cascade context.  (ABI v7) */
typedef struct trl_jpeg trl_jpeg;
/* An encoder for H x W frames (1..65535 px per side) at `quality` (clamped to 1..100 as libjpeg does), batches of up to max_frames. */
int  trl_jpeg_create(int device, int H, int W, int quality, int max_frames, trl_jpeg** out);
int  trl_jpeg_destroy(trl_jpeg* enc);
/* n u8 BGR frames [H][W][3] at d_bgr + k * frame_stride bytes (frame_stride >= H*W*3 when n > 1) -> n complete JPEG files back to
 * back at d_out.  h_sizes (host, n entries) receives every file's size whether or not it fitted: frame k starts at the sum of the
 * sizes before it, and a file that would end past `capacity` bytes is not written, nor anything after it.  Sum(h_sizes) > capacity:
 * grow the buffer and call again.  All work is queued on `stream`; the call returns after one synchronisation (to read the sizes). */
int  trl_jpeg_encode(trl_jpeg* enc, const uint8_t* d_bgr, int n, long long frame_stride, uint8_t* d_out, long long capacity,
                     long long* h_sizes, void* stream);
/* Host only, no GPU: the bytes every file of such an encoder starts with (SOI .. SOS).  *len receives the length; a buffer of
 * fewer than *len bytes gives TRL_ERR_CAPACITY and is left untouched. */
int  trl_jpeg_header(int H, int W, int quality, uint8_t* buf, size_t cap, int* len);
/* The encoder with Pillow's other baseline options: every file is byte-identical to Image.save(format="JPEG", quality=q,
 * subsampling=s, restart_marker_rows=r | restart_marker_blocks=b, optimize=o) on the RGB frame.  (ABI v7, additive)
 *   subsampling     Pillow's numbering: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0.  Anything else: TRL_ERR_INVALID.
 *   restart_rows    a restart interval of that many MCU rows; restart_blocks: of that many MCUs (libjpeg counts MCUs, Pillow calls
 *                   them blocks).  As in libjpeg, rows > 0 wins over blocks, and rows x MCUs-per-row above 65535 becomes 65535.  An
 *                   interval of at least the frame's MCU count writes the DRI segment and no marker.  Negative values, and blocks
 *                   above 65535 (Pillow writes a DRI that its own scan does not follow), are TRL_ERR_INVALID.
 *   optimize        non-zero: per-frame optimal Huffman tables (libjpeg's two passes; four DHT segments DC0 AC0 DC1 AC1 per file).
 *                   Frames of 9,227,465 or more luma coefficients are TRL_ERR_INVALID: libjpeg itself fails where such a frame's
 *                   optimal code is deeper than 32 bits.
 * {quality, 2, 0, 0, 0} is trl_jpeg_create's encoder, kernel for kernel.  Bad options allocate nothing. */
typedef struct trl_jpeg_options {
    int quality, subsampling, restart_rows, restart_blocks, optimize;
} trl_jpeg_options;
int  trl_jpeg_create_ex(int device, int H, int W, const trl_jpeg_options* opt, int max_frames, trl_jpeg** out);
/* trl_jpeg_header with options (the DRI segment follows the DHTs).  With `optimize` every frame has a header of its own; this is
 * then the standard-table header, whose length is an upper bound on every frame's header. */
int  trl_jpeg_header_ex(int H, int W, const trl_jpeg_options* opt, uint8_t* buf, size_t cap, int* len);
/* Host only: the optimal Huffman table of 256 symbol counts exactly as libjpeg's jpeg_gen_optimal_table builds it (the function
 * the encoder runs on the device per frame and table).  bits[16]: codes per length; vals[256]: symbols in code order, *nvals of
 * them; *maxlen (may be null): the longest code length before libjpeg's limiting step to 16. */
int  trl_jpeg_optimal_table(const uint32_t* hist, uint8_t* bits, uint8_t* vals, int* nvals, int* maxlen);

/* ---- Motion-JPEG input (run() on Motion-JPEG AVI) -----------------------------------------------------------------------------
 * A baseline JPEG decoder whose BGR frames are byte-identical to np.asarray(Image.open(f).convert("RGB"))[:, :, ::-1]
 * (libjpeg-turbo's default path: islow IDCT, fancy upsampling, 16-bit-fixed colour tables).  Decoded on the device: SOF0, 8 bit,
 * Huffman, three components in one interleaved scan, luma 2x2 / 2x1 / 1x1 over chroma 1x1, any 8-bit DQT, any DHT, any DRI, any
 * APPn other than APP14 (with a JFIF APP0 or without one libjpeg reads such components as YCbCr).  Everything else is not
 * attempted and is left to the caller (Pillow).  (ABI v7, additive) */
typedef struct trl_jpegd trl_jpegd;
typedef struct {
    int32_t width, height;      /* of the SOF0 frame (0 if the parser did not get that far) */
    int32_t h_samp, v_samp;     /* luma sampling factors; chroma is 1x1 */
    int32_t restart_interval;   /* DRI, in MCUs; 0 = none */
    int32_t scan_offset;        /* of the first entropy-coded byte */
    int32_t supported;          /* 1: the device decoder attempts this file */
    int32_t reason;             /* 0, or why not: 1 truncated headers, 2 no SOI, 3 not SOF0 (progressive, arithmetic, ...), 4 not
                                 * 8 bit, 5 not three YCbCr components, 6 sampling, 7 DQT (16 bit, malformed, missing), 8 DHT
                                 * (malformed, over-long, missing), 9 not one interleaved full scan, 10 Adobe APP14, 11 an
                                 * unexpected marker or malformed segment, 12 zero size */
} trl_jpegd_info;
/* Host only, no GPU: what the marker parser finds in one file up to SOS. */
int  trl_jpegd_parse(const uint8_t* file, size_t len, trl_jpegd_info* info);
/* A decoder for H x W frames (1..65535 px per side), batches of up to max_frames files that lie in a buffer of max_bytes bytes.
 * It owns its workspace (coefficients and sample planes, processed in chunks of frames when a batch needs more than 384 MiB). */
int  trl_jpegd_create(int device, int H, int W, int max_frames, long long max_bytes, trl_jpegd** out);
int  trl_jpegd_destroy(trl_jpegd* dec);
/* TEST HOOK, not part of the decoding interface (it is in the shipped library because the GPU suite runs against the shipped
 * library; it reads no environment and changes no result): fills the decoder's whole device workspace (coefficients, sample planes, tables, segment lists) with `byte`.  The
 * decoder must be idle.  A call after it must give the same frames: every byte it reads it has written in that call. */
int  trl_jpegd_debug_poison(trl_jpegd* dec, int byte);
/* n files: file k is sizes[k] bytes at offsets[k] of a buffer that the caller holds twice, on the host (h_files: the headers
 * are parsed there, and the restart markers of DRI streams are located there) and on the device (d_files: the entropy-coded
 * bytes are read there and nowhere else).  Frame k goes to d_bgr + k * frame_stride as u8 BGR [H][W][3].  h_status[k]: 0 decoded
 * on the device; 1 not attempted (unsupported or malformed headers, a size other than the decoder's, more than 2^20 restart
 * intervals in one call); 2 the entropy decoder met something irregular (an invalid code, a run past coefficient 63, bytes
 * running out, an unexpected marker, bytes left over) or a block holds coefficients outside the IDCT's gate (values at which
 * 16-bit and 32-bit arithmetic part; no encoder makes them from pixels).  A frame with status 1 or 2 has no byte written.
 * TRL_ERR_INVALID with nothing queued: n > max_frames, a file outside the buffer, a stride below H*W*3 when n > 1.  All work is
 * queued on `stream`; the call returns after one synchronisation to read the statuses; where a file brings a 17th distinct
 * table set (a clip normally has one), the call goes on from that file as a second pass with a synchronisation of its own. */
int  trl_jpegd_decode(trl_jpegd* dec, const uint8_t* h_files, const uint8_t* d_files, const long long* offsets, const long long* sizes,
                      int n, uint8_t* d_bgr, long long frame_stride, int32_t* h_status, void* stream);

/* ---- Annotation on device frames (run()'s rectangle and caption, server/model.py:67-74) ----------------------------------------
 * Draws on u8 BGR frames in device memory exactly the bytes annotate.py's own rasteriser (the one used when OpenCV is absent)
 * draws on a host frame, so that frames can go from the colour conversion to the JPEG encoder without visiting the host.
 * Needs no context and no weights; the device is the one that owns d_bgr.  (ABI v7, additive) */
typedef struct {
    int32_t frame;              /* which frame of the batch, 0 <= frame < n; a frame may be listed once per call */
    int32_t x0, y0, x1, y1;     /* cv2.rectangle corners (either order), drawn first; may lie outside the frame */
    int32_t thickness;          /* of the rectangle; 0 = no rectangle */
    int32_t seg_begin, seg_end; /* this frame's segments: segs[seg_begin .. seg_end), blended in that order after the rectangle */
    uint8_t rect_bgr[3];
    uint8_t text_bgr[3];
    uint8_t reserved[2];
} trl_draw_frame;               /* 40 bytes */
/* One anti-aliased thick segment from (x0, y0) to (x0 + dx, y0 + dy): coverage of the pixel centre (x, y) is
 * clip(reach - distance to the segment, 0, 1) with reach = thickness / 2 + 0.5, L2 = dx*dx + dy*dy (0: a dot).  The caller
 * computes the six numbers in double precision and rounds each once (annotate.draw_list); the kernel's arithmetic is float32. */
typedef struct { float x0, y0, dx, dy, L2, reach; } trl_draw_seg;
/* Device bytes trl_draw needs for lists of these lengths. */
size_t trl_draw_workspace(int n_frames, int n_segs);
/* n u8 BGR frames [H][W][3] at d_bgr + k * frame_stride bytes (frame_stride >= H*W*3; H, W >= 1).  `frames` and `segs` are HOST
 * lists: the call checks them, copies what the kernel needs into d_work (device, 16-byte aligned, work_bytes >=
 * trl_draw_workspace(n_frames, n_segs)) and queues the copy and the kernel on `stream`; it returns without synchronising, the
 * host lists may be reused at once, and d_work must stay untouched until the queued work has run.  TRL_ERR_INVALID with nothing
 * drawn: a frame index outside [0, n) or listed twice, a segment range outside the list, a value that is not finite, a negative
 * thickness, a stride below H*W*3, sizes below 1, a workspace too small.  n_frames = 0: TRL_OK, nothing is looked at. */
int  trl_draw(uint8_t* d_bgr, int n, long long frame_stride, int H, int W, const trl_draw_frame* frames, int n_frames,
              const trl_draw_seg* segs, int n_segs, void* d_work, size_t work_bytes, void* stream);

/* ---- Embedding match (the step after InceptionResnetV1: "whose face is this?") -------------------------------------------------
 * A gallery of enrolled 512-float embeddings in device memory, the score matrix of n queries against it, and a fused top-k search
 * that streams the gallery once and never writes that matrix.  Needs no context and no weights; all memory is the caller's, the
 * device is the one that owns d_mat, all work is queued on `stream` and no call synchronises.  (ABI v7, additive)
 *   layout   d_mat is k-major, [512][ld] f32 with ld a positive multiple of 32, padding columns zero; d_n2[ld] holds n2 of every
 *            column.  Gallery row c is column c.
 *   dot      dot(q, g) = chain(0; k = 0..511 ascending: acc = fmaf(q[k], g[k], acc)), one f32 chain; n2(x) = dot(x, x).
 *   metric   0 cosine: dot / (sqrtf(n2 q) * sqrtf(n2 g)), larger is better, a zero row gives NaN.
 *            1 euclidean: s = n2 q + n2 g; d2 = fmaf(-2, dot, s); d2 < 0 ? 0 : d2 (NaN stays NaN); sqrtf(d2), smaller is better.
 *   order    better score first; equal scores (as floats: -0 == +0) to the lower gallery index; NaN scores after every other,
 *            lower index first.  Slots past the gallery (k > m), and every slot of a row with d_valid[r] == 0: index -1, score NaN.
 * Results are the same bits whatever n, strip length or stream.
 * TRL_ERR_INVALID with nothing queued: ld or ldo out of range, k outside 1..16, a metric other than 0 / 1, c0 + m > ld, m > ld,
 * m > 2^31 - 1, max_strip_cols no multiple of 128, a workspace too small or not 8-byte aligned, a null pointer. */
/* d_rows [m][512] row-major (as the embedder writes them) -> columns c0 .. c0 + m - 1 of d_mat and their n2 into d_n2[c0 ..]. */
int    trl_gallery_pack(const float* d_rows, long long m, float* d_mat, long long ld, float* d_n2, long long c0, void* stream);
/* d_out[r * ldo + c] = score of query r against gallery row c, r < n, c < m (ldo >= m); nothing else is written. */
int    trl_gallery_scores(const float* d_q, int n, const float* d_mat, long long ld, const float* d_n2, long long m, int metric,
                          float* d_out, long long ldo, void* stream);
/* Device bytes trl_gallery_search needs: n x k (score, index) pairs per strip of gallery columns.  The strip count follows from n
 * and m and is bounded (512) unless max_strip_cols forces shorter strips, so the size does not grow with m.  0 on bad arguments. */
size_t trl_gallery_search_workspace(int n, long long m, int k, int max_strip_cols);
/* The k best gallery rows of each query, in order: d_score [n][k], d_index [n][k].  d_valid (n bytes) may be null: every row is
 * searched.  max_strip_cols: 0, or the most gallery columns one workgroup walks (a multiple of 128; the tests use it to reach the
 * merge of several strips at a small gallery).  n = 0: nothing is done; m = 0: the outputs are filled with -1 / NaN. */
int    trl_gallery_search(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                          long long m, int metric, int k, float* d_score, int32_t* d_index, void* d_ws, size_t ws_bytes,
                          int max_strip_cols, void* stream);

/* ---- Embedding clustering ("which of these faces are the same person?") ---------------------------------------------------------
 * DBSCAN over n embeddings without the n x n score matrix: a packed link bitmap (n^2 / 8 bytes) and labels computed from it, both
 * on the device.  Context-free, caller-owned memory, work queued on `stream`, the device that of d_mat / d_count.  (ABI v7, additive)
 *   score    score(i, j) is the gallery's (above), row i as the query and row j as the gallery row; it is symmetric bit for bit.
 *   link     i != j, both rows valid, and score >= threshold (cosine) or score <= threshold (euclidean).  A NaN score never links.
 *   degree   1 + the number of links of a valid row (a row counts itself, whatever its own score is); 0 for an invalid row.
 *   core     degree >= min_samples.
 *   cluster  a connected component of the link graph restricted to core rows; clusters are numbered 0, 1, ... in ascending order
 *            of their smallest core member.
 *   label    a core row: its cluster's number.  A valid row that is not core and links to a core row (a border row): the smallest
 *            number among its core neighbours' clusters.  Every other row (noise, invalid rows): -1.
 * This is sklearn.cluster.DBSCAN(metric="precomputed") on D = link ? 0 : 1, eps = 0.5, and it does not depend on visiting order.
 * The result depends on the scores and the rule alone: not on strips, launch geometry or the number of rounds.
 * TRL_ERR_INVALID with nothing queued: n < 0 or n > 65,536 (the bitmap is 512 MB there), pitch_words < ceil(n / 32), a threshold
 * that is NaN or infinite, min_samples < 1, a metric other than 0 / 1, ld out of range or n > ld, max_strip_cols no multiple of
 * 128, a workspace too small or not 8-byte aligned, a null pointer where one is needed. */
/* d_q: the n rows [n][512]; d_mat / d_n2: THE SAME n rows packed by trl_gallery_pack at column 0 (the caller guarantees it).  Writes
 * the bitmap -- bit b of d_adj[i * pitch_words + w] <=> link(i, 32 w + b), rows < n, words < ceil(n / 32), bits at columns >= n zero,
 * nothing else -- and d_degree[i], i < n.  d_valid (n bytes) may be null: every row is valid.  max_strip_cols as in
 * trl_gallery_search.  n = 0: nothing is done.  Does not synchronise. */
int    trl_cluster_links(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                         int metric, float threshold, uint32_t* d_adj, long long pitch_words, int32_t* d_degree,
                         int max_strip_cols, void* stream);
/* Device bytes of trl_cluster_labels' d_ws (three int32 per row and the change flags).  0 on bad arguments. */
size_t trl_cluster_workspace(int n);
/* Labels from a bitmap and its degrees (degree 0 = invalid row; the bitmap must be symmetric with an empty diagonal, as
 * trl_cluster_links writes it): d_labels [n] int32, d_core [n] uint8, *d_count = the number of clusters.  Components come from rounds
 * of min-label hooking (a row, and the row its label names, take the smallest label among the row's core neighbours) and pointer
 * jumping, one launch each; the host reads a device flag after every four rounds, so THIS CALL
 * SYNCHRONISES `stream` (and cannot be captured into a graph).  *rounds_out (a host int, may be null): the rounds up to and including
 * the first that changed nothing.  A loop that passes n rounds returns TRL_ERR_STATE.  n = 0: *d_count = 0, nothing else. */
int    trl_cluster_labels(const uint32_t* d_adj, long long pitch_words, const int32_t* d_degree, int n, int min_samples,
                          int32_t* d_labels, uint8_t* d_core, int32_t* d_count, void* d_ws, size_t ws_bytes, int* rounds_out,
                          void* stream);
/* The label stage over neighbour lists instead of bitmap rows: the same degree / core / cluster / label rules, for up to 16,777,216
 * rows.  The links are CSR lists: d_offsets [n + 1] int64 (ascending from 0), d_index [offsets[n]] int32, row i's neighbours
 * index[offsets[i] .. offsets[i + 1]) -- what trl_gallery_range_count / trl_gallery_range_fill write with self = 1; the scores are
 * not an input.  The lists must be symmetric, without a self entry and without duplicates (the caller guarantees it, as for the
 * bitmap); d_valid (n bytes, may be null: every row valid) tells a valid row without links (degree 1) from an invalid one (degree 0).
 * Writes d_degree [n] (list length + 1 of a valid row, 0 of an invalid one), d_labels [n], d_core [n] and *d_count.  An entry of
 * d_index outside 0 .. n - 1 is skipped and never followed; lists that are not symmetric give unspecified labels, no access out of
 * bounds, and the rounds still end (labels only decrease).
 *   lanes_per_row   4, 16 or 64: the lanes of a wave that walk one row's list.  0: chosen from the mean list length offsets[n] / n
 *                   (4 below 384 entries, else 16: DESIGN section 7, f-8), which is read back first.  The result does not depend on it.
 * Rounds, *rounds_out, the synchronisation of `stream` and TRL_ERR_STATE as for trl_cluster_labels.  TRL_ERR_INVALID with nothing
 * queued and nothing written: n < 0 or n > 16,777,216, min_samples < 1, lanes_per_row not 0 / 4 / 16 / 64, a workspace too small or
 * not 8-byte aligned, a null pointer where one is needed (d_index too unless n = 0; d_valid and rounds_out may be null).
 * n = 0: *d_count = 0, nothing else. */
/* Device bytes of trl_cluster_labels_lists' d_ws: three int32 per row and the change flags, nothing per link.  0 on bad arguments. */
size_t trl_cluster_lists_workspace(int n);
int    trl_cluster_labels_lists(const long long* d_offsets, const int32_t* d_index, const uint8_t* d_valid, int n, int min_samples,
                                int lanes_per_row, int32_t* d_degree, int32_t* d_labels, uint8_t* d_core, int32_t* d_count,
                                void* d_ws, size_t ws_bytes, int* rounds_out, void* stream);

/* ---- Score histograms ("which threshold?") -------------------------------------------------------------------------------------
 * Exact pair counts per score bin, genuine (d_qid[i] == d_gid[j]) and impostor pairs apart, of n query rows against the m gallery
 * rows, without the n x m score matrix: the gallery is streamed once and a few KB are written.  From the counts follow the false
 * and true accept rates of identify / cluster at every candidate threshold.  Context-free, caller-owned memory, work queued on
 * `stream`, no synchronisation, the device that of d_mat.  (ABI v7, additive)
 *   score    the gallery's (above).
 *   edges    d_edges[nedges] f32 candidate thresholds, 1 <= nedges <= 1023, strictly ascending, no NaN, +-inf allowed (THE CALLER
 *            guarantees the values: unsorted edges give unspecified counts, never an access out of bounds).
 *   bin      cosine: #{e : edges[e] <= score}; euclidean: #{e : edges[e] < score}; both in 0..nedges, plain f32 comparisons
 *            (-0 == +0).  A NaN score goes to slot nedges + 1.  So cosine accepts score >= edges[e] <=> bin > e, and euclidean
 *            accepts score <= edges[e] <=> bin <= e: cumulative sums of the counts are the shipped predicates' counts.
 *   counted  pair (i, j): i < n, j < m, d_qvalid[i] != 0, d_gvalid[j] != 0 (either mask may be null: all valid) and, with
 *            pairs = 1 (upper), j > i.
 *   pairs    0 all n x m pairs.  1 upper: n == m and d_q are THE SAME rows as the gallery's (the caller guarantees it, as for
 *            trl_cluster_links); each unordered pair is counted once and the scores below the diagonal are not computed.
 *   counts   d_counts [2][nedges + 2] int64, class 0 impostor, 1 genuine.  The call writes all of it; nothing is pre-zeroed.
 * Counts are integers summed exactly: the same whatever n, strip length or stream.
 * TRL_ERR_INVALID with nothing queued: nedges outside 1..1023, a metric or pairs other than 0 / 1, upper with n != m, ld out of
 * range or m > ld, negative sizes, m > 2^31 - 1, max_strip_cols no multiple of 128, a workspace too small or not 8-byte aligned, a
 * null pointer (d_q and d_qid may be null when n = 0, d_gid when m = 0).  n = 0 or m = 0: the counts are zero. */
/* Device bytes of trl_gallery_hist's d_ws: 2 (nedges + 2) uint32 counters per workgroup (row tile x strip).  0 on bad arguments. */
size_t trl_gallery_hist_workspace(int n, long long m, int nedges, int max_strip_cols);
int    trl_gallery_hist(const float* d_q, const uint8_t* d_qvalid, const int32_t* d_qid, int n, const float* d_mat, long long ld,
                        const float* d_n2, const uint8_t* d_gvalid, const int32_t* d_gid, long long m, int metric, int pairs,
                        const float* d_edges, int nedges, long long* d_counts, void* d_ws, size_t ws_bytes, int max_strip_cols,
                        void* stream);

/* ---- Range search ("every enrolled row within the threshold") ------------------------------------------------------------------
 * All matches of n query rows among the m gallery rows as CSR lists, without the n x m score matrix and without a buffer of n x m
 * bits: the gallery is streamed twice, once to count and once to store.  Context-free, caller-owned memory, work queued on
 * `stream`, no synchronisation, the device that of d_mat.  (ABI v7, additive)
 *   score    the gallery's (above).
 *   match    match(r, c) <=> d_qvalid[r] != 0 and d_gvalid[c] != 0 and (self == 0 or c != r) and
 *            (cosine: score >= threshold | euclidean: score <= threshold), plain f32 comparisons: a NaN score never matches,
 *            -0 == +0, +-inf scores compare as floats do.  Either mask may be null: all rows valid.
 *   self     1: n == m and d_q are THE SAME rows as the gallery's (the caller guarantees it, as for trl_cluster_links); a row does
 *            not match itself.  The lists are then the rows of trl_cluster_links' bitmap at the same threshold.
 *   result   d_offsets [n + 1] int64: offsets[0] = 0, offsets[r + 1] - offsets[r] = the matches of row r, offsets[n] the total.
 *            d_index [total] int32: row r's matching gallery rows in ASCENDING GALLERY INDEX at offsets[r] ..;
 *            d_score [total] f32: their scores, the bits trl_gallery_scores writes.
 * The result depends on the scores and the rule alone: not on n, strips, max_strip_cols, the stream or launch geometry.
 * TRL_ERR_INVALID with nothing queued and nothing written: negative sizes, m > 2^31 - 1, ld out of range or m > ld, a metric or
 * self other than 0 / 1, self = 1 with n != m, a threshold that is NaN or infinite, max_strip_cols no multiple of 128, a workspace
 * too small or not 8-byte aligned, capacity < 0, a null pointer where one is needed (d_q may be null when m = 0, d_index and
 * d_score when capacity = 0, everything but the gallery when n = 0). */
/* Device bytes of d_ws: one uint32 per (strip, wave, row), 4 waves -- pass 1's counts, turned in place into the bases of pass 2.
 * The strip count is trl_gallery_search's, so the size does not grow with m unless max_strip_cols forces shorter strips.  0 on bad
 * arguments, and when n = 0 or m = 0. */
size_t trl_gallery_range_workspace(int n, long long m, int max_strip_cols);
/* Pass 1: streams the gallery once, writes d_offsets[0 .. n] and leaves pass 2's bases in d_ws.  No atomic on global memory.
 * n = 0: nothing is done; m = 0: the offsets are all zero. */
int    trl_gallery_range_count(const float* d_q, const uint8_t* d_qvalid, int n, const float* d_mat, long long ld, const float* d_n2,
                               const uint8_t* d_gvalid, long long m, int metric, float threshold, int self, long long* d_offsets,
                               void* d_ws, size_t ws_bytes, int max_strip_cols, void* stream);
/* Pass 2: streams the gallery again and writes entry p of d_index / d_score iff p < capacity; entries at p >= capacity, and
 * everything else, are not written (trl_jpeg_encode's capacity convention: the caller reads offsets[n] and sizes or refuses).
 * Valid only behind a trl_gallery_range_count with the same arguments, d_offsets and d_ws, in stream order. */
int    trl_gallery_range_fill(const float* d_q, const uint8_t* d_qvalid, int n, const float* d_mat, long long ld, const float* d_n2,
                              const uint8_t* d_gvalid, long long m, int metric, float threshold, int self, const long long* d_offsets,
                              const void* d_ws, size_t ws_bytes, long long capacity, int32_t* d_index, float* d_score,
                              int max_strip_cols, void* stream);

/* ---- Grouped search ("the k most likely people, each with their best shot") -----------------------------------------------------
 * trl_gallery_search over a gallery that enrols several rows per identity: per query the k best DISTINCT groups, each with its best
 * row, without the n x m score matrix -- the gallery is streamed once.  Context-free, caller-owned memory, work queued on `stream`,
 * no synchronisation, the device that of d_mat.  (ABI v7, additive)
 *   group    d_gid [m] int32: gallery row c belongs to group d_gid[c]; a row with d_gid[c] < 0 is excluded (a gallery mask is
 *            expressed this way).
 *   rule     per query: take the rows that are not excluded in the match order above (better score first, equal scores to the lower
 *            index, NaN last); keep a row iff no earlier row of that order has its group; the first k kept rows are the result,
 *            k <= 16.  With all ids distinct this is trl_gallery_search's result.
 *   result   d_score / d_index / d_group [n][k]: the kept rows' scores (trl_gallery_scores' bits), gallery indices and groups.
 *            Slots past the last kept row, and every slot of a row with d_valid[r] == 0: NaN / -1 / -1.
 * The result depends on the scores and the rule alone: not on n, strips, max_strip_cols, the stream or launch geometry.
 * TRL_ERR_INVALID with nothing queued: what trl_gallery_search refuses, and a null d_gid when m > 0. */
/* Device bytes of d_ws: n x k (score, index) pairs and n x k group ids per strip; trl_gallery_search's plan, so 0 when one strip
 * writes the result itself and no growth with m unless max_strip_cols forces shorter strips.  0 on bad arguments. */
size_t trl_gallery_search_groups_workspace(int n, long long m, int k, int max_strip_cols);
/* n = 0: nothing is done; m = 0: the outputs are filled with NaN / -1 / -1. */
int    trl_gallery_search_groups(const float* d_q, const uint8_t* d_valid, int n, const float* d_mat, long long ld, const float* d_n2,
                                 const int32_t* d_gid, long long m, int metric, int k, float* d_score, int32_t* d_index,
                                 int32_t* d_group, void* d_ws, size_t ws_bytes, int max_strip_cols, void* stream);

/* ---- Face tracks ("which face of this frame is which face of the last one") ------------------------------------------------------
 * Association of every face of a clip's sampled frames into tracks, with the drift state machine of trl_drift_update per track
 * instead of per largest face.  Context-free, caller-owned memory, work queued on `stream`, no synchronisation, the device that of
 * d_state.  (ABI v7, additive.)  The rules are DESIGN.md section 2, "Tracks"; in short, per frame of the window and in this order:
 *   ageing    a track whose last matched frame lies more than max_age frames before the previous frame ends (INT32_MAX: never)
 *   pairs     every (live track, detection): iou = torchvision's box_iou in float32; with d_emb, sim = drift_sims_kernel's cosine
 *             of the detection's row and the row of the track's last matched detection.  Admissible iff (iou_min <= 0 or
 *             iou >= iou_min) and (no d_emb or sim >= sim_min); NaN fails.  The key is sim with d_emb, iou without.
 *   matching  greedy: the admissible pair of an unmatched track and an unmatched detection with the largest key, ties to the lower
 *             track id, then the lower detection index; repeat
 *   matched   the track takes the detection's box and row and, with d_emb, makes one state-machine step with the pair's sim
 *   new       every unmatched detection, in ascending index, starts the track with the next id (0, 1, 2, ... over the clip) in the
 *             free slot of the lowest index, else in the slot of the track not matched or created in this frame with the smallest
 *             last frame (ties: smallest id), which ends
 * A frame's detections past its first TRL_TRACK_SLOTS get no track and are counted as dropped.
 *   d_state   TRL_TRACK_STATE_BYTES, 8-byte aligned, zero-filled before a clip's first window; the layout is private.  One clip
 *             is tracked with d_emb in every window or in none.
 *   window    d_counts [n] int32 faces per frame; d_boxes [m][4] f32 x1, y1, x2, y2 and d_emb [m][512] f32 (or NULL) hold the
 *             frames' rows one after the other; rows past the sum of d_counts are not read.  Frame t of the window is the clip's
 *             frame (frames seen by earlier calls) + t.  n = 0 and m = 0 are legal: frames without faces still age the tracks.
 *   outputs   d_track [m] int32 (the row's track id, -1 for none), d_sim [m] f32 (the matched pair's sim; 2.0 = no comparison: a new
 *             track, a dropped row, or no d_emb), d_flag [m] u8 (the state machine's flag).  Rows past the sum: -1 / 2.0 / 0.
 *   d_table   [table_cap][8] int32, row = track id: first_frame, last_frame, n_obs, run, hits, slot (-1 once the track has ended),
 *             0, 0; written whenever a frame touches the track.  A track whose id is >= table_cap is tracked all the same, its
 *             row is not written, and the state counts it; nothing is written past the table.
 * The outputs depend on the inputs and the rules alone: not on how the clip is cut into windows, the stream or launch geometry. */
#define TRL_TRACK_SLOTS 64
#define TRL_TRACK_STATE_BYTES 135200
int    trl_track_update(void* d_state, const float* d_boxes, const int32_t* d_counts, int n, int m, const float* d_emb, float iou_min,
                        float sim_min, int max_age, int32_t* d_track, float* d_sim, uint8_t* d_flag, int32_t* d_table, int table_cap,
                        void* stream);
/* d_score [table_cap] int32: per row the score of trl_drift_score from that track's run and hits and the clip's frame_count and
 * fps (rows of ids not yet created: 0).  d_summary [4] int32: the clip's score (the largest; 0 without a track), the id of the
 * track that has it (the lowest among equals, -1 without a track), the number of tracks created, the dropped detections. */
int    trl_track_scores(const void* d_state, const int32_t* d_table, int table_cap, long long frame_count, int fps, int32_t* d_score,
                        int32_t* d_summary, void* stream);

#ifdef __cplusplus
}
#endif
#endif

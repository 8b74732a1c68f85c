// trl_nets.hip -- host-side walkers that issue the layer kernels of the four networks.
//
// Architecture restated from the published facenet_pytorch 2.6.0 modules (absent from
// /root/reference), call sites server/model.py:18-19,47,59.
// Activations are NHWC f32 in the context arena; a concat is a channel slice of a wider
// buffer (Act.coff / Act.ld), so torch.cat costs nothing.
#include "trl_ctx.h"
#include <stdlib.h>
#include <string.h>

thread_local TrlConvChoice g_trl_conv_choice;

const NetDesc trl_nets[3] = {
    {"pnet", 0, 5, {{"conv1", "prelu1", 3, 1, 10}, {nullptr, nullptr, 2, 2, 0}, {"conv2", "prelu2", 3, 1, 16}, {"conv3", "prelu3", 3, 1, 32},
                    {"heads", nullptr, 1, 1, 6}},
     0, 0, 0, 6, nullptr},
    {"rnet", 24, 7, {{"conv1", "prelu1", 3, 1, 28}, {nullptr, nullptr, 3, 2, 0}, {"conv2", "prelu2", 3, 1, 48}, {nullptr, nullptr, 3, 2, 0},
                     {"conv3", "prelu3", 2, 1, 64}, {"dense4", "prelu4", 3, 1, 128}, {"heads", nullptr, 1, 1, 6}},
     2, 11, 28, 6, &Options::rnet_chunk},
    {"onet", 48, 9, {{"conv1", "prelu1", 3, 1, 32}, {nullptr, nullptr, 3, 2, 0}, {"conv2", "prelu2", 3, 1, 64}, {nullptr, nullptr, 3, 2, 0},
                     {"conv3", "prelu3", 3, 1, 64}, {nullptr, nullptr, 2, 2, 0}, {"conv4", "prelu4", 2, 1, 128}, {"dense5", "prelu5", 3, 1, 256},
                     {"heads", nullptr, 1, 1, 16}},
     2, 23, 32, 16, &Options::onet_chunk},
};

namespace {

struct Runner {
    trl_ctx* c;
    hipStream_t s;
    Arena& X;                         // where alloc() takes the activations from
    const bool check_only = X.counting;   // a counting X: shapes and tensors only -- alloc() counts, issue() launches nothing
    int err = TRL_OK;
    const int32_t* m_dev = nullptr;   // device-sized batch (candidate lists): item count lives on the device, see ConvArgs
    int m_base = 0;
    // the plan rows of trl_debug_facenet_plan and the armed capture of trl_debug_facenet_capture (conv index = walk order)
    std::vector<trl_fn_plan_row>* plan = nullptr;
    int nconv = 0;
    const char* layer = "";           // name of the conv being issued: FaceNet's point into its table, they outlive the walk
    struct ConvMeta { int idx; const char* layer; Act x, y; bool has_res; Act res; };
    std::vector<ConvMeta> pending_meta;

    // Host bookkeeping behind a launch: the plan row (g_trl_conv_choice is what the launcher just picked) and, when this conv is
    // the armed one, stream-ordered copies of its views -- before any later kernel can reuse a slice.
    void launched(const ConvArgs& a, const ConvMeta& m) {
        if (!plan) return;
        trl_fn_plan_row r;
        memset(&r, 0, sizeof(r));
        const TrlConvChoice& ch = g_trl_conv_choice;
        r.conv = m.idx; r.family = ch.family; r.bm = ch.bm; r.bn = ch.bn; r.bk = ch.bk; r.pad = ch.pad; r.nz = ch.nz;
        r.m = a.M; r.cout = a.Cout; r.k = a.K; r.precision = a.lowp; r.has_res = m.has_res;
        strncpy(r.layer, m.layer, sizeof(r.layer) - 1);
        plan->push_back(r);
        if (plan != &c->hook.fn_plan || c->hook.fn_cap_arm != m.idx) return;   // captures are FaceNet convs only
        int st = capture(0, m.x, 1 << 30, 0);
        if (st == TRL_OK && m.has_res) st = capture(1, m.res, 1 << 30, 0);
        if (st == TRL_OK) st = capture(2, m.y, a.ysplit, a.yskip);
        if (st != TRL_OK && err == TRL_OK) err = st;
    }
    int capture(int v, const Act& a, int ysplit, int yskip) {
        auto& b = c->hook.fn_cap[v];
        const size_t es = a.bf ? sizeof(uint16_t) : sizeof(float), row = (size_t)a.c * es, need = row * a.pixels();
        if (b.cap < need) {
            if (b.p) TRL_HIP(hipFree(b.p));
            b.p = nullptr; b.cap = 0;
            TRL_HIP(hipMalloc(&b.p, need));
            b.cap = need;
        }
        const char* src = reinterpret_cast<const char*>(a.p) + (size_t)a.coff * es;
        const int c0 = ysplit < a.c ? ysplit : a.c;    // a scattered destination (block35_grouped): columns >= ysplit sit yskip further
        TRL_HIP(hipMemcpy2DAsync(b.p, row, src, (size_t)a.ld * es, (size_t)c0 * es, a.pixels(), hipMemcpyDeviceToDevice, s));
        if (c0 < a.c)
            TRL_HIP(hipMemcpy2DAsync(static_cast<char*>(b.p) + (size_t)c0 * es, row, src + (size_t)(c0 + yskip) * es, (size_t)a.ld * es,
                                     (size_t)(a.c - c0) * es, a.pixels(), hipMemcpyDeviceToDevice, s));
        const int32_t d[5] = {a.n, a.h, a.w, a.c, (int32_t)es};
        memcpy(b.dims, d, sizeof(d));
        return TRL_OK;
    }

    Act alloc(int n, int h, int w, int ch, bool bf = false) {
        Act a;
        a.n = n; a.h = h; a.w = w; a.c = ch; a.ld = ch; a.coff = 0; a.bf = bf;
        // + 64: slack for READS only (vector loads of a map's last elements may run past its end).  No kernel stores into it: with
        // the slack at 0 and red zones on (trl_debug_redzone), the embedder (f32 both block35 forms, no_fnconv, bf16, fp16), the
        // R-/O-Net walks and the cascade left every guard byte intact.  The sweeps cannot see reads, so the slack stays.
        a.p = (float*)X.alloc((size_t)n * h * w * ch * (bf ? sizeof(uint16_t) : sizeof(float)) + 64);
        if (!a.p && err == TRL_OK) {
            trl_set_error("activation scratch exhausted (%zu of %zu bytes used)", X.off, X.cap);
            err = TRL_ERR_STATE;
        }
        return a;
    }
    static Act slice(const Act& buf, int coff, int ch) {
        Act a = buf;
        a.coff = buf.coff + coff;
        a.c = ch;
        return a;
    }

    // Deferred launches: convs queued between begin_group() and end_group() are independent of each other and go out as ONE
    // launch when the small-map family takes them all (trl_launch_fn_group), else one by one in order.
    std::vector<ConvArgs> pending;
    bool grouping = false;
    int ysplit = 1 << 30, yskip = 0;   // destination scatter of the next conv: output column n >= ysplit lands yskip channels further
    void begin_group() { grouping = true; pending.clear(); pending_meta.clear(); }
    void end_group() {
        grouping = false;
        if (pending.empty() || err != TRL_OK) { pending.clear(); pending_meta.clear(); return; }
        bool all = pending.size() <= 3;
        for (auto& a : pending) all = all && trl_fn_eligible(a);
        if (all) for (auto& a : pending) all = all && (trl_fn_split4_rule(a) == trl_fn_split4_rule(pending[0]));
        int st = TRL_OK;
        if (all) {
            st = trl_launch_fn_group(pending.data(), (int)pending.size(), s);
            if (st == TRL_OK) for (size_t i = 0; i < pending.size(); i++) launched(pending[i], pending_meta[i]);
        } else {
            for (size_t i = 0; i < pending.size(); i++) {
                st = trl_launch_conv(pending[i], s);
                if (st != TRL_OK) break;
                launched(pending[i], pending_meta[i]);
            }
        }
        if (st != TRL_OK) err = st;
        pending.clear(); pending_meta.clear();
    }

    // Every launch of a walk that is no conv goes out through here
    template <class F> void issue(F&& launch) {
        if (check_only || err != TRL_OK) return;
        const int st = launch();
        if (st != TRL_OK) err = st;
    }

    // generic conv launcher; `into` selects a pre-allocated (concat) destination view
    Act conv(const Act& x, const DevW* w, const float* bias, const float* scale, const float* shift, const float* slope,
             int kh, int kw, int sh, int sw, int ph, int pw, int act, const Act* into, const Act* res, float res_scale) {
        const int OH = (x.h + 2 * ph - kh) / sh + 1, OW = (x.w + 2 * pw - kw) / sw + 1;
        Act y = into ? *into : alloc(x.n, OH, OW, w ? w->Cout : 0, x.bf);
        if (err != TRL_OK) return y;
        if (!w || w->K != kh * kw * x.c || (into && (into->h != OH || into->w != OW || into->c != w->Cout))) {
            trl_set_error("conv shape mismatch (K=%d expected %d)", w ? w->K : -1, kh * kw * x.c);
            err = TRL_ERR_WEIGHTS;
            return y;
        }
        if (check_only) return y;
        ConvArgs a;
        a.x = x.p; a.N = x.n; a.H = x.h; a.W = x.w; a.Cin = x.c; a.ldx = x.ld; a.xoff = x.coff;
        a.w = w->p; a.ldw = w->ld; a.K = w->K;
        a.bias = bias; a.scale = scale; a.shift = shift; a.slope = slope;
        a.res = res ? res->p + res->coff : nullptr; a.ldres = res ? res->ld : 0; a.res_scale = res_scale;
        a.y = y.p; a.ldy = y.ld; a.yoff = y.coff;
        a.KH = kh; a.KW = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw;
        a.Cout = w->Cout; a.OH = OH; a.OW = OW; a.act = act;
        a.M = x.n * OH * OW;
        a.m_dev = m_dev; a.m_base = m_base; a.m_per = OH * OW;
        a.ysplit = ysplit; a.yskip = yskip;
        if (yskip && !trl_fn_eligible(a)) { trl_set_error("scattered destination needs the small-map conv family"); err = TRL_ERR_STATE; return y; }
        ConvMeta meta{nconv++, layer, x, y, res != nullptr, res ? *res : Act()};
        if (x.bf) {   // reduced-precision embedder: bf16 in / out / residual, transposed bf16 weights
            if (!w->pt || y.bf != true || (res && !res->bf) || act == TRL_ACT_PRELU) {
                trl_set_error("bf16 conv without bf16 weights / destination");
                err = TRL_ERR_STATE;
                return y;
            }
            a.lowp = c->cfg.embed_precision; a.wt = w->pt; a.ldwt = w->ldt;
            if (res) a.res = reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(res->p) + res->coff);
            int st = trl_launch_conv_bf16(a, s);
            if (st != TRL_OK) err = st;
            else launched(a, meta);
            return y;
        }
        if (grouping) { pending.push_back(a); pending_meta.push_back(meta); return y; }
        int st = trl_launch_conv(a, s);
        if (st != TRL_OK) err = st;
        else launched(a, meta);
        return y;
    }
    // A valid k x k conv (bias, PReLU) of the MTCNN tails and the ceil-mode pk / pst max pool behind it as ONE launch, where the
    // kernel the dispatch picks for the conv has a pooling epilogue for that pool (trl_conv_pool_family): *out = the pooled map; the
    // conv's own map does not exist.  false: not taken, nothing done -- the caller issues conv and pool.
    bool conv_pool(const Act& x, const NetLayerW& lw, int k, int act, int pk, int pst, Act* out) {
        const DevW* w = lw.w;
        if (err != TRL_OK || !w || x.bf || x.h != x.w || w->K != k * k * x.c) return false;
        const int S = x.h - k + 1;
        ConvPoolArgs a;
        a.x = x.p; a.N = x.n; a.H = x.h; a.W = x.w; a.Cin = x.c; a.ldx = x.ld; a.xoff = x.coff;
        a.w = w->p; a.ldw = w->ld; a.K = w->K;
        a.bias = lw.b; a.scale = nullptr; a.shift = nullptr; a.slope = lw.slope;
        a.res = nullptr; a.ldres = 0; a.res_scale = 0.f;
        a.y = nullptr; a.ldy = w->Cout; a.yoff = 0;
        a.KH = k; a.KW = k; a.sh = 1; a.sw = 1; a.ph = 0; a.pw = 0;
        a.Cout = w->Cout; a.OH = S; a.OW = S; a.act = act;
        a.M = x.n * S * S;
        a.m_dev = m_dev; a.m_base = m_base; a.m_per = S * S;
        a.pk = pk; a.pst = pst;
        if (S < pk || (long long)x.n * S * S > (1 << 30) || !trl_conv_pool_family(a, pk, pst)) return false;
        const TailPool tp{S, pk, pst, TRL_TAIL_POOL_BM};
        const Act y = alloc(x.n, tp.P(), tp.P(), w->Cout);
        const Act side = tp.can_straddle() ? alloc(x.n, tp.P(), tp.P(), w->Cout) : Act();   // second parts of windows two tiles share
        *out = y;
        if (err != TRL_OK || check_only) return true;
        a.y = y.p; a.side = side.p;
        ConvMeta meta{nconv++, layer, x, y, false, Act()};
        const int st = trl_launch_conv_pool(a, s);
        if (st != TRL_OK) err = st;
        else launched(a, meta);
        return true;
    }
    // Row r of FaceNet's table (trl_facenet.h): its geometry, and the tensors trl_load_weights resolved for it.  A BasicConv2d ends
    // in ReLU and the final linear in nothing; an up-projection adds scale * itself to the block input `res`, then ReLU or not
    Act fconv(const Act& x, int r, const Act* into = nullptr, const Act* res = nullptr, float scale = 0.f, bool relu = true) {
        const FnRow& g = trl_facenet_rows()[r];
        const FnW& t = c->fn[r];
        layer = g.name;
        return conv(x, t.w, t.bias, t.scale, t.shift, nullptr, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw,
                    g.kind == FN_LINEAR || !relu ? TRL_ACT_NONE : TRL_ACT_RELU, into, res, scale);
    }
    Act pool(const Act& x, int k, int st, int ceil_mode, const Act* into = nullptr) {
        const int OH = trl_pool_out(x.h, k, st, ceil_mode), OW = trl_pool_out(x.w, k, st, ceil_mode);
        Act y = into ? *into : alloc(x.n, OH, OW, x.c, x.bf);
        if (err != TRL_OK) return y;
        issue([&] {
            if (x.bf) return trl_launch_maxpool_bf16(reinterpret_cast<const uint16_t*>(x.p), x.n, x.h, x.w, x.c, x.ld, x.coff, k, st,
                                                     reinterpret_cast<uint16_t*>(y.p), y.ld, y.coff, OH, OW, s, c->cfg.embed_precision);
            return trl_launch_maxpool(x.p, x.n, x.h, x.w, x.c, x.ld, x.coff, k, st, ceil_mode, y.p, y.ld, y.coff, OH, OW, s, m_dev, m_base);
        });
        return y;
    }
};

// The blocks of InceptionResnetV1, each over the rows of FaceNet's table that start at r0.  The 1x1 branches that read the block
// input run as one fused conv (weights concatenated at load time); the concat buffer doubles as their scratch: a slice is only
// overwritten after its last reader has run.
Act block35(Runner& R, const Act& x, int r0) {
    Act cat = R.alloc(x.n, x.h, x.w, 96, x.bf);
    Act s1 = Runner::slice(cat, 32, 32), s2 = Runner::slice(cat, 64, 32);
    R.fconv(x, r0 + B35_FUSED, &cat);                // [branch0 | branch2.0 | branch1.0]
    Act b2 = R.fconv(s1, r0 + B35_B2_1);             // reads branch2.0 (cols 32:64)
    R.fconv(s2, r0 + B35_B1_1, &s1);                 // reads branch1.0 (64:96) -> final branch1 at 32:64
    R.fconv(b2, r0 + B35_B2_2, &s2);                 // final branch2 at 64:96
    return R.fconv(cat, r0 + B35_UP, nullptr, &x, 0.17f);
}
// The same block in 4 launches for the small-map conv family (f32, M <= 16384): the fused 1x1 scatters its columns into a
// 128-wide buffer W = [branch0 | (free) | branch2.0 | branch1.0], so the two independent 3x3s can share ONE launch without a
// hazard -- branch1.1 reads W[96:128] and writes the free slot W[32:64] (nobody reads it), branch2.1 reads W[64:96] into a
// temporary -- then branch2.2 writes W[64:96] and the up-projection reads W[0:96] = [branch0 | branch1 | branch2].
Act block35_grouped(Runner& R, const Act& x, int r0) {
    Act W = R.alloc(x.n, x.h, x.w, 128, false);
    Act w96 = Runner::slice(W, 0, 96);
    Act f1 = Runner::slice(W, 32, 32), f2 = Runner::slice(W, 64, 32), f3 = Runner::slice(W, 96, 32);
    R.ysplit = 32; R.yskip = 32;                     // columns >= 32 land 32 channels further right
    R.fconv(x, r0 + B35_FUSED, &w96);                // [branch0 | - | branch2.0 | branch1.0]
    R.ysplit = 1 << 30; R.yskip = 0;
    R.begin_group();
    Act b2 = R.fconv(f2, r0 + B35_B2_1);             // W[64:96] -> temporary
    R.fconv(f3, r0 + B35_B1_1, &f1);                 // W[96:128] -> W[32:64]
    R.end_group();
    R.fconv(b2, r0 + B35_B2_2, &f2);                 // -> W[64:96] (branch2.0 is dead)
    return R.fconv(w96, r0 + B35_UP, nullptr, &x, 0.17f);
}
// Block17 (two branches of 128, a 1x7 then a 7x1) and Block8 (of 192, 1x3 then 3x1): the same walk over rows of the same roles
Act block17_8(Runner& R, const Act& x, int r0, float scale, bool relu = true) {
    const int half = trl_facenet_rows()[r0 + B17_FUSED].cout / 2;
    Act cat = R.alloc(x.n, x.h, x.w, 2 * half, x.bf);
    Act s1 = Runner::slice(cat, half, half);
    R.fconv(x, r0 + B17_FUSED, &cat);                // [branch0 | branch1.0]
    Act a2 = R.fconv(s1, r0 + B17_B1_1);
    R.fconv(a2, r0 + B17_B1_2, &s1);
    return R.fconv(cat, r0 + B17_UP, nullptr, &x, scale, relu);
}

}  // namespace

// InceptionResnetV1.eval().forward (server/model.py:59)
int trl_run_facenet(trl_ctx* c, Arena& X, const float* d_faces, int n, int h, int w, const uint8_t* d_valid, float* d_emb, hipStream_t s, bool features) {
    if (n <= 0) return TRL_OK;
    Runner R{c, s, X};
    const bool check_only = X.counting;
    struct Disarm { trl_ctx* c; ~Disarm() { if (c) c->hook.fn_cap_arm = -1; } } disarm{check_only ? nullptr : c};   // a capture covers one call, whatever its outcome
    if (!check_only) {
        c->hook.fn_plan.clear();
        R.plan = &c->hook.fn_plan;
        if (c->hook.fn_cap_arm >= 0) for (auto& b : c->hook.fn_cap) b.dims[3] = 0;
    }
    const Act x0 = Act::dense(d_faces, n, h, w, 3);
    Act x = R.fconv(x0, FN_STEM + 0);                // conv2d_1a
    if (c->cfg.embed_precision >= 1) {   // everything after the 3-channel stem conv runs on 16-bit activations (trl_bf16.hip)
        Act xb = R.alloc(x.n, x.h, x.w, x.c, true);
        R.issue([&] { return trl_launch_to_bf16(x.p, x.pixels() * x.c, reinterpret_cast<uint16_t*>(xb.p), s, c->cfg.embed_precision); });
        x = xb;
    }
    x = R.fconv(x, FN_STEM + 1);                     // conv2d_2a
    x = R.fconv(x, FN_STEM + 2);                     // conv2d_2b
    x = R.pool(x, 3, 2, 0);
    x = R.fconv(x, FN_STEM + 3);                     // conv2d_3b
    x = R.fconv(x, FN_STEM + 4);                     // conv2d_4a
    x = R.fconv(x, FN_STEM + 5);                     // conv2d_4b
    if (R.err != TRL_OK) return R.err;
    if (x.h < 3 || x.w < 3) { trl_set_error("face crop %dx%d too small for InceptionResnetV1", h, w); return TRL_ERR_INVALID; }
    const bool small_f32 = !x.bf && (long long)x.n * x.h * x.w <= 16384 && g_trl_no_fnconv == 0;
    for (int i = 0; i < 5; i++) x = (small_f32 ? block35_grouped : block35)(R, x, FN_B35 + i * B35_ROWS);
    {   // Mixed_6a
        const int OH = (x.h - 3) / 2 + 1, OW = (x.w - 3) / 2 + 1;
        Act cat = R.alloc(n, OH, OW, 896, x.bf);
        Act s0 = Runner::slice(cat, 0, 384), s1 = Runner::slice(cat, 384, 256), s2 = Runner::slice(cat, 640, 256);
        R.fconv(x, FN_M6A + M6A_B0, &s0);
        Act a = R.fconv(x, FN_M6A + M6A_B1_0);
        Act a2 = R.fconv(a, FN_M6A + M6A_B1_1);
        R.fconv(a2, FN_M6A + M6A_B1_2, &s1);
        R.pool(x, 3, 2, 0, &s2);
        x = cat;
    }
    if (R.err != TRL_OK) return R.err;
    if (x.h < 3 || x.w < 3) { trl_set_error("face crop %dx%d too small for InceptionResnetV1", h, w); return TRL_ERR_INVALID; }
    for (int i = 0; i < 10; i++) x = block17_8(R, x, FN_B17 + i * B17_ROWS, 0.10f);
    {   // Mixed_7a
        const int OH = (x.h - 3) / 2 + 1, OW = (x.w - 3) / 2 + 1;
        Act cat = R.alloc(n, OH, OW, 1792, x.bf);
        Act s0 = Runner::slice(cat, 0, 384), s1 = Runner::slice(cat, 384, 256), s2 = Runner::slice(cat, 640, 256),
            s3 = Runner::slice(cat, 896, 896);
        Act t = R.fconv(x, FN_M7A + M7A_FUSED);      // [branch0.0 | branch1.0 | branch2.0]
        Act t0 = Runner::slice(t, 0, 256), t1 = Runner::slice(t, 256, 256), t2 = Runner::slice(t, 512, 256);
        R.begin_group();                             // three independent convs over slices of t: one launch
        R.fconv(t0, FN_M7A + M7A_B0_1, &s0);
        R.fconv(t1, FN_M7A + M7A_B1_1, &s1);
        Act a2 = R.fconv(t2, FN_M7A + M7A_B2_1);
        R.end_group();
        R.fconv(a2, FN_M7A + M7A_B2_2, &s2);
        R.pool(x, 3, 2, 0, &s3);
        x = cat;
    }
    for (int i = 0; i < 5; i++) x = block17_8(R, x, FN_B8 + i * B17_ROWS, 0.20f);
    x = block17_8(R, x, FN_B8 + 5 * B17_ROWS, 1.0f, false);   // block8: no ReLU
    if (R.err != TRL_OK) return R.err;
    // avgpool_1a -> last_linear (no bias) -> last_bn (folded) -> F.normalize
    Act g;
    if (!x.bf && x.h * x.w == 1 && x.coff == 0 && x.ld == x.c) {
        g = x;                                   // a 1x1 map IS its average (sum of one element / 1.0f, exact): no kernel
    } else {
        g = R.alloc(n, 1, 1, x.c);
        R.issue([&] {
            if (x.bf) return trl_launch_gap_bf16(reinterpret_cast<const uint16_t*>(x.p), n, x.h * x.w, x.c, g.p, s, c->cfg.embed_precision);
            return trl_launch_gap(x.p, n, x.h * x.w, x.c, g.p, s);
        });
    }
    Act e = R.fconv(g, FN_LAST);
    // (features: the walk ends in front of the normalisation -- trl_facenet_features, what the logits layer reads)
    R.issue([&] { return features ? trl_launch_feat512(e.p, d_valid, n, d_emb, s) : trl_launch_l2norm512(e.p, d_valid, n, d_emb, s); });
    return R.err;
}

// The one walker of the MTCNN nets (contract: trl_ctx.h)
int trl_run_net(trl_ctx* c, Arena& X, const NetDesc& d, int first, const Act& x0, float* d_out, hipStream_t s, const int32_t* m_dev, int m_base) {
    if (x0.n <= 0) return TRL_OK;
    Runner R{c, s, X};
    R.m_dev = m_dev; R.m_base = m_base;
    if (c->hook.mt_plan_arm) { R.plan = &c->hook.mt_plan; R.nconv = (int)c->hook.mt_plan.size(); }   // trl_debug_stage_net: rows of every chunk
    const NetLayerW* lw = c->mt[&d - trl_nets];
    Act x = x0;
    for (int i = first; i < d.nl; i++) {
        const NetLayer& L = d.layer[i];
        if (!L.name) { x = R.pool(x, L.k, L.st, 1); continue; }
        char layer[32];                  // (a conv of this walk is launched, and its plan row written, inside R.conv)
        if (R.plan) { snprintf(layer, sizeof layer, "%s.%s", d.name, L.name); R.layer = layer; }
        // a pool directly behind the conv runs in the conv's epilogue where the kernel has one: the 128-row tiles of R-Net conv2 and
        // O-Net conv2 / conv3 at production capacities (smaller launches, PNet and every other pool: separate launches as below)
        if (c->opt.tail_pool && i + 2 < d.nl && !d.layer[i + 1].name &&
            R.conv_pool(x, lw[i], L.k, L.prelu ? TRL_ACT_PRELU : TRL_ACT_NONE, d.layer[i + 1].k, d.layer[i + 1].st, &x)) {
            i++;
            continue;
        }
        const Act out = Act::dense(d_out, x.n, x.h - L.k + 1, x.w - L.k + 1, d.nout);
        x = R.conv(x, lw[i].w, lw[i].b, nullptr, nullptr, lw[i].slope, L.k, L.k, 1, 1, 0, 0, L.prelu ? TRL_ACT_PRELU : TRL_ACT_NONE,
                   i == d.nl - 1 ? &out : nullptr, nullptr, 0.f);
    }
    return R.err;
}

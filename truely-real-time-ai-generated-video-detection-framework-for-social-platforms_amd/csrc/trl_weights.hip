// trl_weights.hip -- the device half of trl_load_weights: upload what trl_weights.h staged, turn its offsets into the pointers the
// walkers use (c->wmat, c->fn, c->mt, the logits pair), make the 16-bit copies.  The name -> tensor directory lives in
// trl_load_weights alone: no call after it looks a tensor up by name.
#include "trl_ctx.h"
#include "trl_weights.h"

static_assert(TRL_STAGE_REFUSED == TRL_ERR_WEIGHTS, "a refused blob is TRL_ERR_WEIGHTS");

void trl_free_weights(trl_ctx* c) {
    c->have_weights = false;
    for (DevW& w : c->wmat) if (w.pt) (void)hipFree(w.pt);
    c->wmat.clear();
    if (c->wdev) (void)hipFree(c->wdev);
    c->wdev = nullptr; c->wbytes = 0;
    c->logits_w = nullptr; c->logits_b = nullptr; c->num_classes = 0;
}

// Every tensor trl_nets[] names exists with the shape its layer gives it -- K = k k Cin, cout columns, cout biases and slopes --
// and is resolved into c->mt; then what the kernels choose by: the conv1 slope class of the front kernel
static int trl_resolve_nets(trl_ctx* c, const StagedWeights& st) {
    auto vec = [&](int item) { return (const float*)(c->wdev + st.items[item].off); };
    for (int id = 0; id < 3; id++) {
        const NetDesc& d = trl_nets[id];
        int cin = 3;
        for (int i = 0; i < d.nl; i++) {
            const NetLayer& L = d.layer[i];
            c->mt[id][i] = NetLayerW();
            if (!L.name) continue;
            const std::string net = std::string(d.name) + ".", base = net + L.name;
            const int w = st.need(base + ".w", true), b = st.need(base + ".b", false), sl = L.prelu ? st.need(net + L.prelu, false) : -1;
            if (w < 0 || b < 0 || (L.prelu && sl < 0)) return TRL_ERR_WEIGHTS;   // (need() named it)
            const StagedTensor& W = st.items[w];
            if (W.K != L.k * L.k * cin || W.Cout != L.cout) {
                trl_set_error("tensor '%s.w' is [%d][%d], its layer needs [%d][%d]", base.c_str(), W.K, W.Cout, L.k * L.k * cin, L.cout);
                return TRL_ERR_WEIGHTS;
            }
            const int bn = st.items[b].n, sn = sl < 0 ? L.cout : st.items[sl].n;
            if (bn != L.cout || sn != L.cout) {
                trl_set_error("tensor '%s' has %d elements, its layer %d channels", bn != L.cout ? (base + ".b").c_str() : (net + L.prelu).c_str(),
                              bn != L.cout ? bn : sn, L.cout);
                return TRL_ERR_WEIGHTS;
            }
            c->mt[id][i] = NetLayerW{&c->wmat[w], vec(b), sl < 0 ? nullptr : vec(sl)};
            cin = L.cout;
        }
        if (d.side) c->front_mode[id] = trl_front_slope_class(trl_host_of(c, st.image.data(), c->mt[id][0].slope), d.layer[0].cout);
    }
    return TRL_OK;
}

extern "C" int trl_load_weights(trl_ctx* c, const void* blob, size_t nbytes) {
    if (!c || !blob) { trl_set_error("null argument"); return TRL_ERR_INVALID; }
    TRL_HIP(hipSetDevice(c->cfg.device));
    TRL_HIP(hipDeviceSynchronize());               // nothing queued still reads the weights this load replaces
    trl_free_weights(c);                           // (a refused blob leaves the context without weights)
    StagedWeights st;
    TRL_CHECK(trl_stage_weights(blob, nbytes, c->cfg.embed_precision, &st));
    TRL_HIP(hipMalloc((void**)&c->wdev, st.total));
    TRL_HIP(hipMemcpy(c->wdev, st.image.data(), st.total, hipMemcpyHostToDevice));
    c->wbytes = st.total;

    // Every tensor the four nets use is resolved here, never at a call.  c->wmat[i] is the directory's item i where that is a
    // matrix (a vector's stays empty); it has its size before anything points into it.
    c->wmat.resize(st.items.size());
    for (size_t i = 0; i < st.items.size(); i++) {
        const StagedTensor& t = st.items[i];
        if (!t.mat) continue;
        DevW& w = c->wmat[i];
        w.p = (float*)(c->wdev + t.off); w.K = t.K; w.Cout = t.Cout; w.Kpad = t.Kpad; w.ld = t.ld;
    }
    auto vec = [&](int item) { return item < 0 ? nullptr : (const float*)(c->wdev + st.items[item].off); };
    const FnRow* rows = trl_facenet_rows();
    for (int r = 0; r < FN_ROWS; r++) {
        const bool bias = rows[r].kind == FN_RESID;
        c->fn[r] = FnW{&c->wmat[st.fn[r].w], bias ? nullptr : vec(st.fn[r].v[0]), bias ? nullptr : vec(st.fn[r].v[1]), bias ? vec(st.fn[r].v[0]) : nullptr};
    }
    // what the MTCNN kernels choose by (slope classes, the conv3 screen bound) comes from the host image
    TRL_CHECK(trl_resolve_nets(c, st));
    TRL_CHECK(trl_pnet_prepare(c, st.image.data()));
    if (st.logits_w >= 0) {
        c->logits_w = &c->wmat[st.logits_w];
        c->logits_b = vec(st.logits_b);
        c->num_classes = c->logits_w->Cout;
    }
    // One walk of the embedder over a counting arena, on one 160 x 160 face: the walker and the table agree (conv() checks each
    // input view against the row's K = kh kw cin and each `into` view against its cout, which the staging checked the tensors by)
    Arena count = Arena::counter(c->scratch.guard);
    TRL_CHECK(trl_run_facenet(c, count, nullptr, 1, 160, 160, nullptr, nullptr, nullptr));
    c->fn_need_key[0] = 0;
    if (c->cfg.embed_precision >= 1) {   // bf16 / fp16 copies of the embedder's conv weights (all rows but the f32-only ones)
        for (int r = 0; r < FN_ROWS; r++)
            if (!rows[r].f32_only) TRL_CHECK(trl_make_weight_bf16(&c->wmat[st.fn[r].w], nullptr, c->cfg.embed_precision));
        TRL_HIP(hipDeviceSynchronize());
    }
    c->have_weights = true;
    return TRL_OK;
}

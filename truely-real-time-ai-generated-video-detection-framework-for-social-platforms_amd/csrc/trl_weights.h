// trl_weights.h -- the host half of trl_load_weights: a "TRLW0001" blob (weights.py) and embed_precision -> a refusal (status and
// trl_set_error's text) or the directory of tensors, the host image the device receives byte for byte, and FaceNet's rows resolved.
//
// Plain C++17, no HIP: trl_weights.hip uploads what this stages, tests/weights_sim.cpp drives it on a CPU.  Every name and shape is
// checked before anything is copied, so a refusal costs one pass over the directory.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "trl_facenet.h"

void trl_set_error(const char* fmt, ...);   // the library's is in trl_api.hip; a host program supplies its own
constexpr int TRL_STAGE_REFUSED = -3;       // TRL_ERR_WEIGHTS (include/truely_hip.h)

struct TrlwEntry {    // one directory entry of the blob
    char name[56];
    uint32_t ndim;
    uint32_t dims[4];
    uint64_t offset;
    uint64_t nbytes;
};
static_assert(sizeof(TrlwEntry) == 96, "TRLW entry layout");

// A matrix [K][Cout] lies in the image as [Kpad = ceil16(K)][ld = ceil32(Cout)], a vector of n floats in ceil128(n), zero padded;
// every tensor starts at a multiple of 256 bytes.
struct StagedTensor {
    std::string name;
    bool mat;
    int K, Cout, Kpad, ld;   // matrix
    int n;                   // vector
    size_t off;              // in the image
    const uint8_t* src;      // its floats in the blob, dense; null: a fusion, built from parts[] (columns side by side)
    std::vector<int> parts;
};
struct StagedWeights {
    std::vector<StagedTensor> items;                 // the blob's tensors in directory order, then the fusions
    std::unordered_map<std::string, int> index;      // name -> items[] (the last entry of a name wins)
    std::vector<char> image;
    struct { int w, v[2]; } fn[FN_ROWS];             // items[] of each FaceNet row: matrix; scale, shift or bias, -1
    int logits_w = -1, logits_b = -1;                // the optional classifier pair, or -1

    size_t total = 0;
    int add(StagedTensor t) {
        const size_t floats = t.mat ? (size_t)t.Kpad * t.ld : (size_t)((t.n + 127) / 128 * 128);
        t.off = total;
        total += (floats * 4 + 255) & ~(size_t)255;
        index[t.name] = (int)items.size();
        items.push_back(std::move(t));
        return (int)items.size() - 1;
    }
    int add_mat(const std::string& name, int K, int Cout, const uint8_t* src) {
        return add({name, true, K, Cout, (K + 15) / 16 * 16, (Cout + 31) / 32 * 32, 0, 0, src, {}});
    }
    int add_vec(const std::string& name, int n, const uint8_t* src) { return add({name, false, 0, 0, 0, 0, n, 0, src, {}}); }
    int find(const std::string& name) const {
        auto it = index.find(name);
        return it == index.end() ? -1 : it->second;
    }
    // a tensor some layer needs: a miss names it
    int need(const std::string& name, bool mat) const {
        const int i = find(name);
        if (i < 0 || items[i].mat != mat) { trl_set_error("weight %s '%s' not loaded", mat ? "matrix" : "vector", name.c_str()); return -1; }
        return i;
    }

    // Convs that read the same input run as ONE conv: out + ".w" = the parts' matrices side by side (same K), out + suffix = their
    // per-column vectors likewise, for every suffix.  Each output column keeps its own fmaf chain, so results are unchanged.
    bool fuse(const std::string& out, const char* const* part, int nparts, const char* const* suffix, int nsuffix) {
        std::vector<int> pw;
        std::vector<std::vector<int>> pv(nsuffix);
        int K = -1, tot = 0;
        for (int p = 0; p < nparts; p++) {
            const std::string base = part[p];
            const int w = find(base + ".w");
            if (w < 0 || !items[w].mat) { trl_set_error("missing tensor %s.w", part[p]); return false; }
            if (K < 0) K = items[w].K;
            if (K != items[w].K) { trl_set_error("%s.w: the convs merged into %s disagree on K", part[p], out.c_str()); return false; }
            for (int s = 0; s < nsuffix; s++) {
                const int v = find(base + suffix[s]);
                if (v < 0) { trl_set_error("missing tensor %s%s", part[p], suffix[s]); return false; }
                if (items[v].mat || items[v].n != items[w].Cout) { trl_set_error("tensor %s%s has an unexpected shape", part[p], suffix[s]); return false; }
                pv[s].push_back(v);
            }
            pw.push_back(w);
            tot += items[w].Cout;
        }
        items[add_mat(out + ".w", K, tot, nullptr)].parts = pw;
        for (int s = 0; s < nsuffix; s++) items[add_vec(out + suffix[s], tot, nullptr)].parts = pv[s];
        return true;
    }

    // The tensors of FaceNet's rows, with the shapes the table gives them
    bool resolve_facenet() {
        const FnRow* rows = trl_facenet_rows();
        for (int r = 0; r < FN_ROWS; r++) {
            const FnRow& g = rows[r];
            const std::string wname = std::string(g.name) + ".w";
            const int w = need(wname, true);
            if (w < 0) return false;
            if (items[w].K != g.kh * g.kw * g.cin || items[w].Cout != g.cout) {
                trl_set_error("tensor '%s' is [%d][%d], its layer needs [%d][%d]", wname.c_str(), items[w].K, items[w].Cout, g.kh * g.kw * g.cin, g.cout);
                return false;
            }
            fn[r].w = w; fn[r].v[0] = fn[r].v[1] = -1;
            int ns;
            const char* const* sfx = trl_facenet_vec_suffixes(g, &ns);
            for (int s = 0; s < ns; s++) {
                const std::string vname = std::string(trl_facenet_vec_base(g)) + sfx[s];
                const int v = need(vname, false);
                if (v < 0) return false;
                if (items[v].n != g.cout) { trl_set_error("weight vector '%s' has %d elements, its conv %d columns", vname.c_str(), items[v].n, g.cout); return false; }
                fn[r].v[s] = v;
            }
        }
        return true;
    }

    // InceptionResnetV1's classifier is optional (a blob packed from a checkpoint without `logits`, or with include_logits=False):
    // both tensors or neither, w [512][C] and b [C], 1 <= C <= 65535 (the kernel's grid.y carries the class groups)
    bool resolve_logits() {
        const char* const wn = "facenet.logits.w";
        const char* const bn = "facenet.logits.b";
        const int w = find(wn), b = find(bn);
        if (w < 0 && b < 0) return true;
        if (w < 0) { trl_set_error("missing tensor %s (the blob holds %s)", wn, bn); return false; }
        if (b < 0) { trl_set_error("missing tensor %s (the blob holds %s)", bn, wn); return false; }
        if (!items[w].mat || items[w].K != 512 || items[w].Cout > 65535) { trl_set_error("tensor '%s' must be [512][C] with 1 <= C <= 65535", wn); return false; }
        if (items[b].mat || items[b].n != items[w].Cout) { trl_set_error("tensor '%s' must hold the %d biases of %s", bn, items[w].Cout, wn); return false; }
        logits_w = w; logits_b = b;
        return true;
    }

    void build_image() {
        image.assign(total, 0);
        for (const StagedTensor& t : items) {
            char* dst = image.data() + t.off;
            if (t.src && t.mat) for (int k = 0; k < t.K; k++) memcpy(dst + (size_t)k * t.ld * 4, t.src + (size_t)k * t.Cout * 4, (size_t)t.Cout * 4);
            else if (t.src) memcpy(dst, t.src, (size_t)t.n * 4);
            size_t col = 0;
            for (int pi : t.parts) {          // (a fusion: its parts came straight from the blob)
                const StagedTensor& p = items[pi];
                if (t.mat) for (int k = 0; k < t.K; k++) memcpy(dst + ((size_t)k * t.ld + col) * 4, p.src + (size_t)k * p.Cout * 4, (size_t)p.Cout * 4);
                else memcpy(dst + col * 4, p.src, (size_t)p.n * 4);
                col += t.mat ? p.Cout : p.n;
            }
        }
    }
    const float* host(int item) const { return (const float*)(image.data() + items[item].off); }
};

// -> 0, or TRL_STAGE_REFUSED with the reason in trl_set_error.  The blob must outlive the call only.
inline int trl_stage_weights(const void* blob, size_t nbytes, int embed_precision, StagedWeights* st) {
    *st = StagedWeights();
    const uint8_t* b = (const uint8_t*)blob;
    if (nbytes < 16 || memcmp(b, "TRLW0001", 8) != 0) { trl_set_error("bad weights blob magic"); return TRL_STAGE_REFUSED; }
    uint32_t nt;
    memcpy(&nt, b + 8, 4);
    if (16 + (size_t)nt * sizeof(TrlwEntry) > nbytes) { trl_set_error("truncated weights blob"); return TRL_STAGE_REFUSED; }
    for (uint32_t i = 0; i < nt; i++) {
        TrlwEntry e;
        memcpy(&e, b + 16 + (size_t)i * sizeof e, sizeof e);
        if (e.offset > nbytes || e.nbytes > nbytes - e.offset || (e.offset & 3)) { trl_set_error("tensor out of blob bounds"); return TRL_STAGE_REFUSED; }
        if (e.ndim != 1 && e.ndim != 2) continue;
        const std::string name(e.name, strnlen(e.name, sizeof e.name));
        // the declared shape must account for exactly the bytes the entry owns (the copies trust the shape)
        const uint64_t elems = e.ndim == 2 ? (uint64_t)e.dims[0] * e.dims[1] : (uint64_t)e.dims[0];
        if (elems == 0 || elems > (1ull << 31) || elems * 4 != e.nbytes) {
            trl_set_error("tensor '%s': shape and byte count disagree", name.c_str());
            return TRL_STAGE_REFUSED;
        }
        if (e.ndim == 2) st->add_mat(name, (int)e.dims[0], (int)e.dims[1], b + e.offset);
        else st->add_vec(name, (int)e.dims[0], b + e.offset);
    }
    const FnRow* rows = trl_facenet_rows();
    for (int r = 0; r < FN_ROWS; r++) {
        const FnRow& g = rows[r];
        if (!g.nparts) continue;
        const char* part[3] = {g.part[0], g.part[1], g.part[2]};
        int ns;
        const char* const* sfx = trl_facenet_vec_suffixes(g, &ns);
        if (!st->fuse(g.name, part, g.nparts, sfx, ns)) return TRL_STAGE_REFUSED;
    }
    // merged heads: the 1x1 class and regression (and landmark) convs of each MTCNN net as one [K][6] / [K][16] matrix
    static const char* const heads[3][4] = {{"pnet.heads", "pnet.conv4_1", "pnet.conv4_2", nullptr},
                                            {"rnet.heads", "rnet.dense5_1", "rnet.dense5_2", nullptr},
                                            {"onet.heads", "onet.dense6_1", "onet.dense6_2", "onet.dense6_3"}};
    static const char* const bias[1] = {".b"};
    for (auto& h : heads)
        if (!st->fuse(h[0], h + 1, h[3] ? 3 : 2, bias, 1)) return TRL_STAGE_REFUSED;
    if (!st->resolve_logits() || !st->resolve_facenet()) return TRL_STAGE_REFUSED;
    st->build_image();
    if (embed_precision == 2) {   // an fp16 conv weight that rounds past +-65504 would become inf: refuse the blob instead
        for (int r = 0; r < FN_ROWS; r++) {
            if (rows[r].f32_only) continue;
            const StagedTensor& t = st->items[st->fn[r].w];
            const float* w = st->host(st->fn[r].w);
            for (int k = 0; k < t.K; k++)
                for (int j = 0; j < t.Cout; j++)
                    if (!(fabsf(w[(size_t)k * t.ld + j]) < 65520.f)) {   // 65520 is the rounding midpoint to the next (infinite) binade; NaN fails too
                        trl_set_error("weight %s[%zu] = %g is outside the fp16 range", t.name.c_str(), (size_t)k * t.Cout + j, w[(size_t)k * t.ld + j]);
                        return TRL_STAGE_REFUSED;
                    }
        }
    }
    return 0;
}

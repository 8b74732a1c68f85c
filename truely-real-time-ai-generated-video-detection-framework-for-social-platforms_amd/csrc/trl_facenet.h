// trl_facenet.h -- InceptionResnetV1 described once: one row per conv launch of the walk (trl_run_facenet), in walk order.
//
// Plain C++17, no HIP: the walker (trl_nets.hip), the weight staging (trl_weights.h) and tests/weights_sim.cpp read the same
// table.  A row's index is the `conv` index of trl_debug_facenet_plan and the index trl_debug_facenet_capture arms.
// Architecture: facenet_pytorch 2.6.0, InceptionResnetV1 (the Python packer's names, weights.py, behind "facenet.").
#pragma once
#include <stdio.h>

enum { FN_BASIC = 0,     // BasicConv2d: conv without bias, folded batch norm (<name>.scale / .shift), ReLU
       FN_RESID = 1,     // residual up-projection of a block: 1x1 conv with bias (<name>.b); scale and ReLU are the block's
       FN_LINEAR = 2 };  // last_linear without bias, then last_bn folded (facenet.last_bn.scale / .shift)

struct FnRow {
    char name[48];               // canonical name: the matrix is <name>.w, the plan's layer is <name>
    int kh, kw, sh, sw, ph, pw, cin, cout;
    int kind;
    int nparts;                  // > 0: a fused conv -- the columns of these convs side by side, in this order (built at load)
    char part[3][48];
    bool f32_only;               // keeps f32 operands when embed_precision is bf16 / fp16
};

// Rows of a block, from the index the block is given.  Both forms of block35 issue their five rows in this order.
enum { B35_FUSED, B35_B2_1, B35_B1_1, B35_B2_2, B35_UP, B35_ROWS };   // fused = [branch0 | branch2.0 | branch1.0]
enum { B17_FUSED, B17_B1_1, B17_B1_2, B17_UP, B17_ROWS };             // fused = [branch0 | branch1.0]; block8 has the same rows
enum { M6A_B0, M6A_B1_0, M6A_B1_1, M6A_B1_2, M6A_ROWS };
enum { M7A_FUSED, M7A_B0_1, M7A_B1_1, M7A_B2_1, M7A_B2_2, M7A_ROWS };  // fused = [branch0.0 | branch1.0 | branch2.0]
enum { FN_STEM = 0, FN_STEM_ROWS = 6,
       FN_B35 = FN_STEM + FN_STEM_ROWS,       // repeat_1.0 .. 4
       FN_M6A = FN_B35 + 5 * B35_ROWS,
       FN_B17 = FN_M6A + M6A_ROWS,            // repeat_2.0 .. 9
       FN_M7A = FN_B17 + 10 * B17_ROWS,
       FN_B8 = FN_M7A + M7A_ROWS,             // repeat_3.0 .. 4, then block8
       FN_LAST = FN_B8 + 6 * B17_ROWS,
       FN_ROWS = FN_LAST + 1 };
static_assert(FN_ROWS == 105, "6 + 5*5 + 4 + 10*4 + 5 + 6*4 + 1 convs");

struct FnTable {
    FnRow row[FN_ROWS];
    int n = 0;
    // block.leaf: a kh x kw conv, stride s, padding ph / pw
    FnRow& conv(const char* block, const char* leaf, int kh, int kw, int s, int ph, int pw, int cin, int cout, int kind = FN_BASIC) {
        FnRow& r = row[n++];
        r = FnRow();
        snprintf(r.name, sizeof r.name, "facenet.%s%s%s", block, block[0] ? "." : "", leaf);
        r.kh = kh; r.kw = kw; r.sh = r.sw = s; r.ph = ph; r.pw = pw; r.cin = cin; r.cout = cout; r.kind = kind;
        return r;
    }
    // block.fused: the 1x1 branches of a block that read its input, as one conv of cout columns in all
    void fused(const char* block, int cin, int cout, const char* p0, const char* p1, const char* p2 = nullptr) {
        FnRow& r = conv(block, "fused", 1, 1, 1, 0, 0, cin, cout);
        for (const char* p : {p0, p1, p2})
            if (p) snprintf(r.part[r.nparts++], sizeof r.part[0], "facenet.%s.%s", block, p);
    }
    void up(const char* block, int cin, int cout) { conv(block, "conv2d", 1, 1, 1, 0, 0, cin, cout, FN_RESID); }
    FnTable() {
        char b[16];
        conv("", "conv2d_1a", 3, 3, 2, 0, 0, 3, 32).f32_only = true;       // 3 input channels: no 16-bit kernel takes it
        conv("", "conv2d_2a", 3, 3, 1, 0, 0, 32, 32);
        conv("", "conv2d_2b", 3, 3, 1, 1, 1, 32, 64);
        conv("", "conv2d_3b", 1, 1, 1, 0, 0, 64, 80);
        conv("", "conv2d_4a", 3, 3, 1, 0, 0, 80, 192);
        conv("", "conv2d_4b", 3, 3, 2, 0, 0, 192, 256);
        for (int i = 0; i < 5; i++) {                                      // Block35 x 5
            snprintf(b, sizeof b, "repeat_1.%d", i);
            fused(b, 256, 96, "branch0", "branch2.0", "branch1.0");
            conv(b, "branch2.1", 3, 3, 1, 1, 1, 32, 32);
            conv(b, "branch1.1", 3, 3, 1, 1, 1, 32, 32);
            conv(b, "branch2.2", 3, 3, 1, 1, 1, 32, 32);
            up(b, 96, 256);
        }
        conv("mixed_6a", "branch0", 3, 3, 2, 0, 0, 256, 384);
        conv("mixed_6a", "branch1.0", 1, 1, 1, 0, 0, 256, 192);
        conv("mixed_6a", "branch1.1", 3, 3, 1, 1, 1, 192, 192);
        conv("mixed_6a", "branch1.2", 3, 3, 2, 0, 0, 192, 256);
        for (int i = 0; i < 10; i++) {                                     // Block17 x 10
            snprintf(b, sizeof b, "repeat_2.%d", i);
            fused(b, 896, 256, "branch0", "branch1.0");
            conv(b, "branch1.1", 1, 7, 1, 0, 3, 128, 128);
            conv(b, "branch1.2", 7, 1, 1, 3, 0, 128, 128);
            up(b, 256, 896);
        }
        fused("mixed_7a", 896, 768, "branch0.0", "branch1.0", "branch2.0");
        conv("mixed_7a", "branch0.1", 3, 3, 2, 0, 0, 256, 384);
        conv("mixed_7a", "branch1.1", 3, 3, 2, 0, 0, 256, 256);
        conv("mixed_7a", "branch2.1", 3, 3, 1, 1, 1, 256, 256);
        conv("mixed_7a", "branch2.2", 3, 3, 2, 0, 0, 256, 256);
        for (int i = 0; i < 6; i++) {                                      // Block8 x 5, then the one without ReLU
            if (i < 5) snprintf(b, sizeof b, "repeat_3.%d", i); else snprintf(b, sizeof b, "block8");
            fused(b, 1792, 384, "branch0", "branch1.0");
            conv(b, "branch1.1", 1, 3, 1, 0, 1, 192, 192);
            conv(b, "branch1.2", 3, 1, 1, 1, 0, 192, 192);
            up(b, 384, 1792);
        }
        conv("", "last_linear", 1, 1, 1, 0, 0, 1792, 512, FN_LINEAR).f32_only = true;   // f32 on the pooled features
    }
};
inline const FnRow* trl_facenet_rows() {
    static const FnTable t;      // built once; the names live as long as the library
    return t.row;
}
// The per-column vectors of a row: <base><suffix> for each suffix
inline const char* trl_facenet_vec_base(const FnRow& r) { return r.kind == FN_LINEAR ? "facenet.last_bn" : r.name; }
inline const char* const* trl_facenet_vec_suffixes(const FnRow& r, int* n) {
    static const char* const bn[2] = {".scale", ".shift"};
    static const char* const bias[1] = {".b"};
    *n = r.kind == FN_RESID ? 1 : 2;
    return r.kind == FN_RESID ? bias : bn;
}

// trl_pyramid.h -- what the image pyramid (trl_pyramid.hip) and its one reader, the fused PNet (trl_pnet.hip), share: the pixel,
// the per-level geometry and the host interface.  Internal: included by those two files only.
#pragma once
#include "trl_ctx.h"

// One pyramid pixel = three floats (a fourth padding float would be 25 % of the pyramid's write + read traffic).
struct PyrPx { float b, g, r; };
typedef float f32x3_nt __attribute__((ext_vector_type(3), aligned(4)));   // ... as it is stored and loaded

// Where a level lies and how its bins are normalised: all that the streaming pass needs of a level.
struct PyrBins {
    int h, w;                // level size
    int pix0;                // pixel offset of the level inside a frame's pyramid
    int pix_pad;             // h*w rounded up to 64 (pyramid slots of the level)
    int ytab0, xtab0;        // offsets of the level's row / column bin-edge tables
    int khA, kwA;            // adaptive-pool bins of the level are khA or khA+1 rows (kwA / kwA+1 columns)
    int fastdiv;             // bin sizes small enough for the exhaustively verified reciprocal division
    float rkh[2], rkw[2];    // RN(1/khA), RN(1/(khA+1)), same for kw: reciprocal division (see pyr_div)
};
// ... and what the per-pixel kernels (per-level and fine pass) read besides.
struct PyrLevel : PyrBins {
    int khmax, kwmax;        // the larger of the level's two bin sizes when it occurs
    int mode, gshift;        // per-level kernel path, log2(lanes per pixel)
    int nd, grshift;         // re-aligned dwords per row (mode 0), log2 groups per row (mode 1)
    unsigned wmagic, hmagic; // ceil(2^32 / w), ceil(2^32 / h): pixel / w by __umulhi; bin edges by multiply-high when 'arith' (no table
    int arith;               // load in the dependent-latency chain of a pixel): requires H*h*h < 2^32 and W*w*w < 2^32
    unsigned vmA[4], vmB[4]; // mode 0: valid-byte masks of the 4 re-aligned dwords of a row for bins kwA / kwA+1 wide
};
struct PyrLayout {
    int L;                   // levels (1..16)
    long long pyr_stride;    // pixels per frame: the sum of pix_pad
    PyrLevel lv[16];
};

// Levels of an H x W frame, their places in a frame's pyramid and their bin geometry: host arithmetic, no device work.
int trl_pyramid_layout(trl_ctx* c, int H, int W, PyrLayout& lay);
inline size_t trl_pyramid_bytes(const PyrLayout& lay, int n) { return (size_t)lay.pyr_stride * n * sizeof(PyrPx); }
// The pyramid of all n frames in c->scratch (production path of the fused PNet and of the debug exports): fills `lay`, returns
// the workspace in *pyr; ev[0..1], when given, bracket the pyramid kernels on s.
int trl_pyramid_build(trl_ctx* c, const uint8_t* d_frames, int n, int H, int W, PyrLayout& lay, PyrPx** pyr, hipEvent_t* ev, hipStream_t s);

// trl_gallery_bins.h -- the bin of a score among E threshold candidates, for host and device alike: the
// histogram kernel and tests/gallery_bins_main.cpp run this code.
//
// edges[0..E): float32, strictly ascending, no NaN (+-inf allowed), 1 <= E <= TRL_GL_MAX_EDGES.
//   cosine      bin = #{e : edges[e] <= score}
//   euclidean   bin = #{e : edges[e] <  score}
// Both lie in 0..E; a NaN score goes to slot E + 1.  The sides are those of the shipped predicates, so that cumulative sums of
// bin counts ARE the predicates' counts at every edge:
//   cosine accepts    score >= edges[e]  <=>  bin > e
//   euclidean accepts score <= edges[e]  <=>  bin <= e
// Comparisons are plain float32: -0 == +0.
#pragma once
#include "trl_gallery_order.h"

enum { TRL_GL_MAX_EDGES = 1023, TRL_GL_PAIRS_ALL = 0, TRL_GL_PAIRS_UPPER = 1 };

// ceil(log2(E + 1)): the trips of the search below
TRL_HD int trl_gl_bin_steps(int E) {
    int s = 0;
    while ((1 << s) < E + 1) s++;
    return s;
}

// The count is built from its highest bit down: `steps` trips whatever the score, and an edge is read only at an index below E, so
// edges that are not sorted give an unspecified bin in 0..E but never a read out of bounds.
TRL_HD int trl_gl_bin_in(int metric, float score, const float* edges, int E, int steps) {
    if (score != score) return E + 1;
    int bin = 0;
    for (int s = steps - 1; s >= 0; s--) {
        const int t = bin + (1 << s);
        const float e = edges[(t <= E ? t : 1) - 1];
        const bool below = metric == TRL_GL_COSINE ? e <= score : e < score;
        bin = t <= E && below ? t : bin;
    }
    return bin;
}

TRL_HD int trl_gl_bin(int metric, float score, const float* edges, int E) {
    return trl_gl_bin_in(metric, score, edges, E, trl_gl_bin_steps(E));
}

// The same search over a PADDED copy of the edges: padded[0..E) are the edges and padded[E .. (1 << steps) - 1) hold +inf, so no trip
// needs an index guard and the running count takes its bits by OR.  A pad is never < a score and is <= only a score of +inf, whose
// count the last line brings back to E.  The histogram kernel runs this one with steps = TRL_GL_MAX_STEPS and the metric a constant:
// a trip is one read at a constant offset from the running count, a comparison and a select.
enum { TRL_GL_MAX_STEPS = 10, TRL_GL_PADDED_EDGES = (1 << TRL_GL_MAX_STEPS) - 1 };

TRL_HD int trl_gl_bin_padded(int metric, float score, const float* padded, int E, int steps) {
    if (score != score) return E + 1;
    int bin = 0;
    for (int s = steps - 1; s >= 0; s--) {
        const float e = padded[(bin | (1 << s)) - 1];
        const bool below = metric == TRL_GL_COSINE ? e <= score : e < score;
        bin |= below ? 1 << s : 0;
    }
    return bin < E ? bin : E;
}

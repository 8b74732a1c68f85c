// trl_gallery_order.h -- the order of gallery matches and the two list operations built on it, for host and
// device alike: the search kernel's per-row lists, the merge kernel and tests/gallery_order_main.cpp run this code.
//
// A match is (score, gallery index).  a comes before b when
//   * a's score is not NaN and b's is, or
//   * neither is NaN and a's score is better (metric 0, cosine: larger; metric 1, euclidean: smaller), or
//   * the scores are equal as floats (-0 == +0), or both NaN, and a's index is lower.
// Indices are distinct, so the order is total.  An empty slot is (NaN, TRL_GL_EMPTY): it comes after every match, because no
// gallery index reaches 2^31 - 1 (m <= 2^31 - 1).  What the caller sees in an empty slot is (NaN, -1).
#pragma once
#include <stdint.h>

#include "trl_hd.h"

enum { TRL_GL_COSINE = 0, TRL_GL_EUCLIDEAN = 1, TRL_GL_MAX_K = 16 };
#define TRL_GL_EMPTY 0x7fffffff

struct TrlGlEntry {
    float score;
    int32_t index;
};

TRL_HD TrlGlEntry trl_gl_empty() {
    TrlGlEntry e;
    e.score = __builtin_nanf("");
    e.index = TRL_GL_EMPTY;
    return e;
}

// a comes before b
TRL_HD bool trl_gl_before(int metric, float sa, int32_t ia, float sb, int32_t ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return metric == TRL_GL_COSINE ? sa > sb : sa < sb;
    return ia < ib;
}

// list[0..k): matches in order, empty slots last.  Puts (score, index) where it belongs and drops the last entry; false, and the
// list as it was, when it comes after all k.
TRL_HD bool trl_gl_insert(TrlGlEntry* list, int k, int metric, float score, int32_t index) {
    int p = k - 1;
    if (!trl_gl_before(metric, score, index, list[p].score, list[p].index)) return false;
    for (; p > 0 && trl_gl_before(metric, score, index, list[p - 1].score, list[p - 1].index); p--) list[p] = list[p - 1];
    list[p].score = score;
    list[p].index = index;
    return true;
}

// out[0..k) (a list as above) takes the matches of `count` lists of k entries, `stride` entries apart.  Each of them is in order,
// so a list is left at its first entry that does not get in: nothing behind it would.
TRL_HD void trl_gl_merge(TrlGlEntry* out, int k, int metric, const TrlGlEntry* lists, long long count, long long stride) {
    for (long long l = 0; l < count; l++) {
        const TrlGlEntry* src = lists + l * stride;
        for (int e = 0; e < k; e++)
            if (!trl_gl_insert(out, k, metric, src[e].score, src[e].index)) break;
    }
}

// trl_pool.h -- the rules of embedding templates ("Templates"; section 7, f-13), for host and device alike: the
// kernels of trl_pool.hip and tests/pool_main.cpp run this code, tests/pool_ref.py is its reference.
//
// A template is the segmented, optionally weighted mean of unit embeddings, keyed by a group id per row, and its sum is DEFINED IN
// FIXED POINT: every term is one float32 value turned into an integer of 2^-32 units, and integers add associatively.  So the
// accumulators -- and everything computed from them -- are the same bits for any tiling, any split of the rows into calls, any
// order of the rows and any stream.  Every float operation below rounds once (the build has -ffp-contract=off).
//
// The state of groups g0 .. g0 + G - 1 is 8 (514 G + 1) bytes of int64: skipped, W[G], N[G], A[G][512].
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "trl_hd.h"

enum { TRL_POOL_K = 512, TRL_POOL_UNIT = 0, TRL_POOL_MEAN = 1 };
enum { TRL_POOL_IGNORED = 0, TRL_POOL_SKIPPED = 1, TRL_POOL_CONTRIBUTES = 2 };
#define TRL_POOL_MAX_ROWS (1LL << 30)          /* rows of one call, and contributing rows of one group over a state's life */
#define TRL_POOL_MAX_GROUPS 0x7fffffffLL

// the state's layout, in int64 words
TRL_HD long long trl_pool_words(long long groups) { return 514 * groups + 1; }
TRL_HD long long trl_pool_w_at(long long groups) { (void)groups; return 1; }
TRL_HD long long trl_pool_n_at(long long groups) { return 1 + groups; }
TRL_HD long long trl_pool_a_at(long long groups) { return 1 + 2 * groups; }

// x[0..512) with itself: the gallery's chain, trl_gallery_pack's bits
TRL_HD float trl_pool_chain(const float* a, const float* b) {
    float acc = 0.f;
    for (int k = 0; k < TRL_POOL_K; k++) acc = __builtin_fmaf(a[k], b[k], acc);
    return acc;
}

// What becomes of a row: IGNORED (its id lies outside g0 .. g0 + G - 1: counted nowhere), SKIPPED (counted in the state's
// `skipped`) or CONTRIBUTES.  w: the row's weight (1.0f without weights); n2: its chain.  NaN fails every comparison.
TRL_HD int trl_pool_class(int32_t gid, long long g0, long long groups, float w, float n2) {
    const long long g = (long long)gid - g0;
    if (g < 0 || g >= groups) return TRL_POOL_IGNORED;
    if (!(w > 0.f && w <= 1.f)) return TRL_POOL_SKIPPED;
    if (!(n2 >= FLT_MIN && n2 <= FLT_MAX)) return TRL_POOL_SKIPPED;
    return TRL_POOL_CONTRIBUTES;
}

// the factor of a contributing row, its terms and its weight in 2^-32 units.  |c x| <= 1 + 2^-15 (the chain's relative error on a
// normal n2 is at most gamma_512), so |term| < 2^32 (1 + 2^-15): 2^30 terms fit an int64
TRL_HD float trl_pool_factor(float w, float n2) { return w / __builtin_sqrtf(n2); }
TRL_HD long long trl_pool_term(float c, float x) {
    const float p = c * x;
    return (long long)__builtin_rintf(p * 0x1p32f);
}
TRL_HD long long trl_pool_weight(float w) { return (long long)__builtin_rintf(w * 0x1p32f); }

// finishing: an accumulator back to float32 (int64 -> float32 rounds to nearest), then the template's element
TRL_HD float trl_pool_value(long long a) { return (float)a * 0x1p-32f; }
TRL_HD float trl_pool_element(int mode, long long count, float t, float sq_n2t, float wf) {
    if (count == 0) return 0.f;
    return mode == TRL_POOL_UNIT ? t / sq_n2t : t / wf;
}
// the mean resultant length: 1 for identical rows, near 0 for unrelated ones
TRL_HD float trl_pool_cohesion(long long count, float sq_n2t, float wf) { return count == 0 ? 0.f : sq_n2t / wf; }

// one group, finished on the host (the device spreads the elements over a wave): tmpl[512], *weight, *cohesion
TRL_HD void trl_pool_finish_group(int mode, const long long* a, long long w, long long count, float* tmpl, float* weight, float* cohesion) {
    float t[TRL_POOL_K];
    for (int k = 0; k < TRL_POOL_K; k++) t[k] = trl_pool_value(a[k]);
    const float wf = trl_pool_value(w), sq = __builtin_sqrtf(trl_pool_chain(t, t));
    for (int k = 0; k < TRL_POOL_K; k++) tmpl[k] = trl_pool_element(mode, count, t[k], sq, wf);
    *weight = count == 0 ? 0.f : wf;
    *cohesion = trl_pool_cohesion(count, sq, wf);
}

// ---- the representative: the contributing row of a group with the largest gallery cosine against the group's template row ------
// cosine = chain(x, T) / (sqrtf(n2 T) * sqrtf(n2 x)): trl_gallery_scores' bits for query T and gallery row x
TRL_HD float trl_pool_cosine(float dot, float n2t, float n2x) { return dot / (__builtin_sqrtf(n2t) * __builtin_sqrtf(n2x)); }
// a candidate's key is trl_best_key(cosine, row) (trl_bestkey.h): the largest wins, ties to the lower row, a NaN cosine never

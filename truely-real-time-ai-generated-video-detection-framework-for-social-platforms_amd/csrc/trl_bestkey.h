// trl_bestkey.h -- the best row of a group as ONE 64-bit integer, for host and device alike: a template's representative
// (trl_pool.hip) and a group's best shot (trl_quality.hip) are the atomicMax of this key, and trl_best_key_read (trl_pool.hip) turns
// an array of them back into rows and scores.  tests/pool_main.cpp and tests/quality_main.cpp run it, tests/pool_ref.py is its
// reference.  (The tracker's clip score in k_track_scores packs a 32-bit integer score: another rule.)
#pragma once
#include <stdint.h>

#include "trl_hd.h"

// A candidate's 64-bit key; the largest key wins.  0: no candidate (a NaN score is never one).  From the top: the score's bits in
// an order that is the floats' (-0 counted as +0, so that the two tie), 0x7fffffff - index (ties go to the lower index), and one bit
// that says the score was -0, which decides nothing -- indices are distinct -- and lets the decode give back the score's own bits.
TRL_HD unsigned long long trl_best_key(float score, long long index) {
    if (score != score) return 0;
    union { float f; uint32_t u; } b;
    b.f = score;
    const uint32_t negzero = b.u == 0x80000000u;
    if (negzero) b.u = 0;
    const uint32_t ord = (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
    return ((unsigned long long)ord << 32) | ((unsigned long long)(uint32_t)(0x7fffffff - (int32_t)index) << 1) | negzero;
}
TRL_HD void trl_best_key_decode(unsigned long long key, int32_t* index, float* score) {
    if (key == 0) {
        *index = -1;
        *score = __builtin_nanf("");
        return;
    }
    const uint32_t ord = (uint32_t)(key >> 32), low = (uint32_t)key;
    union { float f; uint32_t u; } b;
    b.u = (ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord;
    if (low & 1) b.u = 0x80000000u;
    *index = 0x7fffffff - (int32_t)(low >> 1);
    *score = b.f;
}

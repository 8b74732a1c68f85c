// trl_jpeg_hufftab.h -- the optimal Huffman table of one symbol histogram, exactly as libjpeg's jpeg_gen_optimal_table builds it
// (what Pillow's Image.save(optimize=True) writes into each DHT).  One __host__ __device__ function: k_jpeg_tables runs it on one
// lane per (frame, table), trl_jpeg_optimal_table exports it for the tests, tests/jpeg_hufftab_main.cpp runs it under sanitizers.
//   * the pseudo-symbol 256 with count 1 reserves the all-ones code
//   * the two least frequent live entries are merged until one is left; c1 is the least frequent, c2 the next, and of equal counts
//     the LARGER symbol is taken (libjpeg scans upwards with <=).  Counts above 1,000,000,000 are never picked, as in libjpeg.
//   * code lengths above 16 are brought down to 16 by libjpeg's adjustment: a pair of the longest codes is moved up under a
//     prefix taken from the longest shorter length that has codes
//   * the pseudo-symbol's code (one of the longest) is removed; symbols are listed by length, then by value
// Only the live entries are scanned (kept in ascending symbol order, so the tie rule is unchanged), both minima are found in one
// scan, and the symbols are listed by a counting sort: the cost is quadratic in the number of symbols that occur, not in 257.
#pragma once
#include <stdint.h>

#include "trl_hd.h"

struct trl_hufftab_work {
    uint32_t freq[257];
    int16_t codesize[257];
    int16_t others[257];
    int16_t live[257];
    int16_t bits[33];
    int16_t at[33];
};

// hist: 256 counts.  bits[16]: codes per length 1..16.  vals: the symbols in code order (room for 256).  Returns their number.
// *maxlen (optional): the longest code length before the limiting step (tests use it to know that the step ran).  A histogram
// without any count gives an empty table.
TRL_HD int trl_jpeg_hufftab(const uint32_t* hist, uint8_t* bits, uint8_t* vals, trl_hufftab_work* w, int* maxlen) {
    int nl = 0;
    for (int i = 0; i < 257; ++i) {
        w->freq[i] = i < 256 ? hist[i] : 1u;
        w->codesize[i] = 0;
        w->others[i] = -1;
        if (w->freq[i]) w->live[nl++] = (int16_t)i;
    }
    for (;;) {
        // libjpeg's two scans in one: an entry that takes over as the least frequent leaves the previous one as the runner-up,
        // which is the last of the least among the others because <= always moves the later of two equals to the front
        int k1 = -1, k2 = -1;
        uint32_t v1 = 1000000000u, v2 = 1000000000u;
        for (int k = 0; k < nl; ++k) {
            const uint32_t f = w->freq[w->live[k]];
            if (f <= v1) { v2 = v1; k2 = k1; v1 = f; k1 = k; }
            else if (f <= v2) { v2 = f; k2 = k; }
        }
        if (k1 < 0 || k2 < 0) break;
        int c1 = w->live[k1], c2 = w->live[k2];
        w->freq[c1] += w->freq[c2];
        w->freq[c2] = 0;
        for (int k = k2; k + 1 < nl; ++k) w->live[k] = w->live[k + 1];
        --nl;
        ++w->codesize[c1];
        while (w->others[c1] >= 0) { c1 = w->others[c1]; ++w->codesize[c1]; }
        w->others[c1] = (int16_t)c2;
        ++w->codesize[c2];
        while (w->others[c2] >= 0) { c2 = w->others[c2]; ++w->codesize[c2]; }
    }
    for (int i = 0; i <= 32; ++i) w->bits[i] = w->at[i] = 0;
    int longest = 0;
    for (int i = 0; i < 257; ++i) {
        int cs = w->codesize[i];
        if (!cs) continue;
        if (cs > 32) w->codesize[i] = (int16_t)(cs = 32);     // libjpeg fails here; it takes >= 9,227,465 symbols (Fibonacci counts)
        ++w->bits[cs];
        if (i < 256) ++w->at[cs];                             // (the symbols alone: the pseudo-symbol is not listed)
        if (cs > longest) longest = cs;
    }
    if (maxlen) *maxlen = longest;
    for (int l = 0; l < 16; ++l) bits[l] = 0;
    if (!longest) return 0;
    int i;
    for (i = 32; i > 16; --i) {
        while (w->bits[i] > 0) {
            int j = i - 2;
            while (w->bits[j] == 0) --j;
            w->bits[i] -= 2;
            ++w->bits[i - 1];
            w->bits[j + 1] += 2;
            --w->bits[j];
        }
    }
    while (w->bits[i] == 0) --i;                              // the pseudo-symbol's code is one of the longest
    --w->bits[i];
    for (int l = 1; l <= 16; ++l) bits[l - 1] = (uint8_t)w->bits[l];
    int p = 0;                                                // by unadjusted length, then by value: one counting-sort pass
    for (int l = 1; l <= longest; ++l) { const int n = w->at[l]; w->at[l] = (int16_t)p; p += n; }
    for (int s = 0; s < 256; ++s)
        if (w->codesize[s]) vals[w->at[w->codesize[s]]++] = (uint8_t)s;
    return p;
}

// Drives csrc/trl_gallery_bins.h on the host: trl_gl_bin, the fixed-trip search, and trl_gl_bin_padded, the form of it that the
// histogram kernel runs (over edges padded with +inf, at the least trip count and at the kernel's ten), against a linear count of
// the edges, score by score.
// stdin, any number of cases:   metric E count   then E edge bit patterns (hex), then `count` score bit patterns (hex)
// stdout per score: its bin (E + 1 for NaN).  Exit status 3, and a line on stderr, at the first score whose two bins differ.
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_gallery_bins.h"

static float from_bits(unsigned bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

int main() {
    int metric, E, count;
    while (scanf("%d %d %d", &metric, &E, &count) == 3) {
        if (E < 1 || E > TRL_GL_MAX_EDGES || count < 0 || (metric != TRL_GL_COSINE && metric != TRL_GL_EUCLIDEAN)) return 2;
        std::vector<float> edges((size_t)E);              // exactly E floats: the sanitizer sees a read past either end
        for (int e = 0; e < E; e++) {
            unsigned bits;
            if (scanf("%x", &bits) != 1) return 2;
            edges[e] = from_bits(bits);
        }
        const int steps = trl_gl_bin_steps(E);
        std::vector<float> tight(((size_t)1 << steps) - 1, __builtin_inff()), wide((size_t)TRL_GL_PADDED_EDGES, __builtin_inff());
        for (int e = 0; e < E; e++) tight[e] = wide[e] = edges[e];
        if (trl_gl_bin_steps(E) > 10 || (1 << trl_gl_bin_steps(E)) < E + 1 || (E > 1 && (1 << (trl_gl_bin_steps(E) - 1)) >= E + 1)) return 4;
        for (int i = 0; i < count; i++) {
            unsigned bits;
            if (scanf("%x", &bits) != 1) return 2;
            const float s = from_bits(bits);
            int want = 0;
            for (int e = 0; e < E; e++) want += metric == TRL_GL_COSINE ? edges[e] <= s : edges[e] < s;
            if (s != s) want = E + 1;
            const int got = trl_gl_bin(metric, s, edges.data(), E);
            const int got_tight = trl_gl_bin_padded(metric, s, tight.data(), E, steps);
            const int got_wide = trl_gl_bin_padded(metric, s, wide.data(), E, TRL_GL_MAX_STEPS);
            if (got_tight != want || got_wide != want) {
                fprintf(stderr, "metric %d E %d score %08x: padded bins %d and %d, linear count %d\n", metric, E, bits, got_tight, got_wide, want);
                return 3;
            }
            if (got != want) {
                fprintf(stderr, "metric %d E %d score %08x: bin %d, linear count %d\n", metric, E, bits, got, want);
                return 3;
            }
            printf("%d\n", got);
        }
    }
    return 0;
}

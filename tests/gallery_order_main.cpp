// Drives csrc/trl_gallery_order.h on the host, the way the search and merge kernels use it: every strip's matches go into that
// strip's list with trl_gl_insert; then, as in k_gallery_merge, "lane" l inserts the entries of strips l, l + 64, ... into a list
// of its own and trl_gl_merge folds lists 1..63 into list 0.
// stdin, any number of cases:   metric k count strips   then `count` lines   score-bits(hex) index strip
// stdout per case: k lines      score-bits(hex) index                        (an empty slot: 7fc00000 -1)
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_gallery_order.h"

int main() {
    int metric, k, count, strips;
    while (scanf("%d %d %d %d", &metric, &k, &count, &strips) == 4) {
        if (k < 1 || k > TRL_GL_MAX_K || strips < 1 || count < 0) return 2;
        std::vector<TrlGlEntry> lists((size_t)strips * k, trl_gl_empty());
        for (int i = 0; i < count; i++) {
            unsigned bits;
            int index, strip;
            if (scanf("%x %d %d", &bits, &index, &strip) != 3 || strip < 0 || strip >= strips) return 2;
            float score;
            memcpy(&score, &bits, 4);
            trl_gl_insert(&lists[(size_t)strip * k], k, metric, score, index);
        }
        std::vector<TrlGlEntry> best((size_t)64 * k, trl_gl_empty());
        for (int s = 0; s < strips; s++)
            for (int e = 0; e < k; e++) trl_gl_insert(&best[(size_t)(s % 64) * k], k, metric, lists[(size_t)s * k + e].score, lists[(size_t)s * k + e].index);
        trl_gl_merge(best.data(), k, metric, best.data() + k, 63, k);
        for (int e = 0; e < k; e++) {
            unsigned bits;
            memcpy(&bits, &best[e].score, 4);
            if (best[e].index == TRL_GL_EMPTY) printf("7fc00000 -1\n");
            else printf("%08x %d\n", bits, best[e].index);
        }
    }
    return 0;
}

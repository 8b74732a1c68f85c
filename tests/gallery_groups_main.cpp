// Drives csrc/trl_gallery_groups.h on the host, the way the grouped search and merge kernels use it: every strip's matches go into
// that strip's list with trl_gl_insert_group (rows with a negative group are left out, as the kernel leaves them out); then, as in
// k_gallery_merge_groups, "lane" l inserts the entries of strips l, l + 64, ... into a list of its own and trl_gl_merge_groups folds
// lists 1..63 into list 0.
// stdin, any number of cases:   metric k count strips   then `count` lines   score-bits(hex) index strip group
// stdout per case: k lines      score-bits(hex) index group                  (an empty slot: 7fc00000 -1 -1)
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_gallery_groups.h"

int main() {
    int metric, k, count, strips;
    while (scanf("%d %d %d %d", &metric, &k, &count, &strips) == 4) {
        if (k < 1 || k > TRL_GL_MAX_K || strips < 1 || count < 0) return 2;
        std::vector<TrlGlEntry> lists((size_t)strips * k, trl_gl_empty());
        std::vector<int32_t> ids((size_t)strips * k, -1);
        for (int i = 0; i < count; i++) {
            unsigned bits;
            int index, strip, group;
            if (scanf("%x %d %d %d", &bits, &index, &strip, &group) != 4 || strip < 0 || strip >= strips) return 2;
            float score;
            memcpy(&score, &bits, 4);
            if (group >= 0) trl_gl_insert_group(&lists[(size_t)strip * k], &ids[(size_t)strip * k], k, metric, score, index, group);
        }
        std::vector<TrlGlEntry> best((size_t)64 * k, trl_gl_empty());
        std::vector<int32_t> best_ids((size_t)64 * k, -1);
        for (int s = 0; s < strips; s++)
            for (int e = 0; e < k; e++) {
                const TrlGlEntry& v = lists[(size_t)s * k + e];
                if (v.index != TRL_GL_EMPTY)
                    trl_gl_insert_group(&best[(size_t)(s % 64) * k], &best_ids[(size_t)(s % 64) * k], k, metric, v.score, v.index, ids[(size_t)s * k + e]);
            }
        trl_gl_merge_groups(best.data(), best_ids.data(), k, metric, best.data() + k, best_ids.data() + k, 63, k);
        for (int e = 0; e < k; e++) {
            unsigned bits;
            memcpy(&bits, &best[e].score, 4);
            if (best[e].index == TRL_GL_EMPTY) printf("7fc00000 -1 %d\n", best_ids[e]);
            else printf("%08x %d %d\n", bits, best[e].index, best_ids[e]);
        }
    }
    return 0;
}

// trl_gallery_groups.h -- the list operations of the grouped search, for host and device
// alike: k_gallery_search_groups' per-row lists, k_gallery_merge_groups and tests/gallery_groups_main.cpp run this code.
//
// Every gallery row carries a group id >= 0 (a row with a negative id is excluded by the caller and never reaches these functions).
// A list is k entries of trl_gallery_order.h in match order, empty slots last, plus a PARALLEL int32 array of their groups (-1 in
// an empty slot), and no two entries of a list share a group: it holds the best row of each of the k best groups seen so far.
// The groups lie beside the entries, not inside them, so that an entry stays one aligned 8-byte word -- the comparison with the
// k-th entry that rejects almost every score reads that word alone -- and the search for an entry of the same group, run for
// survivors only, walks k consecutive int32.
#pragma once
#include "trl_gallery_order.h"

// The slot of groups[0..k) that holds `group`, -1 when none does; k <= N.  All N reads are made before any is looked at (slots past
// k read slot k - 1 again) and there is no branch per slot: on the device the reads are in flight together, where a loop that stops
// at the first hit pays a full LDS round trip per slot -- and this search runs in every wave in which any lane has a survivor.
template <int N>
TRL_HD int trl_gl_find_group(const int32_t* groups, int k, int32_t group) {
    int32_t g[N];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e < N; e++) g[e] = groups[e < k ? e : k - 1];
    int f = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e < N; e++)
        if (e < k && g[e] == group) f = e;
    return f;
}

// Puts (score, index) of group `group` (>= 0) where it belongs; false, and the list as it was, when it does not get in:
//   * it comes after the k-th entry: with k better distinct groups in the list it cannot be among the k best groups' best rows,
//     and a list that is not full has an empty k-th slot, which every match comes before;
//   * the list holds an entry of the same group that comes before it.
// An entry of the same group that comes after it is removed: the entries between the newcomer's place and that entry move down by
// one, the entries behind it stay.  Without such an entry this is trl_gl_insert: the last entry is dropped.
TRL_HD bool trl_gl_insert_group(TrlGlEntry* list, int32_t* groups, int k, int metric, float score, int32_t index, int32_t group) {
    if (!trl_gl_before(metric, score, index, list[k - 1].score, list[k - 1].index)) return false;
    // the slot that is given up: the same group's (at most one), or else the last
    const int f = k <= 4 ? trl_gl_find_group<4>(groups, k, group) : k <= 8 ? trl_gl_find_group<8>(groups, k, group)
                                                                           : trl_gl_find_group<TRL_GL_MAX_K>(groups, k, group);
    const bool same = f >= 0;
    int p = same ? f : k - 1;
    if (same && !trl_gl_before(metric, score, index, list[p].score, list[p].index)) return false;
    for (; p > 0 && trl_gl_before(metric, score, index, list[p - 1].score, list[p - 1].index); p--) {
        list[p] = list[p - 1];
        groups[p] = groups[p - 1];
    }
    list[p].score = score;
    list[p].index = index;
    groups[p] = group;
    return true;
}

// out / out_groups (a list as above) take the entries of `count` such lists, `stride` entries apart in `lists` and in `groups`.
// A list is left at its first empty slot, and at its first entry that comes after out's k-th: nothing behind it comes before.
// An entry that fails because out holds a better row of its group does NOT end its list -- the entries behind it belong to other
// groups and may still get in (trl_gl_merge's early break would lose them).
TRL_HD void trl_gl_merge_groups(TrlGlEntry* out, int32_t* out_groups, int k, int metric, const TrlGlEntry* lists, const int32_t* groups,
                                   long long count, long long stride) {
    for (long long l = 0; l < count; l++) {
        const TrlGlEntry* src = lists + l * stride;
        const int32_t* grp = groups + l * stride;
        for (int e = 0; e < k; e++) {
            if (src[e].index == TRL_GL_EMPTY) break;
            if (!trl_gl_before(metric, src[e].score, src[e].index, out[k - 1].score, out[k - 1].index)) break;
            trl_gl_insert_group(out, out_groups, k, metric, src[e].score, src[e].index, grp[e]);
        }
    }
}

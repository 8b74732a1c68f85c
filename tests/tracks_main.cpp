// Drives csrc/trl_tracks.h on the host, composed the way k_track_update composes it: per frame ageing, the key matrix, the greedy
// matching (one "lane": W::first is the identity), the matched tracks, the new tracks, the touched rows.  A pair's similarity is
// not computed here: it is read from the case's table of all detection-pair similarities, by the global rows of the detection
// and of the track's last matched detection (TrlTkSlot::src).
// stdin, any number of cases:
//   has_emb iou_min-bits(hex) sim_min-bits(hex) max_age table_cap n m
//   n counts;  m lines of four box-bits(hex);  with has_emb, m lines of m sim-bits(hex): [det row][track row]
// stdout per case: m lines `track sim-bits flag`, one line `next_id dropped table_overflow`, then min(table_cap, next_id) table rows
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_tracks.h"

static float bits_float(unsigned b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

struct One {
    TrlTkCand first(TrlTkCand c) const { return c; }
};

int main() {
    int has_emb, max_age, cap, n, m;
    unsigned iou_bits, sim_bits;
    while (scanf("%d %x %x %d %d %d %d", &has_emb, &iou_bits, &sim_bits, &max_age, &cap, &n, &m) == 7) {
        if (n < 0 || m < 0 || cap < 0) return 2;
        const float iou_min = bits_float(iou_bits), sim_min = bits_float(sim_bits);
        std::vector<int> counts(n);
        std::vector<float> boxes((size_t)m * 4), sims(has_emb ? (size_t)m * m : 0);
        for (int& c : counts)
            if (scanf("%d", &c) != 1) return 2;
        for (float& v : boxes) {
            unsigned b;
            if (scanf("%x", &b) != 1) return 2;
            v = bits_float(b);
        }
        for (float& v : sims) {
            unsigned b;
            if (scanf("%x", &b) != 1) return 2;
            v = bits_float(b);
        }
        std::vector<int32_t> track(m, -1), table((size_t)cap * TRL_TK_ROW, 0);
        std::vector<float> sim(m, TRL_TK_NO_SIM);
        std::vector<unsigned char> flag(m, 0);
        TrlTkSlot slots[TRL_TK_SLOTS];
        TrlTkHead head;
        memset(slots, 0, sizeof slots);
        memset(&head, 0, sizeof head);
        std::vector<float> key(TRL_TK_SLOTS * TRL_TK_SLOTS);
        int32_t slot_id[TRL_TK_SLOTS], det_slot[TRL_TK_SLOTS];
        int off = 0;
        for (int t = 0; t < n; t++) {
            const long long f = head.frames_seen + t;
            int c = counts[t] < 0 ? 0 : counts[t];
            if (c > m - off) c = m - off;
            const int nd = c < TRL_TK_SLOTS ? c : TRL_TK_SLOTS;
            head.dropped += c - nd;
            unsigned long long live = 0;
            for (int s = 0; s < TRL_TK_SLOTS; s++) {
                trl_tk_age(slots[s], f, max_age, table.data(), cap);
                slot_id[s] = slots[s].used ? slots[s].id : -1;
                if (slots[s].used) live |= 1ull << s;
            }
            const float* dbox = boxes.data() + (size_t)off * 4;
            for (int s = 0; s < TRL_TK_SLOTS; s++)
                for (int d = 0; d < nd && slot_id[s] >= 0; d++) {
                    const float iou = trl_tk_iou(slots[s].box, dbox + 4 * d);
                    const float sv = has_emb && trl_tk_iou_ok(iou, iou_min) ? sims[(size_t)(off + d) * m + slots[s].src] : 0.f;
                    key[s * TRL_TK_SLOTS + d] = trl_tk_pair_key(iou, sv, has_emb != 0, iou_min, sim_min);
                }
            One w;
            trl_tk_greedy<1>(w, 0, key.data(), TRL_TK_SLOTS, slot_id, live, nd, det_slot);
            for (int d = 0; d < nd; d++) {
                const int s = det_slot[d];
                if (s < 0) continue;
                const float k = key[s * TRL_TK_SLOTS + d];
                flag[off + d] = (unsigned char)trl_tk_matched(slots[s], dbox + 4 * d, 0.f, off + d, f, k, has_emb != 0);
                if (has_emb) sim[off + d] = k;
                track[off + d] = slots[s].id;
            }
            trl_tk_create(slots, head, det_slot, nd, dbox, nullptr, off, f, table.data(), cap, track.data());
            for (int s = 0; s < TRL_TK_SLOTS; s++)
                if (slots[s].used && slots[s].last_frame == (int32_t)f) trl_tk_row(slots[s], s, table.data(), cap);
            off += c;
        }
        head.frames_seen += n;
        for (int i = 0; i < m; i++) {
            unsigned b;
            memcpy(&b, &sim[i], 4);
            printf("%d %08x %d\n", track[i], b, flag[i]);
        }
        printf("%d %d %d\n", head.next_id, head.dropped, head.table_overflow);
        for (int i = 0; i < cap && i < head.next_id; i++) {
            const int32_t* r = &table[(size_t)i * TRL_TK_ROW];
            printf("%d %d %d %d %d %d %d %d\n", r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
        }
    }
    return 0;
}

// shots_main.cpp -- csrc/trl_shots.h built for the host: the rules of shot boundaries (the regions, the counts, the distance, the cut
// scan) run exactly as the kernels of trl_shots.hip run them; and csrc/trl_tracks.h composed the way k_track_update composes it,
// with the cut rule in front of ageing.  tests/test_shots_cpu.py compiles this file -- once plain and once with the sanitizers --
// feeds it cases and holds the output to tests/shots_ref.py bit for bit.
//
// argv[1]: a file of raw u8 frames.  stdin, per case:
//   S n H W band_rows                                       the signatures of the file's first n frames, rows taken band_rows at a time
//   D H W drop   then 2 x 1536 counts                        the distance of two signatures
//   U n H W threshold-bits(hex) drop min_shot k w_1 .. w_k   the file's first n frames as a clip in k windows (sum w = n; 0 allowed)
//   T has_emb iou_min-bits sim_min-bits max_age n m          n lines `count cut`;  m lines of four box-bits;  with has_emb, m lines
//                                                            of m sim-bits [det row][track row]
// stdout: S: a line of 1536 counts per frame;  D: dist-bits;  U: a line `dist-bits cut shot` per frame, then `frames_seen last_cut cuts`
//         T: m lines `track sim-bits flag`, one line `next_id dropped`, then next_id table rows
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_shots.h"
#include "trl_tracks.h"

static float f32_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

struct One {
    TrlTkCand first(TrlTkCand c) const { return c; }
};

static int tracks_case() {
    int has_emb, max_age, n, m;
    unsigned iou_bits, sim_bits;
    if (scanf("%d %x %x %d %d %d", &has_emb, &iou_bits, &sim_bits, &max_age, &n, &m) != 6 || n < 0 || m < 0) return 2;
    const float iou_min = f32_of(iou_bits), sim_min = f32_of(sim_bits);
    const int cap = m;
    std::vector<int> counts(n), cuts(n);
    std::vector<float> boxes((size_t)m * 4), sims(has_emb ? (size_t)m * m : 0);
    for (int t = 0; t < n; t++)
        if (scanf("%d %d", &counts[t], &cuts[t]) != 2) return 2;
    for (float& v : boxes) {
        unsigned b;
        if (scanf("%x", &b) != 1) return 2;
        v = f32_of(b);
    }
    for (float& v : sims) {
        unsigned b;
        if (scanf("%x", &b) != 1) return 2;
        v = f32_of(b);
    }
    std::vector<int32_t> track(m, -1), table((size_t)cap * TRL_TK_ROW + 1, 0);
    std::vector<float> sim(m, TRL_TK_NO_SIM);
    std::vector<unsigned char> flag(m, 0);
    std::vector<TrlTkSlot> slots(TRL_TK_SLOTS);
    TrlTkHead head;
    memset(slots.data(), 0, sizeof(TrlTkSlot) * TRL_TK_SLOTS);
    memset(&head, 0, sizeof head);
    std::vector<float> key(TRL_TK_SLOTS * TRL_TK_SLOTS);
    int32_t slot_id[TRL_TK_SLOTS], det_slot[TRL_TK_SLOTS];
    int off = 0;
    for (int t = 0; t < n; t++) {
        const long long f = t;
        int c = counts[t] < 0 ? 0 : counts[t];
        if (c > m - off) c = m - off;
        const int nd = c < TRL_TK_SLOTS ? c : TRL_TK_SLOTS;
        head.dropped += c - nd;
        unsigned long long live = 0;
        for (int s = 0; s < TRL_TK_SLOTS; s++) {
            if (cuts[t]) trl_tk_cut(slots[s], table.data(), cap);
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
        trl_tk_create(slots.data(), head, det_slot, nd, dbox, nullptr, off, f, table.data(), cap, track.data());
        for (int s = 0; s < TRL_TK_SLOTS; s++)
            if (slots[s].used && slots[s].last_frame == (int32_t)f) trl_tk_row(slots[s], s, table.data(), cap);
        off += c;
    }
    for (int i = 0; i < m; i++) printf("%d %08x %d\n", track[i], bits_of(sim[i]), flag[i]);
    printf("%d %d\n", head.next_id, head.dropped);
    for (int i = 0; i < cap && i < head.next_id; i++) {
        const int32_t* r = &table[(size_t)i * TRL_TK_ROW];
        printf("%d %d %d %d %d %d %d %d\n", r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<uint8_t> frames;
    if (FILE* f = fopen(argv[1], "rb")) {
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, f)) > 0) frames.insert(frames.end(), buf, buf + k);
        fclose(f);
    } else
        return 2;
    char kind[4];
    while (scanf("%3s", kind) == 1) {
        if (kind[0] == 'T') {
            if (int rc = tracks_case()) return rc;
            continue;
        }
        if (kind[0] == 'D') {
            int H, W, drop;
            if (scanf("%d %d %d", &H, &W, &drop) != 3 || !trl_shots_dim_ok(H, W) || !trl_shots_drop_ok(drop)) return 2;
            std::vector<int32_t> ab(2 * TRL_SHOTS_SIG);
            for (int32_t& v : ab)
                if (scanf("%d", &v) != 1) return 2;
            printf("%08x\n", bits_of(trl_shots_distance(ab.data(), ab.data() + TRL_SHOTS_SIG, H, W, drop)));
            continue;
        }
        int n, H, W;
        if (scanf("%d %d %d", &n, &H, &W) != 3 || n < 0 || !trl_shots_dim_ok(H, W)) return 2;
        if ((size_t)n * H * W * 3 > frames.size()) return 2;
        std::vector<int32_t> sig((size_t)n * TRL_SHOTS_SIG, 0);
        int band_rows = H;
        if (kind[0] == 'S' && (scanf("%d", &band_rows) != 1 || band_rows < 1)) return 2;
        for (int i = 0; i < n; i++)
            for (int y0 = 0; y0 < H; y0 += band_rows)
                trl_shots_accumulate(frames.data() + (size_t)i * H * W * 3, H, W, y0, y0 + band_rows < H ? y0 + band_rows : H,
                                     sig.data() + (size_t)i * TRL_SHOTS_SIG);
        if (kind[0] == 'S') {
            for (int i = 0; i < n; i++) {
                for (int k = 0; k < TRL_SHOTS_SIG; k++) printf(k ? " %d" : "%d", sig[(size_t)i * TRL_SHOTS_SIG + k]);
                printf("\n");
            }
            continue;
        }
        if (kind[0] != 'U') return 2;
        unsigned thr;
        int windows;
        trl_shots_params prm;
        if (scanf("%x %d %d %d", &thr, &prm.drop, &prm.min_shot, &windows) != 4 || windows < 0) return 2;
        prm.threshold = f32_of(thr);
        if (!trl_shots_params_ok(prm)) return 3;
        std::vector<TrlShotsState> st(1);
        memset(st.data(), 0, sizeof(TrlShotsState));
        std::vector<float> dist(n + 1);
        std::vector<uint8_t> cut(n + 1);
        std::vector<int32_t> shot(n + 1);
        int at = 0;
        for (int k = 0; k < windows; k++) {
            int w;
            if (scanf("%d", &w) != 1 || w < 0 || at + w > n) return 2;
            trl_shots_window(st[0], sig.data() + (size_t)at * TRL_SHOTS_SIG, w, H, W, prm, dist.data() + at, cut.data() + at, shot.data() + at);
            at += w;
        }
        if (at != n) return 2;
        for (int t = 0; t < n; t++) printf("%08x %d %d\n", bits_of(dist[t]), cut[t], shot[t]);
        printf("%lld %lld %lld\n", st[0].frames_seen, st[0].last_cut, st[0].cuts);
    }
    return 0;
}

// quality_main.cpp -- csrc/trl_quality.h built for the host: the rules of face quality (the rectangle, luma, Laplacian, the raw
// integers, the percentiles, the float chains, the best shot's key) run exactly as the kernels of trl_quality.hip run them.
// tests/test_quality_cpu.py compiles this file -- once plain and once with the sanitizers -- feeds it cases and holds the output to
// tests/quality_ref.py bit for bit.
//
// argv[1]: a file of raw u8 BGR frames.  stdin, per case:
//   Q n H W m has_pts band_rows  6 x param-bits(hex)        the frames are the file's first n H W 3 bytes
//     m rows of:  frame_of  4 x box-bits(hex)  [10 x point-bits(hex)]
//   K count                                                  count rows of:  quality-bits(hex)  index
// stdout: per Q row   status  8 x raw (decimal)  12 x feat-bits  256 x hist
//         per K row   key(hex)  decoded index  decoded quality-bits
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_bestkey.h"
#include "trl_quality.h"

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
static bool read_floats(float* dst, int count) {
    for (int i = 0; i < count; i++) {
        uint32_t u;
        if (scanf("%x", &u) != 1) return false;
        dst[i] = f32_of(u);
    }
    return true;
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
        if (kind[0] == 'K') {
            long long count;
            if (scanf("%lld", &count) != 1) return 2;
            for (long long i = 0; i < count; i++) {
                float q;
                long long index;
                if (!read_floats(&q, 1) || scanf("%lld", &index) != 1) return 2;
                const unsigned long long key = trl_best_key(q, index);
                int32_t back;
                float score;
                trl_best_key_decode(key, &back, &score);
                printf("%016llx %d %08x\n", key, back, bits_of(score));
            }
            continue;
        }
        int n, H, W, has_pts, band_rows;
        long long m;
        float ref[6];
        if (scanf("%d %d %d %lld %d %d", &n, &H, &W, &m, &has_pts, &band_rows) != 6 || !read_floats(ref, 6)) return 2;
        if ((size_t)n * H * W * 3 > frames.size() || band_rows < 1) return 2;
        trl_quality_params prm;
        prm.sharp_ref = ref[0], prm.clip_ref = ref[1], prm.contrast_ref = ref[2], prm.yaw_ref = ref[3], prm.pitch_ref = ref[4];
        prm.size_ref = ref[5];
        if (!trl_quality_params_ok(prm)) return 3;
        for (long long r = 0; r < m; r++) {
            long long frame_of;
            float box[4], pts[10] = {0};
            if (scanf("%lld", &frame_of) != 1 || !read_floats(box, 4) || (has_pts && !read_floats(pts, 10))) return 2;
            int rect[4];
            const int status = trl_quality_rect((int)frame_of, n, H, W, box, rect);
            int32_t hist[TRL_QUALITY_BINS] = {0};
            long long sl = 0, sl2 = 0;
            if (status) {
                const uint8_t* frame = frames.data() + (size_t)frame_of * H * W * 3;
                const int h = rect[3] - rect[1];
                for (int y0 = 0; y0 < h; y0 += band_rows)
                    trl_quality_accumulate(frame, W, rect, y0, y0 + band_rows < h ? y0 + band_rows : h, hist, &sl, &sl2);
            }
            long long raw[TRL_QUALITY_RAW];
            int p[2];
            float feat[TRL_QUALITY_FEAT];
            trl_quality_raw(hist, sl, sl2, rect[2] - rect[0], raw, p);
            trl_quality_features(status, raw, p, rect[3] - rect[1], has_pts != 0, pts, prm, feat);
            printf("%d", status);
            for (int i = 0; i < TRL_QUALITY_RAW; i++) printf(" %lld", raw[i]);
            for (int i = 0; i < TRL_QUALITY_FEAT; i++) printf(" %08x", bits_of(feat[i]));
            for (int i = 0; i < TRL_QUALITY_BINS; i++) printf(" %d", hist[i]);
            printf("\n");
        }
    }
    return 0;
}

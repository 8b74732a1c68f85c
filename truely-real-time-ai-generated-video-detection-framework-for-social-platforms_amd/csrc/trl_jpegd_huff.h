// The per-segment entropy decoder of the baseline-JPEG decoder, one function for the kernel (k_jpegd_huff) and for a CPU build
// (tests/jpegd_fuzz.cpp), and the decode tables it reads.  A segment is one restart interval of one frame (a stream without DRI
// is one segment).  Every read is bounded by the segment's limit, every write by the frame's block count and by 64 coefficients
// per block.  Anything irregular -- an invalid code, a run past coefficient 63, bytes running out, a marker other than the
// expected one, bytes left over -- ends the segment with JD_ST_IRREGULAR: libjpeg's error recovery is never imitated.
#ifndef TRL_JPEGD_HUFF_H
#define TRL_JPEGD_HUFF_H
#include "trl_jpegd_parse.h"

#if defined(__HIPCC__)
#define JD_HD __host__ __device__
#else
#define JD_HD
#endif

enum { JD_ST_OK = 0, JD_ST_UNSUPPORTED = 1, JD_ST_IRREGULAR = 2 };

constexpr int kJdLookBits = 9;

struct JdHuff {
    uint16_t look[1 << kJdLookBits];   // the next 9 bits -> (length << 8) | symbol for codes of up to 9 bits, 0 = longer or invalid
    int32_t maxcode[18];               // largest code of each length, -1 = none
    int32_t valoff[17];                // vals index of a code of length l = valoff[l] + code
    uint8_t vals[256];
    uint8_t pad[4];
};                                     // 1424 bytes
struct JdTables {
    JdHuff h[6];                       // DC, AC of component 0, 1, 2
    uint16_t quant[3][64];             // natural order
};
static_assert(sizeof(JdHuff) == 1424 && sizeof(JdTables) % 16 == 0, "table layout");

// Where a frame's blocks lie in its coefficient slot: component c's block (by, bx) is block base[c] + by * bw[c] + bx.
struct JdGeom {
    int mcux, mcuy, hs, vs;
    int base[3], bw[3];
    int nblocks;
};

JD_HD inline JdGeom jd_geom(int H, int W, int hs, int vs) {
    JdGeom g;
    g.hs = hs; g.vs = vs;
    g.mcux = (W + 8 * hs - 1) / (8 * hs);
    g.mcuy = (H + 8 * vs - 1) / (8 * vs);
    g.bw[0] = g.mcux * hs; g.bw[1] = g.bw[2] = g.mcux;
    g.base[0] = 0;
    g.base[1] = g.mcux * hs * g.mcuy * vs;
    g.base[2] = g.base[1] + g.mcux * g.mcuy;
    g.nblocks = g.base[2] + g.mcux * g.mcuy;
    return g;
}

static inline void jd_build_huff(const JdHuffSpec& s, JdHuff* t) {
    memset(t, 0, sizeof(*t));
    memcpy(t->vals, s.vals, 256);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t->valoff[len] = k - code;
        for (int i = 0; i < s.counts[len - 1]; ++i, ++k, ++code) {
            if (len <= kJdLookBits) {
                const int lo = code << (kJdLookBits - len);
                for (int j = 0; j < (1 << (kJdLookBits - len)); ++j)
                    if (lo + j < (1 << kJdLookBits)) t->look[lo + j] = (uint16_t)((len << 8) | s.vals[k]);
            }
        }
        t->maxcode[len] = s.counts[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[0] = -1;
    t->maxcode[17] = -1;
}

static inline void jd_build_tables(const JdParsed& p, JdTables* t) {
    for (int c = 0; c < 3; ++c) {
        jd_build_huff(p.dc[c], &t->h[2 * c]);
        jd_build_huff(p.ac[c], &t->h[2 * c + 1]);
        memcpy(t->quant[c], p.quant[c], sizeof(t->quant[c]));
    }
}

// nmcu MCUs, the frame's mcu0-th onwards, from the bytes [p, lim); the marker 0xFF `expect` must follow the last one inside
// [p, lim).  zz is the zigzag table (kJdZigzag, or the kernel's copy of it).  Non-zero coefficients go to coef (the frame's
// slot, zeroed by the caller) as int16 in natural order.
JD_HD inline int jpegd_decode_segment(const uint8_t* p, const uint8_t* lim, int expect, const JdHuff* h, const uint8_t* zz,
                                      const JdGeom& g, int mcu0, int nmcu, int16_t* coef) {
    uint64_t acc = 0;     // the next nb bits, left-aligned; zero below them
    int nb = 0;
    bool stop = false;    // the segment's end or a marker has been reached: no more bits
    unsigned pred[3] = {0, 0, 0};
#define JD_FILL()                                                                                                   \
    while (nb <= 56 && !stop) {                                                                                     \
        if (p >= lim) { stop = true; break; }                                                                       \
        const unsigned b_ = *p;                                                                                     \
        if (b_ != 0xFF) { acc |= (uint64_t)b_ << (56 - nb); nb += 8; ++p; }                                         \
        else if (p + 1 < lim && p[1] == 0) { acc |= (uint64_t)0xFF << (56 - nb); nb += 8; p += 2; }                 \
        else stop = true;                                                                                           \
    }
// one Huffman symbol of table T into sym
#define JD_SYMBOL(T)                                                                                                \
    {                                                                                                               \
        if (nb < 32) JD_FILL();                                                                                     \
        const unsigned e_ = (T).look[acc >> (64 - kJdLookBits)];                                                    \
        int len_;                                                                                                   \
        if (e_) { len_ = (int)(e_ >> 8); sym = (int)(e_ & 255); }                                                   \
        else {                                                                                                      \
            sym = -1;                                                                                               \
            for (len_ = kJdLookBits + 1; len_ <= 16; ++len_) {                                                      \
                const int c_ = (int)(acc >> (64 - len_));                                                           \
                if (c_ <= (T).maxcode[len_]) {                                                                      \
                    const unsigned i_ = (unsigned)((T).valoff[len_] + c_);                                          \
                    if (i_ < 256) sym = (T).vals[i_];                                                               \
                    break;                                                                                          \
                }                                                                                                   \
            }                                                                                                       \
            if (sym < 0) return JD_ST_IRREGULAR;                                                                    \
        }                                                                                                           \
        if (len_ > nb) return JD_ST_IRREGULAR;                                                                      \
        acc <<= len_; nb -= len_;                                                                                   \
    }
// s (1..15) bits, sign-extended as HUFF_EXTEND does, into val
#define JD_RECEIVE(s)                                                                                               \
    {                                                                                                               \
        if ((s) > nb) return JD_ST_IRREGULAR;                                                                       \
        val = (int)(acc >> (64 - (s)));                                                                             \
        acc <<= (s); nb -= (s);                                                                                     \
        if (val < (1 << ((s) - 1))) val += 1 - (1 << (s));                                                          \
    }
    for (int m = mcu0; m < mcu0 + nmcu; ++m) {
        const int my = m / g.mcux, mx = m - my * g.mcux;
        for (int c = 0; c < 3; ++c) {
            const int ch = c ? 1 : g.hs, cv = c ? 1 : g.vs;
            const JdHuff& D = h[2 * c];
            const JdHuff& A = h[2 * c + 1];
            for (int v = 0; v < cv; ++v)
                for (int hh = 0; hh < ch; ++hh) {
                    const long long blk = (long long)g.base[c] + (long long)(my * cv + v) * g.bw[c] + mx * ch + hh;
                    if (blk < 0 || blk >= g.nblocks) return JD_ST_IRREGULAR;
                    int16_t* B = coef + (size_t)blk * 64;
                    int sym, val;
                    JD_SYMBOL(D);
                    if (sym > 15) return JD_ST_IRREGULAR;
                    if (sym) { JD_RECEIVE(sym); pred[c] += (unsigned)val; }
                    if (pred[c]) B[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        JD_SYMBOL(A);
                        const int r = sym >> 4, s = sym & 15;
                        if (s) {
                            k += r;
                            if (k > 63) return JD_ST_IRREGULAR;
                            JD_RECEIVE(s);
                            B[zz[k]] = (int16_t)val;
                            ++k;
                        } else if (r == 15) {
                            k += 16;
                            if (k > 63) return JD_ST_IRREGULAR;
                        } else break;
                    }
                }
        }
    }
#undef JD_FILL
#undef JD_SYMBOL
#undef JD_RECEIVE
    if (nb >= 8) return JD_ST_IRREGULAR;                                      // whole bytes left over
    if (!(p + 1 < lim && p[0] == 0xFF && p[1] == expect)) return JD_ST_IRREGULAR;
    return JD_ST_OK;
}

// Host: where the restart markers of a DRI stream lie.  Walks [scan, n) at memchr speed, skipping stuffed 0xFF00 and fill 0xFF,
// and stores the offsets of up to cap RSTn markers; stops at the first other marker.  Returns how many it found (it keeps
// counting past cap).
static inline size_t jd_find_restarts(const uint8_t* d, size_t scan, size_t n, long long* pos, size_t cap) {
    size_t found = 0, p = scan;
    while (p < n) {
        const uint8_t* q = (const uint8_t*)memchr(d + p, 0xFF, n - p);
        if (!q) break;
        p = (size_t)(q - d);
        if (p + 1 >= n) break;
        const unsigned m = d[p + 1];
        if (m == 0) p += 2;
        else if (m == 0xFF) p += 1;
        else if (m >= 0xD0 && m <= 0xD7) { if (found < cap) pos[found] = (long long)p; ++found; p += 2; }
        else break;
    }
    return found;
}

// One restart interval of one frame, as k_jpegd_huff takes it.
struct JdSeg {
    long long off;        // of the segment's first byte in the files buffer
    int32_t len;          // bytes the segment may read: up to and including the marker that ends it
    int32_t frame, mcu0, nmcu, expect, pad;
};

// Host: the segments of one parsed file (at file_off of the files buffer, frame index `frame`) into out[0 .. cap); rst is
// scratch for mcux * mcuy offsets.  Returns their number, or -1 if they do not fit.  A stream with fewer markers than its
// interval asks for ends in a segment that cannot find its marker, which the decoder reports as irregular.
static inline long long jd_build_segments(const uint8_t* file, size_t len, const JdParsed& ps, const JdGeom& g, long long file_off,
                                          int frame, long long* rst, JdSeg* out, size_t cap) {
    const long long total = (long long)g.mcux * g.mcuy;
    const long long ri = ps.ri ? ps.ri : total;
    const long long want = (total + ri - 1) / ri;
    if ((size_t)want > cap) return -1;
    size_t marks = 0;
    if (want > 1) {
        marks = jd_find_restarts(file, (size_t)ps.scan, len, rst, (size_t)want - 1);
        if (marks > (size_t)want - 1) marks = (size_t)want - 1;
    }
    long long start = ps.scan;
    for (size_t j = 0; j <= marks; ++j) {
        const long long end = j == marks ? (long long)len : rst[j] + 2;
        JdSeg& sg = out[j];
        sg.off = file_off + start;
        sg.len = (int32_t)(end - start);
        sg.frame = frame;
        sg.mcu0 = (int32_t)((long long)j * ri);
        sg.nmcu = (int32_t)(ri < total - (long long)j * ri ? ri : total - (long long)j * ri);
        sg.expect = (long long)j == want - 1 ? 0xD9 : 0xD0 + (int)(j & 7);
        sg.pad = 0;
        start = end;
    }
    return (long long)marks + 1;
}

#endif

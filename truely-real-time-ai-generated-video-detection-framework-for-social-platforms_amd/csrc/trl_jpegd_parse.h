// Host-only marker parser of the baseline-JPEG decoder (trl_jpegd.hip): SOI .. SOS of one file -> sizes, sampling, restart
// interval, scan offset, the quantisation tables in natural order and the Huffman specifications of the three components, or
// the reason why the device decoder does not attempt the file.  Plain C++, no HIP: a stand-alone program can include it
// (tests/jpegd_fuzz.cpp).  Every read is bounded by the file's length.  tests/jpegd_ref.py's parse() states the same rules.
#ifndef TRL_JPEGD_PARSE_H
#define TRL_JPEGD_PARSE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "trl_zigzag.h"

// why a file is not attempted (trl_jpegd_info.reason, include/truely_hip.h)
enum {
    JD_OK = 0,
    JD_TRUNCATED = 1,     // the file ends inside its headers
    JD_NOT_JPEG = 2,      // no SOI
    JD_PROCESS = 3,       // a frame type other than SOF0: progressive, extended, lossless, arithmetic
    JD_PRECISION = 4,     // samples of other than 8 bits
    JD_COMPONENTS = 5,    // not three components (grayscale, CMYK), or component ids 'R','G','B'
    JD_SAMPLING = 6,      // other than luma 2x2 / 2x1 / 1x1 over chroma 1x1
    JD_DQT = 7,           // a 16-bit, malformed or missing quantisation table
    JD_DHT = 8,           // a malformed, over-long or missing Huffman table
    JD_SCAN = 9,          // not one interleaved scan of all three components with Ss=0, Se=63, Ah=Al=0
    JD_ADOBE = 10,        // an APP14 marker (libjpeg may then read the components as something other than YCbCr)
    JD_MARKER = 11,       // a marker that does not belong between SOI and SOS, or a malformed segment
    JD_SIZE = 12          // zero height or width (DNL).  (A size other than the decoder's is trl_jpegd_decode's to find: status 1)
};

static const uint8_t kJdZigzag[64] = TRL_ZIGZAG_LIST;

struct JdHuffSpec {
    uint8_t counts[16];   // codes of length 1..16
    uint8_t vals[256];
    uint8_t defined;
};

struct JdParsed {
    int reason;           // JD_OK: everything below is set
    int H, W, hs, vs;     // luma sampling factors (chroma is 1x1)
    int ri;               // restart interval in MCUs, 0 = none
    long long scan;       // offset of the first entropy-coded byte
    uint16_t quant[3][64];// per component, natural order
    JdHuffSpec dc[3], ac[3];
};

// jpeg_make_d_derived_tbl's checks: codes must fit their lengths, DC symbols are at most 15
static inline bool jd_huff_spec_ok(const JdHuffSpec& s, bool is_dc) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.counts[len - 1]; ++i, ++k, ++code) {
            if (code >= (1u << len)) return false;
            if (is_dc && s.vals[k] > 15) return false;
        }
        code <<= 1;
    }
    return true;
}

static inline int jpegd_parse(const uint8_t* d, size_t n, JdParsed* out) {
    memset(out, 0, sizeof(*out));
#define JD_FAIL(r) return (out->reason = (r))
    if (!d || n < 4) JD_FAIL(JD_TRUNCATED);
    if (d[0] != 0xFF || d[1] != 0xD8) JD_FAIL(JD_NOT_JPEG);
    uint16_t qt[4][64];
    bool qdef[4] = {false, false, false, false};
    static thread_local JdHuffSpec dht[2][4];
    memset(dht, 0, sizeof(dht));
    bool have_sof = false;
    int cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    size_t p = 2;
    for (;;) {
        if (p + 2 > n) JD_FAIL(JD_TRUNCATED);
        if (d[p] != 0xFF) JD_FAIL(JD_MARKER);
        while (p < n && d[p] == 0xFF) ++p;
        if (p >= n) JD_FAIL(JD_TRUNCATED);
        const int m = d[p++];
        if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) JD_FAIL(JD_PROCESS);
        const bool known = m == 0xC0 || m == 0xC4 || m == 0xDB || m == 0xDD || m == 0xDA || m == 0xFE || (m >= 0xE0 && m <= 0xEF);
        if (!known) JD_FAIL(JD_MARKER);
        if (p + 2 > n) JD_FAIL(JD_TRUNCATED);
        const size_t L = ((size_t)d[p] << 8) | d[p + 1];
        if (L < 2) JD_FAIL(JD_MARKER);
        if (p + L > n) JD_FAIL(JD_TRUNCATED);
        const uint8_t* b = d + p + 2;
        const size_t bl = L - 2;
        p += L;
        if (m == 0xEE) JD_FAIL(JD_ADOBE);
        if (m == 0xDB) {
            for (size_t q = 0; q < bl; q += 65) {
                if ((b[q] >> 4) != 0 || (b[q] & 15) > 3 || q + 65 > bl) JD_FAIL(JD_DQT);
                const int id = b[q] & 15;
                for (int i = 0; i < 64; ++i) qt[id][kJdZigzag[i]] = b[q + 1 + i];
                qdef[id] = true;
            }
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < bl) {
                if (q + 17 > bl || (b[q] >> 4) > 1 || (b[q] & 15) > 3) JD_FAIL(JD_DHT);
                JdHuffSpec s;
                memset(&s, 0, sizeof(s));
                size_t total = 0;
                for (int i = 0; i < 16; ++i) { s.counts[i] = b[q + 1 + i]; total += s.counts[i]; }
                if (total > 256 || q + 17 + total > bl) JD_FAIL(JD_DHT);
                memcpy(s.vals, b + q + 17, total);
                s.defined = 1;
                if (!jd_huff_spec_ok(s, (b[q] >> 4) == 0)) JD_FAIL(JD_DHT);
                dht[b[q] >> 4][b[q] & 15] = s;
                q += 17 + total;
            }
        } else if (m == 0xDD) {
            if (bl != 2) JD_FAIL(JD_MARKER);
            out->ri = (b[0] << 8) | b[1];
        } else if (m == 0xC0) {
            if (have_sof || bl < 6) JD_FAIL(JD_MARKER);
            if (b[0] != 8) JD_FAIL(JD_PRECISION);
            out->H = (b[1] << 8) | b[2];
            out->W = (b[3] << 8) | b[4];
            if (b[5] != 3 || bl != 6 + 9) JD_FAIL(JD_COMPONENTS);
            if (out->H < 1 || out->W < 1) JD_FAIL(JD_SIZE);
            int h[3], v[3];
            for (int i = 0; i < 3; ++i) { cid[i] = b[6 + 3 * i]; h[i] = b[7 + 3 * i] >> 4; v[i] = b[7 + 3 * i] & 15; ctq[i] = b[8 + 3 * i]; }
            if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') JD_FAIL(JD_COMPONENTS);
            const bool luma_ok = (h[0] == 2 && v[0] == 2) || (h[0] == 2 && v[0] == 1) || (h[0] == 1 && v[0] == 1);
            if (!luma_ok || h[1] != 1 || v[1] != 1 || h[2] != 1 || v[2] != 1) JD_FAIL(JD_SAMPLING);
            if (ctq[0] > 3 || ctq[1] > 3 || ctq[2] > 3) JD_FAIL(JD_DQT);
            out->hs = h[0]; out->vs = v[0];
            have_sof = true;
        } else if (m == 0xDA) {
            if (!have_sof) JD_FAIL(JD_SCAN);
            if (bl != 10 || b[0] != 3) JD_FAIL(JD_SCAN);
            for (int i = 0; i < 3; ++i) {
                if (b[1 + 2 * i] != cid[i]) JD_FAIL(JD_SCAN);
                const int td = b[2 + 2 * i] >> 4, ta = b[2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !dht[0][td].defined || !dht[1][ta].defined) JD_FAIL(JD_DHT);
                if (!qdef[ctq[i]]) JD_FAIL(JD_DQT);
                out->dc[i] = dht[0][td];
                out->ac[i] = dht[1][ta];
                memcpy(out->quant[i], qt[ctq[i]], sizeof(qt[0]));
            }
            if (b[7] != 0 || b[8] != 63 || b[9] != 0) JD_FAIL(JD_SCAN);
            out->scan = (long long)p;
            return out->reason = JD_OK;
        }
    }
#undef JD_FAIL
}

#endif

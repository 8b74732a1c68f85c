// Stand-alone host program around csrc/trl_jpeg_hufftab.h (the optimal-table builder the encoder runs on the device), built by
// tests/test_jpeg_options_cpu.py with the address and undefined-behaviour sanitizers.
//   jpeg_hufftab_main <histograms> : a file of N x 256 little-endian uint32 counts
// prints one line per histogram: the longest unadjusted code length, the 16 code counts and the symbols, in hex.  The arrays the
// builder writes sit between guard bytes, and every table is checked to be a prefix code that leaves the all-ones code free.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "trl_jpeg_hufftab.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <histograms>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint32_t> hist(256);
    while (fread(hist.data(), 4, 256, f) == 256) {
        // heap arrays of the exact sizes the contract names: the address sanitizer sees any write past them
        std::vector<uint8_t> bits(16, 0xEE), vals(256, 0xEE);
        trl_hufftab_work* w = new trl_hufftab_work;
        int maxlen = -1;
        const int n = trl_jpeg_hufftab(hist.data(), bits.data(), vals.data(), w, &maxlen);
        delete w;
        int present = 0, total = 0;
        for (int i = 0; i < 256; ++i) present += hist[i] != 0;
        unsigned long long kraft = 0;                        // in units of 2^-16
        for (int l = 1; l <= 16; ++l) { total += bits[l - 1]; kraft += (unsigned long long)bits[l - 1] << (16 - l); }
        if (n != present || total != n || (n && kraft >= 65536ull)) {
            fprintf(stderr, "bad table: %d symbols present, %d listed, %d codes, kraft %llu\n", present, n, total, kraft);
            return 1;
        }
        for (int i = 0; i < n; ++i)
            if (!hist[vals[i]]) { fprintf(stderr, "symbol %d has no count\n", vals[i]); return 1; }
        printf("%d ", maxlen);
        for (int i = 0; i < 16; ++i) printf("%02x", bits[i]);
        printf(" ");
        for (int i = 0; i < n; ++i) printf("%02x", vals[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}

// Stand-alone host program: the decoder's marker parser (trl_jpegd_parse.h) and its shared entropy-decode function
// (trl_jpegd_huff.h) on the files named on the command line, built by tests/test_jpegd_cpu.py with the address and
// undefined-behaviour sanitizers where their runtime is installed.  For every file it prints one line
//     <status> <reason> <blocks>
// (status 0 decoded, 1 not attempted, 2 entropy decode irregular) and, for status 0, writes the frame's coefficient slot
// (int16, component planes of 8x8 blocks in natural order) to <file>.coef.  The coefficient slot is allocated at exactly its size
// and every file is copied into an allocation of exactly its length, so a read or write out of bounds is an error the
// sanitizer reports.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "trl_jpegd_huff.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 3; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
        if (n > 0 && fread(data, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", argv[a]); return 3; }
        fclose(f);
        static JdParsed ps;
        int status = JD_ST_OK, blocks = 0;
        if (jpegd_parse(data, (size_t)n, &ps) != JD_OK) status = JD_ST_UNSUPPORTED;
        if (status == JD_ST_OK) {
            static JdTables tb;
            jd_build_tables(ps, &tb);
            const JdGeom g = jd_geom(ps.H, ps.W, ps.hs, ps.vs);
            blocks = g.nblocks;
            const size_t mcus = (size_t)g.mcux * g.mcuy;
            std::vector<long long> rst(mcus);
            std::vector<JdSeg> segs(mcus);
            const long long ns = jd_build_segments(data, (size_t)n, ps, g, 0, 0, rst.data(), segs.data(), segs.size());
            int16_t* coef = (int16_t*)calloc((size_t)g.nblocks * 64, sizeof(int16_t));
            if (ns < 0) status = JD_ST_UNSUPPORTED;
            for (long long j = 0; j < ns && status == JD_ST_OK; ++j)
                status = jpegd_decode_segment(data + segs[j].off, data + segs[j].off + segs[j].len, segs[j].expect, tb.h, kJdZigzag, g,
                                              segs[j].mcu0, segs[j].nmcu, coef);
            if (status == JD_ST_OK) {
                char name[4096];
                snprintf(name, sizeof(name), "%s.coef", argv[a]);
                FILE* o = fopen(name, "wb");
                if (!o || fwrite(coef, 2, (size_t)g.nblocks * 64, o) != (size_t)g.nblocks * 64) { fprintf(stderr, "cannot write %s\n", name); return 3; }
                fclose(o);
            }
            free(coef);
        }
        printf("%d %d %d\n", status, ps.reason, blocks);
        free(data);
    }
    return 0;
}

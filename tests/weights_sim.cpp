// weights_sim.cpp -- csrc/trl_weights.h and csrc/trl_facenet.h alone: the host half of trl_load_weights (tests/test_weights_cpu.py).
//
//   weights_sim <blob file> <embed_precision> <image file | ->
//     prints FaceNet's table, then stages the blob and prints what the staging made of it; writes the host image unless "-":
//       row <r> <name> <kind> <kh> <kw> <sh> <sw> <ph> <pw> <cin> <cout> <f32_only> <nparts> <part> ...
//       status <0 | -3>
//       error <text of trl_set_error>
//       item <i> <name> m <K> <Cout> <Kpad> <ld> <offset>      (a matrix)      |  only with status 0
//       item <i> <name> v <n> <offset>                          (a vector)      |
//       fn <r> <item of the matrix> <item of scale or bias> <item of shift, or -1>
//       logits <item of w> <item of b>                          (-1 -1: the blob has none)
//       total <bytes of the image>
//   weights_sim <blob file> <embed_precision> --drop
//     for every name on stdin: blanks the name of the blob's directory entry in memory, stages, restores it:
//       drop <name> <status> <error text>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "trl_weights.h"

static char g_err[512] = "";
void trl_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<char> blob;
    char buf[1 << 16];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    const int precision = atoi(argv[2]);
    StagedWeights st;

    if (!strcmp(argv[3], "--drop")) {
        uint32_t nt = 0;
        if (blob.size() >= 16) memcpy(&nt, blob.data() + 8, 4);
        if (16 + (size_t)nt * sizeof(TrlwEntry) > blob.size()) return 2;
        std::string name;
        while (std::getline(std::cin, name)) {
            int hit = 0;
            for (uint32_t i = 0; i < nt; i++) {
                char* e = blob.data() + 16 + (size_t)i * sizeof(TrlwEntry);   // (name is the entry's first field)
                if (strncmp(e, name.c_str(), 56) != 0) continue;
                hit++;
                char saved[56];
                memcpy(saved, e, 56);
                memset(e, 0, 56);
                g_err[0] = 0;
                const int s = trl_stage_weights(blob.data(), blob.size(), precision, &st);
                memcpy(e, saved, 56);
                printf("drop %s %d %s\n", name.c_str(), s, g_err);
            }
            if (!hit) return 3;
        }
        return 0;
    }

    const FnRow* rows = trl_facenet_rows();
    for (int r = 0; r < FN_ROWS; r++) {
        const FnRow& g = rows[r];
        printf("row %d %s %d %d %d %d %d %d %d %d %d %d %d", r, g.name, g.kind, g.kh, g.kw, g.sh, g.sw, g.ph, g.pw, g.cin, g.cout, (int)g.f32_only, g.nparts);
        for (int p = 0; p < g.nparts; p++) printf(" %s", g.part[p]);
        printf("\n");
    }
    const int s = trl_stage_weights(blob.data(), blob.size(), precision, &st);
    printf("status %d\nerror %s\n", s, g_err);
    if (s != 0) return 0;
    for (size_t i = 0; i < st.items.size(); i++) {
        const StagedTensor& t = st.items[i];
        if (t.mat) printf("item %zu %s m %d %d %d %d %zu\n", i, t.name.c_str(), t.K, t.Cout, t.Kpad, t.ld, t.off);
        else printf("item %zu %s v %d %zu\n", i, t.name.c_str(), t.n, t.off);
    }
    for (int r = 0; r < FN_ROWS; r++) printf("fn %d %d %d %d\n", r, st.fn[r].w, st.fn[r].v[0], st.fn[r].v[1]);
    printf("logits %d %d\ntotal %zu\n", st.logits_w, st.logits_b, st.image.size());
    if (strcmp(argv[3], "-") != 0) {
        FILE* o = fopen(argv[3], "wb");
        if (!o || fwrite(st.image.data(), 1, st.image.size(), o) != st.image.size() || fclose(o) != 0) return 4;
    }
    return 0;
}

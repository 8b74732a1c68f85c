// pool_main.cpp -- csrc/trl_pool.h built for the host: the rules of embedding templates (what a row becomes, a term, a weight, the
// finish, the representative's key) run exactly as the kernels of trl_pool.hip run them.  tests/test_pool_cpu.py compiles this file
// (with the sanitizers where the compiler has them), feeds it cases and holds the output to tests/pool_ref.py bit for bit.
//
// stdin, per case:   G g0 m
//                    m rows of:  gid  weight-bits(hex)  512 x element-bits(hex)
// stdout, per case:  skipped
//                    per group:  N  W  512 x A                                     (decimal int64)
//                    per mode (unit, mean), per group:  count  weight-bits  cohesion-bits  512 x template-bits
//                    per group:  key(hex)  index  score-bits                       (representative against the unit template)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "trl_bestkey.h"
#include "trl_pool.h"

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

int main() {
    long long G, g0, m;
    while (scanf("%lld %lld %lld", &G, &g0, &m) == 3) {
        std::vector<long long> state((size_t)trl_pool_words(G), 0);
        long long* W = state.data() + trl_pool_w_at(G);
        long long* N = state.data() + trl_pool_n_at(G);
        long long* A = state.data() + trl_pool_a_at(G);
        std::vector<float> x((size_t)m * TRL_POOL_K), w((size_t)m), n2((size_t)m);
        std::vector<int32_t> gid((size_t)m);
        std::vector<int> cls((size_t)m);
        for (long long i = 0; i < m; i++) {
            long long id;
            uint32_t u;
            if (scanf("%lld %x", &id, &u) != 2) return 2;
            gid[i] = (int32_t)id;
            w[i] = f32_of(u);
            for (int k = 0; k < TRL_POOL_K; k++) {
                if (scanf("%x", &u) != 1) return 2;
                x[(size_t)i * TRL_POOL_K + k] = f32_of(u);
            }
            const float* xi = &x[(size_t)i * TRL_POOL_K];
            n2[i] = trl_pool_chain(xi, xi);
            cls[i] = trl_pool_class(gid[i], g0, G, w[i], n2[i]);
            if (cls[i] == TRL_POOL_SKIPPED) state[0]++;
            if (cls[i] != TRL_POOL_CONTRIBUTES) continue;
            const long long g = (long long)gid[i] - g0;
            const float c = trl_pool_factor(w[i], n2[i]);
            for (int k = 0; k < TRL_POOL_K; k++) A[g * TRL_POOL_K + k] += trl_pool_term(c, xi[k]);
            W[g] += trl_pool_weight(w[i]);
            N[g] += 1;
        }
        printf("%lld\n", state[0]);
        for (long long g = 0; g < G; g++) {
            printf("%lld %lld", N[g], W[g]);
            for (int k = 0; k < TRL_POOL_K; k++) printf(" %lld", A[g * TRL_POOL_K + k]);
            printf("\n");
        }
        std::vector<float> unit((size_t)G * TRL_POOL_K), t(TRL_POOL_K);
        for (int mode = 0; mode < 2; mode++)
            for (long long g = 0; g < G; g++) {
                float weight, cohesion;
                trl_pool_finish_group(mode, A + g * TRL_POOL_K, W[g], N[g], t.data(), &weight, &cohesion);
                if (mode == TRL_POOL_UNIT) memcpy(&unit[(size_t)g * TRL_POOL_K], t.data(), sizeof(float) * TRL_POOL_K);
                printf("%lld %08x %08x", N[g], bits_of(weight), bits_of(cohesion));
                for (int k = 0; k < TRL_POOL_K; k++) printf(" %08x", bits_of(t[k]));
                printf("\n");
            }
        std::vector<unsigned long long> key((size_t)G, 0);
        for (long long i = 0; i < m; i++) {
            if (cls[i] != TRL_POOL_CONTRIBUTES) continue;
            const long long g = (long long)gid[i] - g0;
            const float* T = &unit[(size_t)g * TRL_POOL_K];
            const float* xi = &x[(size_t)i * TRL_POOL_K];
            const unsigned long long k = trl_best_key(trl_pool_cosine(trl_pool_chain(T, xi), trl_pool_chain(T, T), n2[i]), i);
            if (k > key[g]) key[g] = k;
        }
        for (long long g = 0; g < G; g++) {
            int32_t index;
            float score;
            trl_best_key_decode(key[g], &index, &score);
            printf("%016llx %d %08x\n", key[g], index, bits_of(score));
        }
    }
    return 0;
}

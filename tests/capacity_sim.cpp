// capacity_sim.cpp -- csrc/trl_capacity.h driven from stdin, for tests/test_capacity_cpu.py (host only, no GPU, no HIP).
// Commands, one per line; floats travel as the decimal value of their 32 bits:
//   new <cap_level> <cap_frame>     a fresh context's capacities with these configured start values
//   hint <t2 bits> <t3 bits>        what trl_debug_batch_capacity sets (0 bits: leave)
//   plan <n> <L> <cells[0..L)>      the attempt's capacities -> "plan L S capF cap_t2 cap_t3 capl[0..L) rec0[0..L)"
//   check <TRL_NFLAGS words>        the feedback of that attempt, on the layout of the last plan
//                                   -> "caps retry resume_stage t2 t3 frame_hint spill_hint lvl_hint[0..32)"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "trl_capacity.h"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static float from_bits(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

int main() {
    CascadeCaps caps;
    CascadePlan plan;
    int cap_level = 2048, cap_frame = 2048, n = 1;
    std::string line, cmd;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "new") {
            caps = CascadeCaps();
            plan = CascadePlan();
            if (!(in >> cap_level >> cap_frame)) return 2;
        } else if (cmd == "hint") {
            uint32_t b[2];
            if (!(in >> b[0] >> b[1])) return 2;
            for (int s = 0; s < 2; s++) if (b[s]) caps.t_per_frame[s] = from_bits(b[s]);
        } else if (cmd == "plan") {
            int L;
            long long cells[32];
            if (!(in >> n >> L) || L < 0 || L > 32 || n < 1) return 2;
            for (int l = 0; l < L; l++) if (!(in >> cells[l])) return 2;
            plan = trl_caps_plan(caps, cap_level, cap_frame, cells, L, n);
            caps.cap_t[0] = plan.cap_t[0]; caps.cap_t[1] = plan.cap_t[1];
            printf("plan %d %d %d %d %d", plan.lay.L, plan.lay.S, plan.capF, plan.cap_t[0], plan.cap_t[1]);
            for (int l = 0; l < L; l++) printf(" %d", plan.lay.capl[l]);
            for (int l = 0; l < L; l++) printf(" %d", plan.lay.rec0[l]);
            printf("\n");
        } else if (cmd == "check") {
            int32_t f[TRL_NFLAGS];
            for (int i = 0; i < TRL_NFLAGS; i++) {
                long long v;
                if (!(in >> v)) return 2;
                f[i] = (int32_t)v;
            }
            const CapsVerdict v = trl_caps_check(caps, f, n, plan.lay);
            if (v.resume_stage != caps.resume_stage) return 3;
            printf("caps %d %d %" PRIu32 " %" PRIu32 " %" PRIu32 " %llu", v.retry, v.resume_stage, bits(caps.t_per_frame[0]), bits(caps.t_per_frame[1]),
                   bits(caps.frame_hint), (unsigned long long)caps.spill_hint);
            for (int l = 0; l < 32; l++) printf(" %" PRIu32, bits(caps.lvl_hint[l]));
            printf("\n");
        } else {
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}

// Reads one request per line from stdin (tests/test_plan_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS HZ MAX_PC
//   in:  plan mno T M                  out: PC TC bytes end next
// bytes: the plan's bytes(); end: where the plan's last region ends by its offset functions; next: bytes() of the same plan with one frame more.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d %d %d\n", EVAL_LDS_BYTES, EVAL_THREADS, (int)PlanLds::HZ, (int)PlanLds::MAX_PC);
        } else if (!std::strcmp(cmd, "plan")) {
            int mno = 0, T = 0, M = 0, pc = 0, tc = 0;
            if (std::scanf("%d %d %d", &mno, &T, &M) != 3) return 1;
            plan_geometry(mno, T, M, &pc, &tc);
            const PlanLds l(mno, pc, tc);
            const size_t end = EVAL_PAIR_BYTES * (l.plans() + l.pos()) + 4 * ((size_t)l.clear(PlanLds::SETS - 1) + (size_t)pc * PlanLds::HZ);
            std::printf("%d %d %zu %zu %zu\n", pc, tc, l.bytes(), end, PlanLds(mno, pc, tc + 1).bytes());
        } else return 2;
    }
    return 0;
}

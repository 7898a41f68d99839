// Reads one request per line from stdin (tests/test_plan_cond_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS MAX_PC ITEMS
//   in:  cond K t_cond M               out: PC TC rows bytes end next
// bytes: the plan's bytes(); end: where the plan's last region ends by its offset functions; next: bytes() of the same plan with one frame more.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d %d %d\n", EVAL_LDS_BYTES, EVAL_THREADS, (int)PlanCondLds::MAX_PC, (int)PlanCondLds::ITEMS);
        } else if (!std::strcmp(cmd, "cond")) {
            int K = 0, T = 0, M = 0, pc = 0, tc = 0, rows = 0;
            if (std::scanf("%d %d %d", &K, &T, &M) != 3) return 1;
            plan_cond_geometry(K, T, M, &pc, &tc, &rows);
            const PlanCondLds l(K, pc, tc, rows);
            const size_t end = EVAL_PAIR_BYTES * (l.plans() + l.rows()) + 4 * ((size_t)l.count() + (size_t)pc);
            std::printf("%d %d %d %zu %zu %zu\n", pc, tc, rows, l.bytes(), end, PlanCondLds(K, pc, tc + 1, rows).bytes());
        } else return 2;
    }
    return 0;
}

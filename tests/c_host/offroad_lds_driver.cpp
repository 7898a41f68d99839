// Reads one request per line from stdin (tests/test_offroad_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS
//   in:  off mno T Mh Mw               out: TC staged bytes end field
// TC, staged: offroad_geometry's; bytes: bytes() of the plan the launcher sizes the LDS by; end: where the plan's last region ends by its offset
// functions; field: the byte offset of the staged field.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d\n", EVAL_LDS_BYTES, EVAL_THREADS);
        } else if (!std::strcmp(cmd, "off")) {
            int mno = 0, T = 0, Mh = 0, Mw = 0, tc = 0, staged = 0;
            if (std::scanf("%d %d %d %d", &mno, &T, &Mh, &Mw) != 4) return 1;
            offroad_geometry(mno, T, Mh, Mw, &tc, &staged);
            const OffLds l(mno, tc, staged ? Mh * Mw : 0);
            const size_t field = EVAL_PAIR_BYTES * (l.c.pos() + l.c.grad()) + 4 * l.field_words();
            std::printf("%d %d %zu %zu %zu\n", tc, staged, l.bytes(), field + (size_t)4 * l.cells, field);
        } else return 2;
    }
    return 0;
}

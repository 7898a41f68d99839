// Reads one request per line from stdin (tests/test_collision_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS
//   in:  coll mno T                    out: TC bytes end next park
// bytes: the plan's bytes(); end: where the plan's last region ends by its offset functions; next: bytes() of the same plan with one frame more;
// park: the row stride of the two slot-major parks.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d\n", EVAL_LDS_BYTES, EVAL_THREADS);
        } else if (!std::strcmp(cmd, "coll")) {
            int mno = 0, T = 0;
            if (std::scanf("%d %d", &mno, &T) != 2) return 1;
            const int tc = coll_chunk_frames(mno, T);
            const CollLds l(mno, tc);
            const size_t end = EVAL_PAIR_BYTES * (l.pos() + l.grad()) + 4 * (l.unit_words() + (size_t)CollLds::UNIT_WORDS);
            std::printf("%d %zu %zu %zu %d\n", tc, l.bytes(), end, CollLds(mno, tc + 1).bytes(), l.park_stride());
        } else return 2;
    }
    return 0;
}

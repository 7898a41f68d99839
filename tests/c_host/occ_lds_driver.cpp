// Reads one request per line from stdin (tests/test_occ_lds.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                          out: EVAL_LDS_BYTES EVAL_THREADS ENTRIES
//   in:  occ K frames Oh Ow until        out: ok KC FC rows bands bytes end
// frames: the frames of a sample one workgroup walks at most (1 in mode AT, the largest horizon in mode UNTIL).  ok: the geometry accepted the
// shape (else the rest of the line is zeros); bytes: the plan's bytes(); end: where the plan's last region ends by its offset functions.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d %d\n", EVAL_LDS_BYTES, EVAL_THREADS, (int)OccLds::ENTRIES);
        } else if (!std::strcmp(cmd, "occ")) {
            int K = 0, frames = 0, Oh = 0, Ow = 0, until = 0, kc = 0, fc = 0, rows = 0;
            if (std::scanf("%d %d %d %d %d", &K, &frames, &Oh, &Ow, &until) != 5) return 1;
            if (!occupancy_geometry(K, frames, Oh, Ow, until, &kc, &fc, &rows)) {
                std::printf("0 0 0 0 0 0 0\n");
                continue;
            }
            const OccLds l(rows * Ow, kc * fc, until);
            const size_t end = 4 * (l.chunk(OccLds::CHUNK_REGIONS - 1) + (size_t)l.ent);
            std::printf("1 %d %d %d %d %zu %zu\n", kc, fc, rows, eval_chunks(Oh, rows), l.bytes(), end);
        } else return 2;
    }
    return 0;
}

// Reads one request per line from stdin (tests/test_scene_modes_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS DESIRE_MODES_MAX DESIRE_MODES_MAX_ITERS
//   in:  scene mno K T n               out: ok SC bytes end fixed slot
// ok: scene_modes_geometry's answer (0: the per-window words and one slot do not fit; SC, bytes and end are then zeros); bytes: the plan's
// bytes(); end: where the plan's last region ends by its offset functions; fixed, slot: SceneModesLds::fixed_bytes and slot_bytes.
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d %d %d\n", EVAL_LDS_BYTES, EVAL_THREADS, DESIRE_MODES_MAX, DESIRE_MODES_MAX_ITERS);
        } else if (!std::strcmp(cmd, "scene")) {
            int mno = 0, K = 0, T = 0, n = 0, sc = 0;
            if (std::scanf("%d %d %d %d", &mno, &K, &T, &n) != 4) return 1;
            const size_t fixed = SceneModesLds::fixed_bytes(K, T, n, mno), slot = SceneModesLds::slot_bytes(K, T, n);
            if (!scene_modes_geometry(mno, K, T, n, &sc)) { std::printf("0 0 0 0 %zu %zu\n", fixed, slot); continue; }
            const SceneModesLds l(T, sc, K, n, mno);
            const size_t end = EVAL_PAIR_BYTES * l.pairs() + 4 * (l.slots() + (size_t)mno);
            std::printf("1 %d %zu %zu %zu %zu\n", sc, l.bytes(), end, fixed, slot);
        } else return 2;
    }
    return 0;
}

// Reads one request per line from stdin (tests/test_modes_cpu.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS DESIRE_MODES_MAX DESIRE_MODES_MAX_ITERS
//   in:  modes mno K T n               out: ok SC G bytes end agent
// ok: modes_geometry's answer (0: one agent does not fit; the rest of the line is then zeros but `agent`); bytes: the plan's bytes(); end: where
// the plan's last region ends by its offset functions; agent: ModesLds::agent_bytes(K, T, n).
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d %d %d\n", EVAL_LDS_BYTES, EVAL_THREADS, DESIRE_MODES_MAX, DESIRE_MODES_MAX_ITERS);
        } else if (!std::strcmp(cmd, "modes")) {
            int mno = 0, K = 0, T = 0, n = 0, sc = 0, g = 0;
            if (std::scanf("%d %d %d %d", &mno, &K, &T, &n) != 4) return 1;
            const size_t agent = ModesLds::agent_bytes(K, T, n);
            if (!modes_geometry(mno, K, T, n, &sc, &g)) { std::printf("0 0 0 0 0 %zu\n", agent); continue; }
            const ModesLds l(T, sc, K, n);
            const size_t end = EVAL_PAIR_BYTES * l.pairs() + 4 * l.slot_words(ModesLds::SLOT_WORDS);
            std::printf("1 %d %d %zu %zu %zu\n", sc, g, l.bytes(), end, agent);
        } else return 2;
    }
    return 0;
}

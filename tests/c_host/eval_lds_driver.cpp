// Reads one request per line from stdin (tests/test_eval_lds.py) and answers from desire_amd/csrc/eval_lds.h:
//   in:  budget                        out: EVAL_LDS_BYTES EVAL_THREADS
//   in:  errors mno K T                out: ok SC KC bytes end smallest
//   in:  kde T                         out: ok SA 0 bytes end smallest
//   in:  select mno K metric t_end     out: ok SC G bytes end smallest
//   in:  recon mno K T                 out: ok SC KC bytes end smallest
//   in:  joint mno T                   out: 1 TC 0 bytes end smallest
// ok: the geometry accepted the shape (else the rest of the line is zeros but `smallest`); bytes: the plan's bytes(); end: where the plan's last
// region ends by its offset functions; smallest: bytes() of the smallest plan of the shape (one row / agent / frame).
#include "eval_lds.h"

#include <cstdio>
#include <cstring>

static void say(bool ok, int a, int b, size_t bytes, size_t end, size_t smallest) {
    if (ok) std::printf("1 %d %d %zu %zu %zu\n", a, b, bytes, end, smallest);
    else std::printf("0 0 0 0 0 %zu\n", smallest);
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        int mno = 0, K = 0, T = 0, metric = 0, t_end = 0, a = 0, b = 0;
        if (!std::strcmp(cmd, "budget")) {
            std::printf("%d %d\n", EVAL_LDS_BYTES, EVAL_THREADS);
        } else if (!std::strcmp(cmd, "errors")) {
            if (std::scanf("%d %d %d", &mno, &K, &T) != 3) return 1;
            const bool ok = sample_errors_geometry(mno, K, T, &a, &b);
            const ErrLds l(T, a, b);
            say(ok, a, b, l.bytes(), 4 * ((size_t)l.e() + (size_t)a * b * l.Tp), ErrLds(T, 1, 1).bytes());
        } else if (!std::strcmp(cmd, "kde")) {
            if (std::scanf("%d", &T) != 1) return 1;
            const bool ok = kde_geometry(T, &a);
            const KdeLds l(T, a);
            say(ok, a, 0, l.bytes(), 4 * ((size_t)l.cm() + (size_t)a * l.Tp), KdeLds(T, 1).bytes());
        } else if (!std::strcmp(cmd, "select")) {
            if (std::scanf("%d %d %d %d", &mno, &K, &metric, &t_end) != 4) return 1;
            const bool ok = select_geometry(mno, K, metric, t_end, &a, &b);
            const SelLds l(SelLds::staged(metric, t_end), a, K);
            say(ok, a, b, l.bytes(), EVAL_PAIR_BYTES * l.pairs() + 4 * (size_t)l.slot_words(SelLds::SLOT_WORDS), SelLds(SelLds::staged(metric, t_end), 1, K).bytes());
        } else if (!std::strcmp(cmd, "recon")) {
            if (std::scanf("%d %d %d", &mno, &K, &T) != 3) return 1;
            const bool ok = recon_geometry(mno, K, T, &a, &b);
            const ReconLds l(T, a, b);
            say(ok, a, b, l.bytes(), EVAL_PAIR_BYTES * (l.rows() + l.slots()) + 4 * l.slots(), ReconLds(T, 1, 1).bytes());
        } else if (!std::strcmp(cmd, "joint")) {
            if (std::scanf("%d %d", &mno, &T) != 2) return 1;
            a = joint_chunk_frames(mno, T);
            const JointLds l(mno, a);
            say(true, a, 0, l.bytes(), EVAL_PAIR_BYTES * l.pairs() + 4 * 2 * (size_t)mno, JointLds(mno, 1).bytes());
        } else return 2;
    }
    return 0;
}

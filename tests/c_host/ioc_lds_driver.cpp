// Reads one request per line from stdin (tests/test_ioc_lds.py) and answers from desire_amd/csrc/ioc_lds.h / ioc_plan.h:
//   in:  lds <plan> H TM bins np mw flag      out: <regions> off(0) .. off(regions)       (off(regions) = bytes(); EV = 16, C = 32)
//   in:  route bf16 training H grid_size mno   out: <forward family> <backward family> ioc_uses_cluster ioc_x6r2_supported
//   in:  fits H bins                           out: ioc_uses_cluster(64, H, bins) ioc_x6r2_supported(64, H, bins)
#include "ioc_plan.h"

#include <cstdio>
#include <cstring>

template <int N>
static void show(const IocLdsRegions<N>& l) {
    std::printf("%d", N);
    for (int r = 0; r <= N; ++r) std::printf(" %d", l.off(r));
    std::printf(" %zu\n", l.bytes());
}
static const char* const FWD[] = {"STEPWISE", "FP32", "FP32_WIDE", "FP32_CLUSTER", "BF16", "BF16_WIDE", "BF16_CLUSTER", "X3", "X3R2", "X6", "X6R2"};
static const char* const BWD[] = {"FP32", "X3", "CLUSTER"};

int main() {
    char cmd[16], plan[32];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "route")) {
            int bf16, training, H, G, mno;
            if (std::scanf("%d %d %d %d %d", &bf16, &training, &H, &G, &mno) != 5) return 1;
            desire_dims d{};
            d.bf16 = bf16; d.H = H; d.grid_size = G; d.mno = mno; d.iters = 1;
            const IocPlan p = ioc_plan(d, training != 0, mno, 0, 4096L * mno);
            std::printf("%s %s %d %d\n", FWD[(int)p.fwd], BWD[(int)p.bwd], (int)ioc_uses_cluster(mno, H, G * G, 0), (int)ioc_x6r2_supported(mno, H, G * G));
            continue;
        }
        if (!std::strcmp(cmd, "fits")) {
            int H, bins;
            if (std::scanf("%d %d", &H, &bins) != 2) return 1;
            std::printf("%d %d\n", (int)ioc_uses_cluster(64, H, bins, 0), (int)ioc_x6r2_supported(64, H, bins));
            continue;
        }
        int H, TM, bins, np, mw, flag;
        if (std::scanf("%31s %d %d %d %d %d %d", plan, &H, &TM, &bins, &np, &mw, &flag) != 7) return 1;
        if (!std::strcmp(plan, "tile")) show(IocLds::tile(H, 16, 32, TM, bins));
        else if (!std::strcmp(plan, "cluster")) show(IocLds::cluster(H, 16, 32, bins));
        else if (!std::strcmp(plan, "step")) show(flag ? IocLds::step_x2(H, 16, 32, bins, mw) : IocLds::step(H, 16, 32, bins, mw));
        else if (!std::strcmp(plan, "bf16")) show(IocHtLds::bf16(H, 16, 32, TM / 32, bins, flag != 0));
        else if (!std::strcmp(plan, "bf16_cluster")) show(IocHtLds::bf16_cluster(H, 16, 32, bins));
        else if (!std::strcmp(plan, "x3")) show(IocHtLds::x3(H, 16, 32, np, bins));
        else if (!std::strcmp(plan, "x6r2")) show(IocHtLds::x6r2(H, 16, 32, bins));
        else if (!std::strcmp(plan, "bwd_tile")) show(IocBwdLds::tile(H, TM, bins));
        else if (!std::strcmp(plan, "bwd_x3")) show(IocBwdLds::x3(H, bins));
        else if (!std::strcmp(plan, "bwd_cluster")) show(IocBwdLds::cluster(H, bins));
        else return 2;
    }
    return 0;
}

// Reads one case per line from stdin and prints the IOC plan of desire_amd/csrc/ioc_plan.h for it (tests/test_ioc_plan.py):
//   in:  bf16 training ioc_form ioc_split H grid_size iters mno train_fp32_mask view_mno gpt R capacity
//   out: forward nspl backward padded cluster bin_split
#include "ioc_plan.h"

#include <cstdio>

static const char* fwd_name(IocFwd f) {
    switch (f) {
        case IocFwd::STEPWISE: return "STEPWISE";
        case IocFwd::FP32: return "FP32";
        case IocFwd::FP32_WIDE: return "FP32_WIDE";
        case IocFwd::FP32_CLUSTER: return "FP32_CLUSTER";
        case IocFwd::BF16: return "BF16";
        case IocFwd::BF16_WIDE: return "BF16_WIDE";
        case IocFwd::BF16_CLUSTER: return "BF16_CLUSTER";
        case IocFwd::X3: return "X3";
        case IocFwd::X3R2: return "X3R2";
        case IocFwd::X6: return "X6";
        case IocFwd::X6R2: return "X6R2";
    }
    return "?";
}

int main() {
    int bf16, training, form, split, H, G, iters, mno, mask, vmno, gpt, cap;
    long R;
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %ld %d", &bf16, &training, &form, &split, &H, &G, &iters, &mno, &mask, &vmno, &gpt, &R, &cap) == 13) {
        desire_dims d{};
        d.bf16 = bf16; d.ioc_form = form; d.ioc_split = split; d.H = H; d.grid_size = G; d.iters = iters; d.mno = mno; d.train_fp32_mask = mask;
        const IocPlan p = ioc_plan(d, training != 0, vmno, gpt, R, [&](int) { return cap; });
        std::printf("%s %d %s %d %d %d\n", fwd_name(p.fwd), p.nspl, p.bwd == IocBwd::CLUSTER ? "CLUSTER" : p.bwd == IocBwd::X3 ? "X3" : "FP32",
                    p.padded, p.cluster(), p.nspl > 1);
    }
    return 0;
}

// ioc_plan.h -- which IOC kernel family serves a call, decided in one place: ioc_plan() below.  Host code only and free of HIP headers
// (tests/test_ioc_plan.py compiles it with g++); the launchers launch the family they are asked for and pick only template instances.
#pragma once
#include "../../include/desire_hip.h"
#include "ioc_lds.h"

#include <functional>

// Which IOC form serves (mno, H, bins): the cluster form (32-row tiles exchanging hidden states through global memory) takes every
// group that does not fit ONE workgroup's LDS tile -- more than 64 agents, 64 agents at H = 256, or 64 agents with so many
// social bins (> 25 at H = 128) that the 64-row tile's neighbour masks push it past 160 KB.
inline bool ioc_uses_cluster(int mno, int H, int bins, int variant) {
    if (mno > 64 || (mno == 64 && H == 256) || (variant == 4 && mno >= 64)) return true;
    return mno == 64 && IocLds::tile(H, 16, 32, 64, bins).bytes() > 160 * 1024;
}
// Few tiles (a handful of windows): how many workgroups share one 32-row tile's social bins (k_ioc NSPL), so that the launch covers
// up to 256 CUs instead of one per (scene, k) group.  1 = the plain form.
inline int ioc_bin_split(long R, int mno, int H, int bins, int iters) {
    if (mno > 32 || H > 128 || iters != 1) return 1;
    const long tiles = (R + 31) / 32;
    for (int n = 4; n >= 2; --n)          // (8 per tile measured no faster than 4: what is left of a step is the part every member repeats)
        if (tiles * n <= 256 && bins >= n) return n;
    return 1;
}
// split-bf16 form on 32-row tiles (kernels_x3.hip): groups that divide 32, H = 64 / 128
inline bool ioc_x3_supported(int mno, int H, int bins) { return mno >= 1 && mno <= 32 && 32 % mno == 0 && (H == 64 || H == 128) && bins <= 64; }
// ... on 64-row tiles, two row blocks per wave (kernels_x6r2.hip): its LDS tile must fit 160 KB
inline bool ioc_x6r2_supported(int mno, int H, int bins) {
    if (!((H == 64 || H == 128) && mno >= 1 && ((mno <= 32 && 32 % mno == 0) || mno == 64))) return false;
    return IocHtLds::x6r2(H, 16, 32, bins).bytes() <= 160 * 1024;
}
// split-bf16 BPTT (kernels_bwd_x3.hip): groups of up to 32 agents, H = 64 / 128
inline bool ioc_bwd_x3_supported(int mno, int H) { return mno <= 32 && (H == 64 || H == 128); }

// STEPWISE: k_ioc_step per step (desire_ioc_refine, no view form); FP32*: k_ioc on 32 / 64-row tiles, k_ioc_cl; BF16* (dims.bf16 = 1): k_ioc_bf16
// with one / two row blocks, k_ioc_bf16_cl; X3 / X6 (two / three pieces): k_ioc_x3 on 32-row tiles, X3R2 / X6R2: k_ioc_x6r2 on 64-row tiles
enum class IocFwd { STEPWISE, FP32, FP32_WIDE, FP32_CLUSTER, BF16, BF16_WIDE, BF16_CLUSTER, X3, X3R2, X6, X6R2 };
enum class IocBwd { FP32, X3, CLUSTER };   // k_ioc_bwd, k_ioc_bwd_x3, k_ioc_bwd_cl

struct IocPlan {
    IocFwd fwd = IocFwd::FP32;
    int nspl = 1;                          // > 1: FP32 with the bins of a tile split over nspl workgroups (k_ioc NSPL; the bin-split exchange)
    IocBwd bwd = IocBwd::FP32;             // the training BPTT of the same view
    bool padded = false;                   // padded tiles (slot class 10) are served for this handle
    bool cluster() const { return fwd == IocFwd::FP32_CLUSTER || fwd == IocFwd::BF16_CLUSTER; }     // needs the cluster exchange
    bool fp32_weights() const { return fwd == IocFwd::FP32 || fwd == IocFwd::FP32_WIDE || fwd == IocFwd::FP32_CLUSTER; }
};

// The plan of one IOC launch sequence over a view of mno slots per window (gpt > 0: padded tiles of gpt groups, R rows) of a handle with
// dims d.  The step-wise test looks at the handle's own d.mno; everything else at the view.  capacity(n) = the resident workgroups of the
// n-member bin-split kernel on this device (ioc_bin_split_capacity, a device query); left empty, the bin split is not considered.
inline IocPlan ioc_plan(const desire_dims& d, bool training, int mno, int gpt, long R, const std::function<int(int)>& capacity = {}) {
    IocPlan p;
    const int H = d.H, B = d.grid_size * d.grid_size, v = d.ioc_form;
    // padded tiles: k_ioc<TM = 32> and k_ioc_x3 in the forward, k_ioc_bwd / k_ioc_bwd_x3 in training; fp32 BPTT under dims.bf16 = 2 has none
    p.padded = v == DESIRE_IOC_AUTO && H <= 128 && (d.bf16 == 0 || d.bf16 == 2) && (!training || d.bf16 == 0 || !(d.train_fp32_mask & 4));
    // the BPTT of a view: the cluster test passes ioc_form 0 (the training forward passes the handle's ioc_form)
    p.bwd = ioc_uses_cluster(mno, H, B, 0) ? IocBwd::CLUSTER
          : d.bf16 == 2 && !(d.train_fp32_mask & 4) && ioc_bwd_x3_supported(mno, H) ? IocBwd::X3 : IocBwd::FP32;
    // step-wise: scenes of 160 .. 256 agents (beyond the cluster form's 128-bit neighbour masks), and -- dims.bf16 = 2 / 3, inference, the form
    // left to the handle -- H = 256 (BASELINE configs[3]: no persistent split kernel, the bin-split accumulators do not fit eight waves' registers)
    // with split operands instead of the fp32 fallback: 16.1 -> 9.1 ms (three products) / 12.7 ms (six) at configs[3]'s per-GPU shape.  (Groups
    // of 96 / 128 agents at H <= 128 were measured too: 34.4 vs 34.9 ms with three products, SLOWER with six -- they keep the fp32 cluster kernel.)
    const bool split_mode = (d.bf16 == 2 || d.bf16 == 3) && !training;
    const bool split_served = ioc_x3_supported(d.mno, H, B) || (d.mno == 64 && ioc_x6r2_supported(d.mno, H, B));
    if (d.mno > 128 || (split_mode && !split_served && H == 256 && v == DESIRE_IOC_AUTO)) { p.fwd = IocFwd::STEPWISE; return p; }
    // split forms: groups of up to 32 agents on 32-row tiles (also the training-mode forward); inference on groups of 64 agents runs the
    // 64-row tile of kernels_x6r2.hip (one group per tile) in either piece count
    const bool wide64 = mno == 64 && !training && ioc_x6r2_supported(mno, H, B);
    const bool x3 = d.bf16 == 2 && (ioc_x3_supported(mno, H, B) || wide64 || (gpt > 0 && ioc_x3_supported(32, H, B)));
    const bool x6 = d.bf16 == 3 && (ioc_x3_supported(mno, H, B) || wide64);          // six-product form: inference only
    // bf16: one workgroup holds groups of up to 64 agents; 96 / 128 (and 64 when ioc_form 4 / 6 asks for it) run the cluster form
    const bool cluster = d.bf16 == 1 ? (mno > 64 || (mno == 64 && (v == DESIRE_IOC_CLUSTER || v == DESIRE_IOC_CLUSTER_BINS)))
                                     : (!(x3 || x6) || training) && ioc_uses_cluster(mno, H, B, v);
    // 32-row tiles (two workgroups per CU at H <= 128) whenever whole (scene, k) groups fit; ioc_form 2 forces 64 rows (A/B); H = 256: 32 rows
    const bool wide = mno > 32 || v == DESIRE_IOC_TILE64;
    const IocFwd fp32 = cluster ? IocFwd::FP32_CLUSTER : wide && H != 256 ? IocFwd::FP32_WIDE : IocFwd::FP32;
    if (training && d.bf16 != 1) p.fwd = x3 ? IocFwd::X3 : fp32;        // training-mode forward (saves): split operands or the fp32 kernels
    else if (x6)         // 64-row tiles for groups of 64 and for launches of >= 256 of them (ioc_form 13: never, 14: always); fewer leave CUs idle
        p.fwd = (mno > 32 || (v != DESIRE_IOC_X6_TILE32 && ((R + 63) / 64 >= 256 || v == DESIRE_IOC_X6_TILE64))) && ioc_x6r2_supported(mno, H, B) ? IocFwd::X6R2 : IocFwd::X6;
    else if (x3)         // two pieces: the 64-row tile only for groups of 64 (for <= 32 it was measured slower: 30.7 vs 29.1 ms at 512 windows)
        p.fwd = mno > 32 && ioc_x6r2_supported(mno, H, B) ? IocFwd::X3R2 : IocFwd::X3;
    else if (d.bf16 == 1) p.fwd = cluster ? IocFwd::BF16_CLUSTER : wide ? IocFwd::BF16_WIDE : IocFwd::BF16;       // (inference only: the caller refuses training)
    else p.fwd = fp32;
    // a handful of windows, fp32 inference: the bins of every tile split over several workgroups (dims.ioc_split = 1: off, 2 .. 4: a cap).
    // The members of a tile wait for each other, so the split is taken only when the whole launch is co-resident on THIS device
    // (occupancy x compute units, not a constant: a partition with fewer CUs falls back to the plain form).
    if (p.fwd == IocFwd::FP32 && d.bf16 == 0 && !training && d.ioc_split != 1 && v == DESIRE_IOC_AUTO && gpt == 0 && capacity) {
        int n = ioc_bin_split(R, mno, H, B, d.iters);
        if (n > 1 && d.ioc_split > 1) n = n < d.ioc_split ? n : d.ioc_split;
        const long tiles = (R + 31) / 32;
        while (n > 1 && (long)capacity(n) < tiles * n) --n;
        p.nspl = n;
    }
    return p;
}

// modes_fit.h -- the steps of the mode-fit contract (include/desire_hip.h: desire_fit_modes, desire_fit_scene_modes), each stated once for
// k_fit_modes and k_fit_scene_modes: the seed check, the weights, the distance of a row to a mean, the nearest mode, the member sums of the
// update and of the covariance, the Gaussian term at the ground truth, the mixture's value of a frame and the horizon emit.  At mno == 1 the two
// calls return the same bits because both kernels are built from these functions; what differs between them comes in as a functor (how a weight
// is indexed, how "k is a member of mode i" is asked) or stays in the kernel: every decision about lanes, LDS and barriers.  k_fit_scene_modes
// writes two of the steps out instead (the nearest mode, the value of a frame: its file header says why); a change to either is made there too.
// The arguments the two calls share (ModesFitParams, ModesFitOut) are kernels.h's, where the entry points fill them.
//
// RULE: this header is made of product-sums, and the contract rounds every operation once.  So it sets `#pragma clang fp contract(off)` itself,
// for everything after it in the including file, and is included AFTER eval_tile.h (which must stay under the default contraction: it says
// why) and by kernels_modes.hip and kernels_scene_modes.hip only -- a file that needs contraction below its includes must not include it.
#pragma once
#include "eval_tile.h"

#pragma clang fp contract(off)

constexpr float MODES_LOG_2PI = 1.8378770664093453f;

// ---- the seed check: the first n entries of an order row are in 0 .. K-1 and distinct.  sink(i, entry, bad so far) sees every entry.
template <class Sink>
__device__ __forceinline__ int modes_seed_check(const int32_t* ord, int n, int K, Sink sink) {
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const int c = ord[i];
        bad |= (unsigned)c >= (unsigned)K;
        for (int j = 0; j < i; ++j) bad |= ord[j] == c;
        sink(i, c, bad);
    }
    return bad;
}

// ---- the weights in place of the K scores w[] (desire_kde_nll's step 1, eval_weight_stats): 1 / K each, or e_k / sum.  One lane.
__device__ __forceinline__ void modes_weights(bool scored, int K, float* w) {
    const EvalWeightStats ws = eval_weight_stats(scored, K, [&](int k) { return w[k]; }, [&](int k, float e) { w[k] = e; });
    const float u = 1.f / (float)K;
    for (int k = 0; k < K; ++k) w[k] = ws.uniform ? u : w[k] / ws.sum;
}

// ---- the distance of row y to mean m over the frames t < t_end, in increasing t
__device__ __forceinline__ float modes_row_dist(const float2* y, const float2* m, int t_end, float ux, float uy) {
    float D = 0.f;
#pragma unroll 4
    for (int t = 0; t < t_end; ++t) {
        const float a = (y[t].x - m[t].x) * ux, b = (y[t].y - m[t].y) * uy;
        D = D + (a * a + b * b);
    }
    return D;
}

// ---- the nearest of the n modes at distances D(i): strict, so ties go to the lower i; a NaN is never chosen; -1 when every D(i) is a NaN
template <class Dist>
__device__ __forceinline__ int modes_nearest(int n, Dist D) {
    int best = -1;
    float bd = 0.f;
    for (int i = 0; i < n; ++i) {
        const float d = D(i);
        if (d == d && (best < 0 || d < bd)) { best = i; bd = d; }
    }
    return best;
}

// ---- the member sums, over the K rows ys[k * stride] in increasing k; in(k): row k is a member, w(k): its weight.  Branch-free, so that the
// LDS reads of several k are in flight at once: a row of another mode adds 0.f, which leaves a sum that started at +0.f bit for bit as it is
// (it is never -0.f), and the row is selected away, not multiplied (it may hold a NaN).
struct ModesSum { float W, x, y; int c; };       // mass, the mean's numerator, members (W and c only with MASS)
template <bool MASS, class In, class Wt>
__device__ __forceinline__ ModesSum modes_member_sum(const float2* ys, int stride, int K, In in, Wt w) {
    ModesSum r{0.f, 0.f, 0.f, 0};
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const bool mine = in(k);
        const float wk = w(k);
        const float2 y = ys[(size_t)k * stride];
        if constexpr (MASS) { r.W = r.W + (mine ? wk : 0.f); r.c += mine; }
        r.x = r.x + (mine ? wk * y.x : 0.f); r.y = r.y + (mine ? wk * y.y : 0.f);
    }
    return r;
}
// the covariance (xx, yy, xy) about the mean m of a mode of mass W > 0 (the caller's test: without mass the triple is zeros)
struct ModesCov { float xx, yy, xy; };
template <class In, class Wt>
__device__ __forceinline__ ModesCov modes_member_cov(const float2* ys, int stride, int K, float2 m, float ux, float uy, float W, float var_floor,
                                                     In in, Wt w) {
    ModesCov r{0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const bool mine = in(k);
        const float wk = w(k);
        const float2 y = ys[(size_t)k * stride];
        const float cx = (y.x - m.x) * ux, cy = (y.y - m.y) * uy;
        r.xx = r.xx + (mine ? wk * (cx * cx) : 0.f); r.yy = r.yy + (mine ? wk * (cy * cy) : 0.f); r.xy = r.xy + (mine ? wk * (cx * cy) : 0.f);
    }
    r.xx = r.xx / W + var_floor; r.yy = r.yy / W + var_floor; r.xy = r.xy / W;
    return r;
}

// ---- the Gaussian term of one (mode, slot, t) at the ground truth (gx, gy).  modes_cov_usable: the covariance is not degenerate (det comes
// back); then modes_gauss_term: q = quad / det and hl = 0.5f * logf(det); modes_chain continues a mode's log-likelihood L by it
struct ModesTerm { float q, hl; };
__device__ __forceinline__ bool modes_cov_usable(float cxx, float cyy, float cxy, float& det) {
    det = cxx * cyy - cxy * cxy;
    return det > DESIRE_KDE_MIN_DET_RATIO * cxx * cyy;
}
__device__ __forceinline__ ModesTerm modes_gauss_term(float cxx, float cyy, float cxy, float det, float mx, float my, float gx, float gy, float ux,
                                                      float uy) {
    const float dx = (mx - gx) * ux, dy = (my - gy) * uy, c2 = 2.f * cxy;
    return ModesTerm{(-0.5f * ((cyy * (dx * dx) - c2 * (dx * dy)) + cxx * (dy * dy))) / det, 0.5f * logf(det)};
}
__device__ __forceinline__ float modes_chain(float L, const ModesTerm& g) { return ((L + g.q) - MODES_LOG_2PI) - g.hl; }

// ---- the value of a counted frame: the log-sum-exp over the usable modes in increasing i (mode(i, l): mode i is usable, and then its
// log-likelihood l), never below log_floor, which is also the value when none is usable.  k_fit_scene_modes divides by the counted slots first
template <class Mode>
__device__ __forceinline__ float modes_frame_value(int n, float log_floor, Mode mode) {
    float v = log_floor, M = -INFINITY, l = 0.f;
    bool any = false;
    for (int i = 0; i < n; ++i)
        if (mode(i, l)) { M = fmaxf(M, l); any = true; }
    if (any) {
        float S = 0.f;
        for (int i = 0; i < n; ++i)
            if (mode(i, l)) S = S + expf(l - M);
        const float r = M + logf(S);
        if (r > log_floor) v = r;
    }
    return v;
}

// ---- one lane walks a row of frame values: o[hi] = (-mean, -last) over the counted frames up to horizon hi, zeros where none is counted
__device__ __forceinline__ void modes_emit_nll(const float* counted, const float* val, const int* hzs, int n_h, float* o) {
    eval_horizon_walk(counted, val, hzs, n_h,
                      [&](int hi, float sum, float last, int np) { o[2 * hi] = np ? -(sum / (float)np) : 0.f; o[2 * hi + 1] = np ? -last : 0.f; });
}

// kernels_kde.hip -- KDE log-likelihood of the ground truth under an agent's K samples (desire_kde_nll; the contract, operation by operation,
// is in include/desire_hip.h).
//
//   k_kde_weights  one lane per agent: the K weights (softmax of the scores, or 1 / K), written once in the score layout, and (den, h2)
//   k_kde_nll      one workgroup = SA whole agents.  A lane owns one (agent, t) pair: for one (window, k) Y is contiguous over (slot, t), so a wave
//                  reads 512 contiguous bytes per sample, at a stride of mno * T_pred * 2 floats between samples.  Up to 24 samples the lane keeps
//                  its K differences and weights in registers (Y comes from HBM once, three passes over registers); beyond, every pass re-reads
//                  them -- a workgroup's share of Y is a few hundred KiB and stays in L2.  The frame values go to LDS; after the barrier one lane
//                  per agent walks its frames and writes the two columns of every horizon.
//
// The weight statistics of the scores, the horizon list and its walk are eval_tile.h's; the LDS plan is eval_lds.h's.
// No atomics, no host synchronisation, horizons by value: a result is a fixed sequence of fp32 operations per (agent, t), so it does not depend on
// the grid or on the rest of the batch, and the call can be captured in a graph.
#include "eval_tile.h"

#pragma clang fp contract(off)                 // the contract rounds every operation once (after the includes: eval_tile.h says why)

namespace {

constexpr float KD_LOG_2PI = 1.8378770664093453f;

__global__ __launch_bounds__(EVAL_THREADS) void k_kde_weights(const float* __restrict__ score, float* __restrict__ w, float* __restrict__ st, int A,
                                                            int mno, int K) {
    const int a = blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (a >= A) return;
    const int scene = a / mno, slot = a - scene * mno;
    const size_t row0 = (size_t)scene * K * mno + slot;            // row of sample k: row0 + k * mno
    const EvalWeightStats ws = eval_weight_stats(score != nullptr, K, [&](int k) { return score[row0 + (size_t)k * mno]; }, [](int, float) {});
    const float u = 1.f / (float)K;
    float den = 0.f, s2 = 0.f;
    bool one = false;
    for (int k = 0; k < K; ++k) {
        const float wk = ws.uniform ? u : expf(score[row0 + (size_t)k * mno] - ws.mx) / ws.sum;
        w[row0 + (size_t)k * mno] = wk;
        den += wk * (1.f - wk);
        s2 += wk * wk;
        one = one || wk == 1.f;
    }
    const float n_eff = 1.f / s2;
    st[2 * (size_t)a] = one ? 0.f : den;                            // (a weight of exactly 1: degenerate, as den <= 0 is)
    st[2 * (size_t)a + 1] = powf(n_eff, -1.f / 3.f);
}

// KC > 0: K <= KC, the lane's differences and weights live in registers.  KC == 0: any K, re-read in every pass.
template <int KC>
__global__ __launch_bounds__(EVAL_THREADS) void k_kde_nll(const float* __restrict__ Y, const float* __restrict__ fut, const float* __restrict__ w,
                                                        const float* __restrict__ st, float* __restrict__ out, float* __restrict__ frame, int A,
                                                        int mno, int K, int T, int SA, int vec, float sx, float sy, float ux, float uy,
                                                        float log_floor, RankHz hz) {
    extern __shared__ float kd_sm[];
    __shared__ int hzs[8];
    const KdeLds L(T, SA);
    const int Tp = L.Tp;
    float* val = kd_sm + L.val();
    float* cm = kd_sm + L.cm();
    const int tid = threadIdx.x;
    const int a0 = blockIdx.x * SA, na = min(SA, A - a0);
    eval_stage_horizons(hzs, hz);

    for (int i = tid; i < na * T; i += EVAL_THREADS) {
        const int s = i / T, t = i - s * T, a = a0 + s;
        const int scene = a / mno, slot = a - scene * mno;
        const float* f = fut + (((size_t)scene * T + t) * mno + slot) * 3;
        const bool counted = f[0] != 0.f;
        float v = 0.f;
        if (counted) {
            const float gx = f[1] * sx, gy = f[2] * sy;
            const size_t row0 = (size_t)scene * K * mno + slot;
            const float* yp = Y + (row0 * T + t) * 2;               // sample k: + k * ystride
            const size_t ystride = (size_t)mno * T * 2;
            const float* wp = w + row0;                             // sample k: + k * mno
            const float den = st[2 * (size_t)a], h2 = st[2 * (size_t)a + 1];
            auto diff = [&](int k, float& dx, float& dy) {
                const float* p = yp + (size_t)k * ystride;
                float y0, y1;
                if (vec) { const float2 y = *reinterpret_cast<const float2*>(p); y0 = y.x; y1 = y.y; }
                else { y0 = p[0]; y1 = p[1]; }
                dx = (y0 - gx) * ux; dy = (y1 - gy) * uy;
            };
            v = log_floor;
            float mx = 0.f, my = 0.f, cxx = 0.f, cyy = 0.f, cxy = 0.f;
            if constexpr (KC > 0) {
                float dx[KC], dy[KC], wk[KC];
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < K) { diff(k, dx[k], dy[k]); wk[k] = wp[(size_t)k * mno]; }
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < K) { mx += wk[k] * dx[k]; my += wk[k] * dy[k]; }
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    if (k < K) {
                        const float cx = dx[k] - mx, cy = dy[k] - my;
                        cxx += wk[k] * (cx * cx); cyy += wk[k] * (cy * cy); cxy += wk[k] * (cx * cy);
                    }
                cxx /= den; cyy /= den; cxy /= den;
                const float det = cxx * cyy - cxy * cxy;
                if (den > 0.f && det > DESIRE_KDE_MIN_DET_RATIO * cxx * cyy) {
                    const float dd = det * h2, c2 = 2.f * cxy;
                    float M = -INFINITY, S = 0.f;
#pragma unroll
                    for (int k = 0; k < KC; ++k)
                        if (k < K) {
                            const float q = (-0.5f * ((cyy * (dx[k] * dx[k]) - c2 * (dx[k] * dy[k])) + cxx * (dy[k] * dy[k]))) / dd;
                            dx[k] = q;
                            M = fmaxf(M, q);
                        }
#pragma unroll
                    for (int k = 0; k < KC; ++k)
                        if (k < K) S += wk[k] * expf(dx[k] - M);
                    const float l = M + logf(S) - KD_LOG_2PI - 0.5f * logf(det) - logf(h2);
                    if (l > log_floor) v = l;
                }
            } else {
                for (int k = 0; k < K; ++k) {
                    float dx, dy; diff(k, dx, dy);
                    const float wk = wp[(size_t)k * mno];
                    mx += wk * dx; my += wk * dy;
                }
                for (int k = 0; k < K; ++k) {
                    float dx, dy; diff(k, dx, dy);
                    const float wk = wp[(size_t)k * mno];
                    const float cx = dx - mx, cy = dy - my;
                    cxx += wk * (cx * cx); cyy += wk * (cy * cy); cxy += wk * (cx * cy);
                }
                cxx /= den; cyy /= den; cxy /= den;
                const float det = cxx * cyy - cxy * cxy;
                if (den > 0.f && det > DESIRE_KDE_MIN_DET_RATIO * cxx * cyy) {
                    const float dd = det * h2, c2 = 2.f * cxy;
                    auto quad = [&](int k) {
                        float dx, dy; diff(k, dx, dy);
                        return (-0.5f * ((cyy * (dx * dx) - c2 * (dx * dy)) + cxx * (dy * dy))) / dd;
                    };
                    float M = -INFINITY, S = 0.f;
                    for (int k = 0; k < K; ++k) M = fmaxf(M, quad(k));
                    for (int k = 0; k < K; ++k) S += wp[(size_t)k * mno] * expf(quad(k) - M);
                    const float l = M + logf(S) - KD_LOG_2PI - 0.5f * logf(det) - logf(h2);
                    if (l > log_floor) v = l;
                }
            }
        }
        val[s * Tp + t] = v;
        cm[s * Tp + t] = counted ? 1.f : 0.f;
        if (frame) frame[(size_t)a * T + t] = v;
    }
    __syncthreads();

    const int n_h = hz.n;
    for (int s = tid; s < na; s += EVAL_THREADS) {
        float* o = out + (size_t)(a0 + s) * n_h * 2;
        eval_horizon_walk(cm + s * Tp, val + s * Tp, hzs, n_h, [&](int hi, float sum, float last, int np) {
            o[2 * hi] = np ? -(sum / (float)np) : 0.f;
            o[2 * hi + 1] = np ? -last : 0.f;
        });
    }
}

}  // namespace

// step 1 alone, for a caller that weighs the samples itself (desire_occupancy): the same kernel into the same scratch
void launch_kde_weights(const EvalIn& in, const KdeOut& o, hipStream_t s) {
    const int A = in.n_scenes * in.mno;
    hipLaunchKernelGGL(k_kde_weights, dim3((A + EVAL_THREADS - 1) / EVAL_THREADS), dim3(EVAL_THREADS), 0, s, in.score, o.w, o.st, A, in.mno, in.K);
}

void launch_kde_nll(const EvalIn& in, const RankHz& hz, const EvalScale& sc, float log_floor, const KdeOut& o, hipStream_t s) {
    int SA = 1;
    if (!kde_geometry(in.T, &SA)) return;                             // (refused by the caller before it gets here)
    launch_kde_weights(in, o, s);
    const int A = in.n_scenes * in.mno;
    const size_t lds = KdeLds(in.T, SA).bytes();
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 7) == 0;
    const dim3 grid((A + SA - 1) / SA), block(EVAL_THREADS);
#define KDE_LAUNCH(KK)                                                                                                                         \
    hipLaunchKernelGGL(k_kde_nll<KK>, grid, block, lds, s, in.Y, in.fut, o.w, o.st, o.out, o.frame, A, in.mno, in.K, in.T, SA, vec, sc.sx, sc.sy, \
                       sc.ux, sc.uy, log_floor, hz)
    if (in.K <= 8) KDE_LAUNCH(8);
    else if (in.K <= 24) KDE_LAUNCH(24);
    else KDE_LAUNCH(0);
#undef KDE_LAUNCH
}

// kernels_rank.hip -- what consumes the IOC score on the device: the per-agent order of the K samples by score, the gather of the
// n_top best-scored trajectories, and the errors of the paper's protocol (top-1 by score and best of the top n, per horizon).
//
//   k_rank_select    one wave per agent: rank by counting (an integer path, bit-exact), write order [A,K], copy the n_top best rows
//   k_sample_errors  streams Y once and writes a table [R, n_h, 2] = (ADE_h, FDE_h) of every sample, plus the number of counted
//                    frames [A, n_h] of every agent
//   k_ranked_pick    reads the table through the order: [A, n_h, 4]
//
// The streaming loop, the order rule, the pick and the horizon walk are eval_tile.h's; the LDS plan and the chunking are eval_lds.h's.
// No atomics, no host synchronisation, horizons by value: every result is a fixed sequence of fp32 operations per (row, horizon), so
// it does not depend on the grid or on the rest of the batch, and the calls can be captured in a graph.
// This file is compiled with the compiler's default contraction (the table's bits are defined by it: kernels_joint.hip reads the table).
#include "eval_tile.h"

namespace {

constexpr int RK_BATCH = 4;                    // 16-byte loads a lane has in flight

// rank_k = #{ j : s_j before s_k } (eval_before: a strict total order, so the ranks are a permutation of 0 .. K-1)
__global__ __launch_bounds__(64) void k_rank_select(const float* __restrict__ score, const float* __restrict__ Y, int32_t* __restrict__ order,
                                                    float* __restrict__ top_Y, float* __restrict__ top_score, int mno, int K, int T,
                                                    int n_top) {
    extern __shared__ float rk_sm[];
    float* s = rk_sm;
    int* ord = reinterpret_cast<int*>(rk_sm + K);
    const int a = blockIdx.x, lane = threadIdx.x;
    const int scene = a / mno, slot = a - scene * mno;
    const size_t row0 = (size_t)scene * K * mno + slot;            // row of sample k: row0 + k * mno
    for (int k = lane; k < K; k += 64) s[k] = score[row0 + (size_t)k * mno];
    __syncthreads();
    for (int k = lane; k < K; k += 64) {
        const float sk = s[k];
        int r = 0;
        for (int j = 0; j < K; ++j) r += eval_before(s[j], j, sk, k) ? 1 : 0;
        ord[r] = k;
        order[(size_t)a * K + r] = k;
    }
    if (!top_Y && !top_score) return;
    __syncthreads();
    const int T2 = 2 * T;
    for (int j = 0; j < n_top; ++j) {
        const int k = ord[j];
        if (top_score && lane == 0) top_score[(size_t)a * n_top + j] = s[k];
        if (top_Y) {
            const float* src = Y + (row0 + (size_t)k * mno) * T2;
            float* dst = top_Y + ((size_t)a * n_top + j) * T2;
            for (int i = lane; i < T2; i += 64) dst[i] = src[i];
        }
    }
}

// One workgroup = (window, a chunk of SC slots, a chunk of KC samples).  The ground truth of the slot chunk goes to LDS once
// (fut [n, T, mno, 3] is contiguous over the slots of a frame), then the rows of the chunk -- contiguous in Y over (slot, t) for one
// (window, k), and over k as well when the chunk holds every slot -- are streamed and each (row, t) pair leaves its error in LDS.  After
// the barrier one lane per row walks its T errors and writes (ADE_h, FDE_h) at each horizon.
__global__ __launch_bounds__(EVAL_THREADS) void k_sample_errors(const float* __restrict__ Y, const float* __restrict__ fut,
                                                                float* __restrict__ tab, int32_t* __restrict__ cnt, int mno, int K, int T,
                                                                int SC, int KC, int n_sc, int n_kc, int vec, float sx, float sy, float ux,
                                                                float uy, RankHz hz) {
    extern __shared__ float rk_sm[];
    __shared__ int hzs[8];
    const ErrLds L(T, SC, KC);
    const int Tp = L.Tp;
    float* gm = rk_sm + L.gm();
    float* gx = rk_sm + L.gx();
    float* gy = rk_sm + L.gy();
    float* eL = rk_sm + L.e();
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int kc = b % n_kc; b /= n_kc;
    const int sc = b % n_sc;
    const int scene = b / n_sc;
    const int slot0 = sc * SC, ns = min(SC, mno - slot0), k0 = kc * KC, nk = min(KC, K - k0);
    eval_stage_horizons(hzs, hz);
    const int w3 = ns * 3;
    for (int i = tid; i < T * w3; i += EVAL_THREADS) {
        const int t = i / w3, rem = i - t * w3, s = rem / 3, c = rem - 3 * s;
        const float v = fut[(((size_t)scene * T + t) * mno + slot0) * 3 + rem];
        const int o = s * Tp + t;
        if (c == 0) gm[o] = v != 0.f ? 1.f : 0.f;
        else if (c == 1) gx[o] = __fmul_rn(v, sx);
        else gy[o] = __fmul_rn(v, sy);
    }
    __syncthreads();

    // segments of rows that are contiguous in Y: the whole chunk when it holds every slot, else one per sample
    const bool whole = ns == mno;
    const int n_seg = whole ? 1 : nk, seg_rows = whole ? nk * ns : ns;
    eval_stream<RK_BATCH>(
        Y, vec, n_seg, seg_rows * T, T, [&](int sg) { return EvalSeg{(((size_t)scene * K + k0 + sg) * mno + slot0) * T, sg * seg_rows}; },
        [&](int row0, int rl, int t, float y0, float y1) {
            const int g = (rl % ns) * Tp + t;
            const float dx = (y0 - gx[g]) * ux, dy = (y1 - gy[g]) * uy;
            eL[(row0 + rl) * Tp + t] = sqrtf(dx * dx + dy * dy);
        });
    __syncthreads();

    const int n_h = hz.n;
    for (int rr = tid; rr < nk * ns; rr += EVAL_THREADS) {
        const int kk = rr / ns, s = rr - kk * ns;
        const size_t row = ((size_t)scene * K + k0 + kk) * mno + slot0 + s;
        float* trow = tab + row * n_h * 2;
        int32_t* crow = (k0 + kk == 0) ? cnt + ((size_t)scene * mno + slot0 + s) * n_h : nullptr;
        eval_horizon_walk(gm + s * Tp, eL + (size_t)rr * Tp, hzs, n_h, [&](int hi, float sum, float last, int np) {
            trow[2 * hi] = np ? sum / (float)np : 0.f;
            trow[2 * hi + 1] = last;
            if (crow) crow[hi] = np;
        });
    }
}

// out [A, n_h, 4] = eval_pick through the order; zeros without a counted frame.
__global__ __launch_bounds__(EVAL_THREADS) void k_ranked_pick(const float* __restrict__ tab, const int32_t* __restrict__ cnt,
                                                              const int32_t* __restrict__ order, float* __restrict__ out, int A, int mno,
                                                              int K, int n_h, int n_top) {
    const size_t idx = (size_t)blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (idx >= (size_t)A * n_h) return;
    const int a = (int)(idx / n_h), hi = (int)(idx - (size_t)a * n_h);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt[idx] > 0) {
        const int scene = a / mno, slot = a - scene * mno;
        o = eval_pick(order + (size_t)a * K, n_top, [&](int k) {
            k = min(max(k, 0), K - 1);                                        // (a caller's buffer: never an index outside the table)
            return tab + ((((size_t)scene * K + k) * mno + slot) * n_h + hi) * 2;
        });
    }
    float* op = out + idx * 4;
    op[0] = o.x; op[1] = o.y; op[2] = o.z; op[3] = o.w;
}

}  // namespace

void launch_rank_select(const EvalIn& in, int n_top, const RankOut& o, hipStream_t s) {
    hipLaunchKernelGGL(k_rank_select, dim3(in.n_scenes * in.mno), dim3(64), (size_t)in.K * 8, s, in.score, in.Y, o.order, o.top_Y, o.top_score, in.mno,
                       in.K, in.T, n_top);
}

// The table alone: tab [R, hz.n, 2] and cnt [A, hz.n] (desire_joint_metrics sums the same rows per (window, k)).
void launch_sample_errors(const EvalIn& in, const RankHz& hz, const EvalScale& sc, const ErrOut& o, hipStream_t s) {
    int SC = 1, KC = 1;
    if (!sample_errors_geometry(in.mno, in.K, in.T, &SC, &KC)) return;         // (refused by the caller before it gets here)
    const int n_sc = eval_chunks(in.mno, SC), n_kc = eval_chunks(in.K, KC);
    const int vec = (reinterpret_cast<uintptr_t>(in.Y) & 15) == 0;
    hipLaunchKernelGGL(k_sample_errors, dim3((unsigned)((size_t)in.n_scenes * n_sc * n_kc)), dim3(EVAL_THREADS), ErrLds(in.T, SC, KC).bytes(), s, in.Y,
                       in.fut, o.tab, o.cnt, in.mno, in.K, in.T, SC, KC, n_sc, n_kc, vec, sc.sx, sc.sy, sc.ux, sc.uy, hz);
}

void launch_ranked_errors(const EvalIn& in, const int32_t* order, int n_top, const RankHz& hz, const EvalScale& sc, const ErrOut& o, hipStream_t s) {
    int SC = 1, KC = 1;
    if (!sample_errors_geometry(in.mno, in.K, in.T, &SC, &KC)) return;         // (refused by the caller before it gets here)
    launch_sample_errors(in, hz, sc, o, s);
    const size_t n = (size_t)in.n_scenes * in.mno * hz.n;
    hipLaunchKernelGGL(k_ranked_pick, dim3((unsigned)((n + EVAL_THREADS - 1) / EVAL_THREADS)), dim3(EVAL_THREADS), 0, s, o.tab, o.cnt, order, o.out,
                       in.n_scenes * in.mno, in.mno, in.K, hz.n, n_top);
}
